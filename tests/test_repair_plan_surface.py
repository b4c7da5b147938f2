"""CPU-side checks of the pattern plans (fec_repair_plan_new, fec_repair_plan_free,
fec_repair_batch_planned, Decoder.repair_plan / decode_plan): the exports, the
validation that runs before any GPU work and its order, NULL safety, the Python
preconditions and the ZFEC_HIP_MIXED_FUSED knob.  No kernel launches here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

torch = pytest.importorskip("torch")

NONE = capi.FEC_REPAIR_NONE


def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_repair_plan_new", "fec_repair_plan_free", "fec_repair_batch_planned"} <= exported
    L = capi.lib()
    assert len(L.fec_repair_plan_new.argtypes) == 7 and L.fec_repair_plan_new.restype is ctypes.c_int
    assert len(L.fec_repair_plan_free.argtypes) == 1 and L.fec_repair_plan_free.restype is None
    assert len(L.fec_repair_batch_planned.argtypes) == 12 and L.fec_repair_batch_planned.restype is ctypes.c_int
    assert hasattr(capi.Code, "repair_plan") and hasattr(capi.RepairPlan, "repair_batch")
    assert hasattr(capi.RepairPlan, "close")
    assert hasattr(zfec_amd.Decoder, "repair_plan") and hasattr(zfec_amd.Decoder, "decode_plan")
    assert hasattr(zfec_amd.RepairPlan, "repair_batch") and hasattr(zfec_amd.RepairPlan, "decode_batch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zfec_hip.h")).read()
    assert "typedef struct fec_repair_plan fec_repair_plan_t;" in header


# ---- fec_repair_plan_new: validation before any GPU work ------------------------------------

def plan_new(code, present, targets, ntargets=None, npatterns=None, present_null=False, targets_null=False,
             code_null=False, plan_null=False, device=-1):
    """(status, message, plan pointer)."""
    L = capi.lib()
    nt = len(targets[0]) if ntargets is None else ntargets
    out = ctypes.c_void_p()
    st = L.fec_repair_plan_new(
        None if code_null else code.ptr,
        None if present_null else capi.uint_array([x for p in present for x in p]),
        None if targets_null else capi.uint_array([x for t in targets for x in t]), nt,
        len(present) if npatterns is None else npatterns, device, None if plan_null else ctypes.byref(out))
    return st, L.fec_last_error_message().decode(), out.value


GOOD = dict(present=[[7, 8, 9], [0, 5, 2]], targets=[[0, 1], [9, NONE]])

# One case per item of the documented order.  Every case also carries ALL the
# later items' faults it can, so that reporting a later one first fails.
LATER_TARGETS = [[0, 12], [9, NONE]]           # a target neither < n nor NONE
LATER_DUP = [[7, 8, 9], [5, 5, 2]]             # a duplicate among present
LATER_RANGE = [[7, 8, 10], [0, 5, 2]]          # a present number >= n
ORDER = [
    ("invalid fec_t", dict(code_null=True, present_null=True, targets_null=True, plan_null=True, ntargets=0,
                           npatterns=70000), "invalid fec_t"),
    ("NULL present", dict(present_null=True, targets_null=True, plan_null=True, ntargets=0, npatterns=70000),
     "present is NULL"),
    ("NULL targets", dict(targets_null=True, plan_null=True, ntargets=0, npatterns=70000), "targets is NULL"),
    ("NULL plan", dict(plan_null=True, ntargets=0, npatterns=70000), "plan is NULL"),
    ("ntargets == 0", dict(ntargets=0, npatterns=0), "ntargets is 0"),
    ("ntargets > 32", dict(ntargets=33, npatterns=70000), "ntargets is 33"),
    ("npatterns == 0", dict(npatterns=0, present=LATER_RANGE), "npatterns is 0"),
    ("more than 65536 patterns", dict(npatterns=65537, present=LATER_RANGE), "at most 65536"),
    ("present >= n", dict(present=[[7, 7, 9], [0, 10, 2]], targets=LATER_TARGETS),
     "pattern 1: block number 10 out of range"),
    ("duplicate present", dict(present=LATER_DUP, targets=LATER_TARGETS), "pattern 1: duplicate block number 5"),
    ("bad target", dict(targets=LATER_TARGETS), "pattern 0: target 12 is neither"),
]


@pytest.mark.parametrize("what,kw,match", ORDER, ids=[o[0] for o in ORDER])
def test_validation_order(what, kw, match):
    """Each check fires with every later fault also present, with or without
    a GPU (and with a device that does not exist): validation precedes
    FEC_ENODEV and the device."""
    args = dict(GOOD)
    args.update(kw)
    st, msg, ptr = plan_new(capi.Code(3, 10), device=4096, **args)
    assert st == capi.FEC_EINVAL and match in msg, (what, st, msg)
    assert not ptr


@pytest.mark.parametrize("k,m", [(3, 10), (5, 9), (40, 60)])
def test_nodev_comes_after_every_check(k, m):
    """Valid arguments pass every check; without a GPU the call is FEC_ENODEV,
    with one it makes a plan (k > 32: one without device records)."""
    pres = [list(range(m - k, m)), list(range(k))]
    tg = [[0, NONE, m - 1 - k], [m - 1, 0, 0]]
    st, msg, ptr = plan_new(capi.Code(k, m), pres, tg)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg and not ptr, msg
        st, msg, ptr = plan_new(capi.Code(k, m), pres, [[0, NONE, m], tg[1]])
        assert st == capi.FEC_EINVAL and "target %d is neither" % m in msg
    else:
        assert st == capi.FEC_OK and ptr, msg
        capi.lib().fec_repair_plan_free(ptr)
        st, msg, ptr = plan_new(capi.Code(k, m), pres, tg, device=4096)
        assert st == capi.FEC_EINVAL and "device 4096" in msg and not ptr


def test_null_plan_is_safe():
    L = capi.lib()
    L.fec_repair_plan_free(None)
    L.fec_repair_plan_free(None)
    buf = ctypes.create_string_buffer(256)
    ids = capi.uint_array([0, 0])
    st = L.fec_repair_batch_planned(None, ctypes.addressof(buf), 8, 24, ctypes.addressof(buf), 8, 8,
                                    ctypes.cast(ids, ctypes.c_void_p), 8, 2, None, 0)
    assert st == capi.FEC_EINVAL and "invalid fec_repair_plan_t" in L.fec_last_error_message().decode()
    # memory that is no plan
    st = L.fec_repair_batch_planned(ctypes.addressof(buf), ctypes.addressof(buf), 8, 24, ctypes.addressof(buf), 8, 8,
                                    ctypes.cast(ids, ctypes.c_void_p), 8, 2, None, 0)
    assert st == capi.FEC_EINVAL and "invalid fec_repair_plan_t" in L.fec_last_error_message().decode()


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    with pytest.raises(capi.FecError, match="pattern 0: duplicate block number 8"):
        code.repair_plan([[8, 8, 9]], [[-1]])
    with pytest.raises(capi.FecError, match="pattern 1: target 11 is neither"):
        code.repair_plan(np.array([[7, 8, 9], [3, 1, 2]]), np.array([[-1], [11]]))
    with pytest.raises(capi.FecError, match="one row per pattern"):
        code.repair_plan([[7, 8, 9]], [[1], [2]])
    with pytest.raises(capi.FecError, match=r"\[npatterns, k = 3\]"):
        code.repair_plan([[7, 8]], [[1]])
    closed = capi.RepairPlan(None, 3, 1, 1)
    closed.close()
    closed.close()
    with pytest.raises(capi.FecError, match="the repair plan is closed"):
        closed.repair_batch(0, 8, 24, 0, 8, 8, 0, 8, 2)


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    good = [[7, 8, 9], [0, 5, 2]]
    tg = [[0, 1], [9, -1]]
    with pytest.raises(zfec_amd.Error, match="patterns is required to be a 2-D integer array"):
        dec.repair_plan([7, 8, 9], tg)
    with pytest.raises(zfec_amd.Error, match="targets is required to be a 2-D integer array"):
        dec.repair_plan(good, [0, 1])
    with pytest.raises(zfec_amd.Error, match="patterns is required to be an integer array \\[P, k = 3\\]"):
        dec.repair_plan([p[:2] for p in good], tg)
    with pytest.raises(zfec_amd.Error, match="at least one pattern"):
        dec.repair_plan(np.zeros((0, 3), dtype=np.int64), np.zeros((0, 2), dtype=np.int64))
    with pytest.raises(zfec_amd.Error, match="one row per pattern: 1 rows, 2 patterns"):
        dec.repair_plan(good, tg[:1])
    with pytest.raises(zfec_amd.Error, match="between 1 and 32 block nums per pattern, not 33"):
        dec.repair_plan(good, np.zeros((2, 33), dtype=np.int64))
    with pytest.raises(zfec_amd.Error, match="between 1 and 32 block nums per pattern, not 0"):
        dec.repair_plan(good, np.zeros((2, 0), dtype=np.int64))
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        dec.repair_plan([[7, 8, 10], [0, 5, 2]], tg)
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but one stripe has \\[5, 5, 2\\]"):
        dec.repair_plan(torch.tensor([[7, 8, 9], [5, 5, 2]]), tg)
    with pytest.raises(zfec_amd.Error, match="targets are required to be in .* or -1 \\(none\\), but one was -2"):
        dec.repair_plan(good, [[0, 1], [9, -2]])
    with pytest.raises(zfec_amd.Error, match="decode_plan takes codes of k <= 32, not k = 40"):
        zfec_amd.Decoder(40, 60).decode_plan([list(range(40))])
    with pytest.raises(zfec_amd.Error, match="patterns is required to be an integer array \\[P, k = 3\\]"):
        dec.decode_plan([[1, 2]])


# ---- the knob --------------------------------------------------------------------------------

def test_mixed_fused_knob_is_parsed(knobs):
    """ZFEC_HIP_MIXED_FUSED is re-read by fec_reload_config; any value parses."""
    for v in ("0", "1", "", "x"):
        knobs(ZFEC_HIP_MIXED_FUSED=v)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "zfec_amd", "csrc", "config.cpp")).read()
    assert 'env("ZFEC_HIP_MIXED_FUSED")' in src
    assert "mixed_fused" in open(os.path.join(root, "zfec_amd", "csrc", "config.hpp")).read()
