"""CPU-side checks of the batched repair (fec_repair_batch, fec_repair_rows,
Decoder.repair_batch): the exports, the validation that runs before any GPU
work and its order, the host-side matrices against the CPU oracle, and the
Python preconditions.  No kernel launches here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

torch = pytest.importorskip("torch")

NONE = capi.FEC_REPAIR_NONE


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_repair_batch", "fec_repair_rows"} <= exported
    L = capi.lib()
    assert L.fec_repair_batch.argtypes and L.fec_repair_rows.argtypes
    assert L.fec_repair_batch.restype is ctypes.c_int and L.fec_repair_rows.restype is ctypes.c_int
    assert len(L.fec_repair_batch.argtypes) == 16 and len(L.fec_repair_rows.argtypes) == 5
    assert hasattr(capi.Code, "repair_batch") and hasattr(capi, "repair_rows")
    assert hasattr(zfec_amd.Decoder, "repair_batch")
    assert capi.FEC_REPAIR_NONE == 0xFFFFFFFF
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define FEC_REPAIR_NONE 0xFFFFFFFFu" in open(os.path.join(root, "include", "zfec_hip.h")).read()


# ---- validation before any GPU work ---------------------------------------------------

def repair_call(code, present, targets, ids, ntargets=None, npatterns=None, nstripes=None, src=True, dst=True,
                present_null=False, targets_null=False, ids_null=False, code_null=False, sz=8):
    """fec_repair_batch over pageable host buffers; returns (status, message)."""
    L = capi.lib()
    k = code.k
    nt = len(targets[0]) if ntargets is None else ntargets
    ns = len(ids) if nstripes is None else nstripes
    buf = ctypes.create_string_buffer(max(1, ns) * k * sz)
    obuf = ctypes.create_string_buffer(max(1, ns) * max(1, min(nt, 64)) * sz)
    st = L.fec_repair_batch(
        None if code_null else code.ptr, ctypes.addressof(buf) if src else None, sz, k * sz,
        ctypes.addressof(obuf) if dst else None, sz, max(1, min(nt, 64)) * sz,
        None if present_null else capi.uint_array([x for p in present for x in p]),
        None if targets_null else capi.uint_array([x for t in targets for x in t]), nt,
        len(present) if npatterns is None else npatterns,
        None if ids_null else ctypes.cast(capi.uint_array(ids), ctypes.c_void_p), sz, ns, None, 0)
    return st, L.fec_last_error_message().decode()


GOOD = dict(present=[[7, 8, 9], [0, 5, 2]], targets=[[0, 1], [9, NONE]], ids=[0, 1, 1, 0])

# One case per item of the documented order.  Every case also carries ALL the
# later items' faults it can, so that reporting a later one first fails.
LATER_IDS = [0, 1, 7, 0]                       # a host-side id >= npatterns
LATER_TARGETS = [[0, 12], [9, NONE]]           # a target neither < n nor NONE
LATER_DUP = [[7, 8, 9], [5, 5, 2]]             # a duplicate among present
LATER_RANGE = [[7, 8, 10], [0, 5, 2]]          # a present number >= n
ORDER = [
    ("invalid fec_t", dict(code_null=True, src=False, targets_null=True, ntargets=0, npatterns=70000), "invalid fec_t"),
    ("NULL src", dict(src=False, ntargets=0, npatterns=70000), "NULL buffer"),
    ("NULL dst", dict(dst=False, ntargets=33, npatterns=0), "NULL buffer"),
    ("NULL present", dict(present_null=True, ntargets=0, npatterns=70000), "present is NULL"),
    ("NULL targets", dict(targets_null=True, ntargets=0, npatterns=70000), "targets is NULL"),
    ("ntargets == 0", dict(ntargets=0, npatterns=0, ids_null=True), "ntargets is 0"),
    ("ntargets > 32", dict(ntargets=33, npatterns=70000, ids_null=True), "ntargets is 33"),
    ("npatterns == 0 with stripes", dict(npatterns=0, ids_null=True, present=LATER_RANGE), "npatterns is 0"),
    ("more than 65536 patterns", dict(npatterns=65537, ids_null=True, present=LATER_RANGE), "at most 65536"),
    ("pattern_of NULL, npatterns != 1", dict(ids_null=True, nstripes=4, present=LATER_RANGE, targets=LATER_TARGETS),
     "pattern_of is NULL with 2 patterns"),
    ("present >= n", dict(present=[[7, 7, 9], [0, 10, 2]], targets=LATER_TARGETS, ids=LATER_IDS),
     "pattern 1: block number 10 out of range"),
    ("duplicate present", dict(present=LATER_DUP, targets=LATER_TARGETS, ids=LATER_IDS),
     "pattern 1: duplicate block number 5"),
    ("bad target", dict(targets=LATER_TARGETS, ids=LATER_IDS), "pattern 0: target 12 is neither"),
    ("host id >= npatterns", dict(ids=LATER_IDS), "stripe 2: pattern id 7 out of range"),
]


@pytest.mark.parametrize("what,kw,match", ORDER, ids=[o[0] for o in ORDER])
def test_validation_order(what, kw, match):
    """Each check fires with every later fault also present, on pageable host
    memory, with or without a GPU: validation precedes FEC_ENODEV."""
    args = dict(GOOD)
    args.update(kw)
    st, msg = repair_call(capi.Code(3, 10), **args)
    assert st == capi.FEC_EINVAL and match in msg, (what, st, msg)


@pytest.mark.parametrize("k,m", [(3, 10), (5, 9)])
@pytest.mark.parametrize("with_ids", [True, False])
def test_valid_arguments_on_pageable_host_memory(k, m, with_ids):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host buffers this call does
    not stage.  Neither crashes."""
    if with_ids:
        pres = [list(range(m - k, m)), list(range(k))]
        tg = [[0, NONE, m - 1 - k], [m - 1, 0, 0]]
        st, msg = repair_call(capi.Code(k, m), pres, tg, [0, 1, 1, 0])
    else:
        st, msg = repair_call(capi.Code(k, m), [list(range(m - k, m))], [[0, NONE]], [], ids_null=True, nstripes=3)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        assert st == capi.FEC_EINVAL and "pageable host memory" in msg, msg


def test_nothing_to_do_is_ok_or_nodev():
    """nstripes == 0 and sz == 0 return FEC_OK (after FEC_ENODEV where no GPU is visible)."""
    want = capi.FEC_ENODEV if zfec_amd.device_count() == 0 else capi.FEC_OK
    assert repair_call(capi.Code(3, 10), [[7, 8, 9]], [[0]], [])[0] == want
    assert repair_call(capi.Code(3, 10), [[7, 8, 9]], [[0]], [0, 0], sz=0)[0] == want


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    ids = capi.uint_array([0, 0])
    with pytest.raises(capi.FecError, match="pattern 0: duplicate block number 8"):
        code.repair_batch(ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 8, [[8, 8, 9]], [[-1]],
                          ctypes.addressof(ids), 8, 2)
    with pytest.raises(capi.FecError, match="pattern 1: target 11 is neither"):
        code.repair_batch(ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 8, np.array([[7, 8, 9], [3, 1, 2]]),
                          np.array([[-1], [11]]), ctypes.addressof(ids), 8, 2)
    with pytest.raises(capi.FecError, match="one row per pattern"):
        code.repair_batch(ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 8, [[7, 8, 9]], [[1], [2]],
                          ctypes.addressof(ids), 8, 2)
    with pytest.raises(capi.FecError, match=r"\[npatterns, k = 3\]"):
        code.repair_batch(ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 8, [[7, 8]], [[1]],
                          ctypes.addressof(ids), 8, 2)


# ---- fec_repair_rows ---------------------------------------------------------------------

def test_rows_validation():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * (33 * 3))()
    outp = ctypes.cast(out, ctypes.c_void_p)
    ua = capi.uint_array

    def call(present, targets, nt=None, code_ptr=code.ptr, rows=outp):
        st = L.fec_repair_rows(code_ptr, None if present is None else ua(present),
                               None if targets is None else ua(targets), len(targets or []) if nt is None else nt, rows)
        return st, L.fec_last_error_message().decode()

    for args, match in (
            (dict(present=[1, 2, 3], targets=[0], code_ptr=None), "invalid fec_t"),
            (dict(present=None, targets=[0]), "present is NULL"),
            (dict(present=[1, 2, 3], targets=None, nt=1), "targets is NULL"),
            (dict(present=[1, 2, 3], targets=[0], rows=None), "rows is NULL"),
            (dict(present=[1, 2, 3], targets=[0], nt=0), "ntargets is 0"),
            (dict(present=[1, 2, 3], targets=[0] * 33), "ntargets is 33"),
            (dict(present=[3, 4, 10], targets=[0]), "block number 10 out of range"),
            (dict(present=[3, 3, 4], targets=[0]), "duplicate block number 3"),
            (dict(present=[3, 5, 4], targets=[0, 10]), "target 10 is neither")):
        st, msg = call(**args)
        assert st == capi.FEC_EINVAL and match in msg, (args, st, msg)
    assert call([1, 2, 3], [0, NONE, 9] + [4] * 29)[0] == capi.FEC_OK  # 32 targets


def gf_matmul(a, b):
    """(r, k) x (k, c) over GF(2^8) with the oracle's multiply."""
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.uint8)
    for i in range(a.shape[0]):
        for j in range(b.shape[1]):
            acc = 0
            for l in range(a.shape[1]):
                acc ^= oracle.gf_mul(int(a[i, l]), int(b[l, j]))
            out[i, j] = acc
    return out


def expected_rows(k, m, present, targets):
    """E[targets] . inverse(E[present]) from the oracle alone.  The oracle's
    decode matrix wants primary i at slot i, so it is built for the present
    set in such an order and its columns are then moved to `present`'s slots."""
    enc = oracle.enc_matrix(k, m)
    ruled = [None] * k
    rest = []
    for b in present:
        if b < k:
            ruled[b] = b
        else:
            rest.append(b)
    for i in range(k):
        if ruled[i] is None:
            ruled[i] = rest.pop()
    dec = oracle.decode_matrix(k, m, ruled)  # row i: primary i from the ruled slots
    rows = np.zeros((len(targets), k), dtype=np.uint8)
    live = [i for i, t in enumerate(targets) if t != NONE]
    if live:
        full = gf_matmul(enc[[targets[i] for i in live]], dec)
        cols = [ruled.index(b) for b in present]
        rows[live] = full[:, cols]
    return rows


def rows_of(code, present, targets):
    return np.frombuffer(capi.repair_rows(code, present, targets), dtype=np.uint8).reshape(len(targets), code.k)


@pytest.mark.parametrize("k,m", [(1, 5), (3, 10), (4, 12), (10, 16), (20, 60)])
def test_rows_against_the_oracle(k, m):
    code = capi.Code(k, m)
    rng = np.random.default_rng(10 * k + m)
    enc = oracle.enc_matrix(k, m)
    for trial in range(6):
        present = rng.permutation(m)[:k].tolist()  # a random set in a random slot order
        absent = [b for b in rng.permutation(m).tolist() if b not in present]
        nt = int(rng.integers(1, min(32, m) + 1))
        targets = rng.integers(0, m, size=nt).tolist()  # drawn from all n numbers: present ones and repeats included
        targets[int(rng.integers(0, nt))] = NONE
        got = rows_of(code, present, targets)
        assert (got == expected_rows(k, m, present, targets)).all(), (present, targets)
        for i, t in enumerate(targets):
            if t == NONE:
                assert not got[i].any(), "a NONE row is all zeros"
            elif t in present:
                unit = np.zeros(k, dtype=np.uint8)
                unit[present.index(t)] = 1
                assert (got[i] == unit).all(), "a present target is a unit row at its slot"
            for j in range(i):
                if targets[j] == t:
                    assert (got[i] == got[j]).all(), "duplicate targets give equal rows"
        # distinct targets disjoint from present: fec_verify_rows of present + targets
        checks = absent[:min(len(absent), 32, 1 + trial)]
        want = np.frombuffer(capi.verify_rows(code, present + checks), dtype=np.uint8).reshape(len(checks), k)
        assert (rows_of(code, present, checks) == want).all(), (present, checks)
        # -1 is taken for FEC_REPAIR_NONE by the binding
        assert (rows_of(code, present, [-1 if t == NONE else t for t in targets]) == got).all()
    # present = 0..k-1 in order gives the encode rows
    every = list(range(m))[:32]
    assert (rows_of(code, list(range(k)), every) == enc[every]).all()
    # a present target and a duplicate, explicitly
    present = rng.permutation(m)[:k].tolist()
    got = rows_of(code, present, [present[-1], present[-1], NONE])
    assert got[0, k - 1] == 1 and got[0].sum() == 1 and (got[0] == got[1]).all() and not got[2].any()


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    ns, sz = 4, 16
    host = torch.zeros((ns, 3, sz), dtype=torch.uint8)
    good = [[7, 8, 9], [0, 5, 2], [9, 1, 4], [3, 2, 1]]
    tg = [[0, 1], [9, -1], [0, 0], [-1, -1]]
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        dec.repair_batch(host, good, tg)
    with pytest.raises(zfec_amd.Error, match="host \\(numpy\\) blocks are not staged"):
        dec.repair_batch(host.numpy(), good, tg)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 3, sz\\]"):
        dec.repair_batch(host.reshape(ns * 3, sz), good, tg)
    with pytest.raises(zfec_amd.Error, match="required to hold 3 blocks per stripe, not 4"):
        dec.repair_batch(torch.zeros((ns, 4, sz), dtype=torch.uint8), good, tg)
    with pytest.raises(zfec_amd.Error, match="blocknums is required to be an integer array \\[nstripes, k\\] = \\[4, 3\\]"):
        dec.repair_batch(host, good[:3], tg)
    with pytest.raises(zfec_amd.Error, match="blocknums is required to be an integer array \\[nstripes, k\\]"):
        dec.repair_batch(host, [p[:2] for p in good], tg)
    with pytest.raises(zfec_amd.Error, match="targets is required to be an integer array \\[nstripes, t\\] = \\[4, t\\]"):
        dec.repair_batch(host, good, tg[:3])
    with pytest.raises(zfec_amd.Error, match="targets is required to be an integer array"):
        dec.repair_batch(host, good, [0, 1, 2, 3])
    with pytest.raises(zfec_amd.Error, match="between 1 and 32 block nums per stripe, not 33"):
        dec.repair_batch(host, good, np.zeros((ns, 33), dtype=np.int64))
    with pytest.raises(zfec_amd.Error, match="between 1 and 32 block nums per stripe, not 0"):
        dec.repair_batch(host, good, np.zeros((ns, 0), dtype=np.int64))
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but one stripe has \\[9, 1, 9\\]"):
        dec.repair_batch(host, [[7, 8, 9], [0, 5, 2], [9, 1, 9], [3, 2, 1]], tg)
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        dec.repair_batch(host, np.array([[7, 8, 9], [0, 5, 2], [10, 1, 4], [3, 2, 1]]), tg)
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 12"):
        dec.repair_batch(host, torch.tensor([[7, 8, 9], [0, 5, 2], [6, 1, 4], [3, 12, 1]]), tg)
    with pytest.raises(zfec_amd.Error, match="targets are required to be in .* or -1 \\(none\\), but one was 10"):
        dec.repair_batch(host, good, [[0, 1], [9, -1], [0, 10], [-1, -1]])
    with pytest.raises(zfec_amd.Error, match="targets are required to be in .* or -1 \\(none\\), but one was -2"):
        dec.repair_batch(host, good, torch.tensor([[0, 1], [9, -2], [0, 0], [-1, -1]]))
    # the tuple form
    with pytest.raises(zfec_amd.Error, match="pattern_of is required to hold nstripes = 4 ids, not 3"):
        dec.repair_batch(host, ([[7, 8, 9], [0, 5, 2]], [0, 1, 1]), [[0], [1]])
    with pytest.raises(zfec_amd.Error, match="pattern_of ids are required to be in \\[0, 1\\]"):
        dec.repair_batch(host, ([[7, 8, 9], [0, 5, 2]], [0, 1, 2, 0]), [[0], [1]])
    with pytest.raises(zfec_amd.Error, match="required to be distinct"):
        dec.repair_batch(host, ([[7, 8, 9], [5, 5, 2]], [0, 1, 1, 0]), [[0], [1]])
    with pytest.raises(zfec_amd.Error, match="one row per pattern: 3 rows, 2 patterns"):
        dec.repair_batch(host, ([[7, 8, 9], [0, 5, 2]], [0, 1, 1, 0]), [[0], [1], [2]])
    # out: wrong shape, dtype, device
    with pytest.raises(zfec_amd.Error, match="out is required to be a uint8 tensor \\[nstripes, t, sz\\] = \\[4, 2, 16\\]"):
        dec.repair_batch(host, good, tg, out=torch.zeros((ns, 3, sz), dtype=torch.uint8))
    with pytest.raises(zfec_amd.Error, match="out is required to be a uint8 tensor"):
        dec.repair_batch(host, good, tg, out=torch.zeros((ns, 2, sz), dtype=torch.int16))
    with pytest.raises(zfec_amd.Error, match="out is required to be a uint8 tensor"):
        dec.repair_batch(host, good, tg, out=np.zeros((ns, 2, sz), dtype=np.uint8))
    with pytest.raises(zfec_amd.Error, match="out is required to be on the blocks' device"):
        dec.repair_batch(host, good, tg, out=torch.zeros((ns, 2, sz), dtype=torch.uint8, device="meta"))
    with pytest.raises(zfec_amd.Error, match="out rows are required to be contiguous along sz"):
        dec.repair_batch(host, good, tg, out=torch.zeros((ns, 2, 2 * sz), dtype=torch.uint8)[:, :, ::2])
