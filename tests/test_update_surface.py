"""CPU-side checks of the batched parity update (fec_update_batch,
fec_update_rows, Encoder.update_batch): the exports, the validation that runs
before any GPU work and its order, the host-side coefficients against the CPU
oracle, and the Python preconditions.  No kernel launches here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

torch = pytest.importorskip("torch")

NONE = capi.FEC_UPDATE_NONE


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_update_batch", "fec_update_rows"} <= exported
    L = capi.lib()
    assert L.fec_update_batch.restype is ctypes.c_int and L.fec_update_rows.restype is ctypes.c_int
    assert len(L.fec_update_batch.argtypes) == 16 and len(L.fec_update_rows.argtypes) == 5
    assert hasattr(capi.Code, "update_batch") and hasattr(capi, "update_rows")
    assert hasattr(zfec_amd.Encoder, "update_batch")
    assert capi.FEC_UPDATE_NONE == 0xFFFFFFFF
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zfec_hip.h")).read()
    assert "#define FEC_UPDATE_NONE 0xFFFFFFFFu" in header
    assert "int fec_update_batch(const fec_t* code," in header and "int fec_update_rows(const fec_t* code," in header


# ---- validation before any GPU work ---------------------------------------------------

def update_call(code, block_nums, changed, nchanged=None, num=None, nstripes=None, oldb=False, newb=True, rows=True,
                nums_null=False, changed_null=False, code_null=False, sz=8):
    """fec_update_batch over pageable host buffers; `changed` is a list of
    per-stripe lists.  Returns (status, message)."""
    L = capi.lib()
    nc = len(changed[0]) if nchanged is None else nchanged
    ns = len(changed) if nstripes is None else nstripes
    nb = len(block_nums) if num is None else num
    real_ns, real_nc, real_nb = max(1, len(changed)), max(1, len(changed[0]) if changed else 1), max(1, len(block_nums))
    ibuf = ctypes.create_string_buffer(real_ns * real_nc * sz + 8)
    obuf = ctypes.create_string_buffer(real_ns * real_nc * sz + 8)
    rbuf = ctypes.create_string_buffer(real_ns * real_nb * sz + 8)
    st = L.fec_update_batch(
        None if code_null else code.ptr, ctypes.addressof(obuf) if oldb else None,
        ctypes.addressof(ibuf) if newb else None, sz, real_nc * sz,
        ctypes.addressof(rbuf) if rows else None, sz, real_nb * sz,
        None if nums_null else capi.uint_array(block_nums), nb,
        None if changed_null else ctypes.cast(capi.uint_array([x for row in changed for x in row]), ctypes.c_void_p),
        nc, sz, ns, None, 0)
    return st, L.fec_last_error_message().decode()


GOOD = dict(block_nums=[3, 9, 4, 0], changed=[[0, NONE], [2, 2], [NONE, NONE], [1, 0]])

# One case per item of the documented order.  Every case also carries ALL the
# later items' faults it can, so that reporting a later one first fails.
BAD_CHANGED = [[0, NONE], [2, 3], [NONE, NONE], [1, 0]]   # 8: a host-side number that is neither < k nor NONE
MANY = 2**32                                               # 7: nstripes >= 2^32
DUP = [3, 9, 3, 0]                                         # 5: a duplicate block number
RANGE = [3, 10, 3, 0]                                      # 4: a block number >= n (and a duplicate)
ORDER = [
    ("invalid fec_t", dict(code_null=True, newb=False, num=0, nchanged=0, nstripes=MANY, changed=BAD_CHANGED),
     "invalid fec_t"),
    ("NULL newb", dict(newb=False, num=0, nchanged=0, nstripes=MANY, changed=BAD_CHANGED), "newb is NULL"),
    ("NULL rows", dict(rows=False, num=11, nchanged=5, nstripes=MANY, changed=BAD_CHANGED), "rows is NULL"),
    ("NULL block_nums", dict(nums_null=True, num=0, nchanged=5, nstripes=MANY, changed=BAD_CHANGED),
     "block_nums is NULL"),
    ("NULL changed", dict(changed_null=True, num=0, nchanged=5, nstripes=MANY), "changed is NULL"),
    ("num_block_nums == 0", dict(num=0, block_nums=RANGE, nchanged=0, nstripes=MANY, changed=BAD_CHANGED),
     "num_block_nums is 0"),
    ("num_block_nums > n", dict(num=11, block_nums=RANGE + [1] * 7, nchanged=5, nstripes=MANY, changed=BAD_CHANGED),
     "num_block_nums is 11"),
    ("block number >= n", dict(block_nums=RANGE, nchanged=5, nstripes=MANY, changed=BAD_CHANGED),
     "block number 10 out of range"),
    ("duplicate block number", dict(block_nums=DUP, nchanged=0, nstripes=MANY, changed=BAD_CHANGED),
     "duplicate block number 3"),
    ("nchanged == 0", dict(nchanged=0, nstripes=MANY, changed=BAD_CHANGED), "nchanged is 0"),
    ("nchanged > 4", dict(nchanged=5, nstripes=MANY, changed=BAD_CHANGED), "nchanged is 5"),
    ("nstripes >= 2^32", dict(nstripes=MANY, changed=BAD_CHANGED), "fewer than 2^32"),
    ("bad host-side number", dict(changed=BAD_CHANGED), "stripe 1, slot 1: changed block 3 is neither"),
]


@pytest.mark.parametrize("what,kw,match", ORDER, ids=[o[0] for o in ORDER])
def test_validation_order(what, kw, match):
    """Each check fires with every later fault also present, on pageable host
    memory, with or without a GPU: validation precedes FEC_ENODEV."""
    args = dict(GOOD)
    args.update(kw)
    st, msg = update_call(capi.Code(3, 10), **args)
    assert st == capi.FEC_EINVAL and match in msg, (what, st, msg)


def test_a_number_equal_to_k_is_bad_on_the_host():
    st, msg = update_call(capi.Code(3, 10), [7], [[0], [3]])
    assert st == capi.FEC_EINVAL and "stripe 1, slot 0: changed block 3" in msg, msg
    st, msg = update_call(capi.Code(3, 10), [7], [[0], [0xFFFFFFFE]])
    assert st == capi.FEC_EINVAL and "stripe 1, slot 0: changed block 4294967294" in msg, msg


@pytest.mark.parametrize("k,m", [(3, 10), (20, 24)])
@pytest.mark.parametrize("with_old", [True, False])
def test_valid_arguments_on_pageable_host_memory(k, m, with_old):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host buffers this call does
    not stage.  Neither crashes."""
    nums = list(range(m - 1, -1, -1))  # every block of the code, primaries included
    st, msg = update_call(capi.Code(k, m), nums, [[0, NONE, k - 1, k - 1], [NONE] * 4], oldb=with_old)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        assert st == capi.FEC_EINVAL and "pageable host memory" in msg, msg


def test_nothing_to_do_is_ok_or_nodev():
    """nstripes == 0 and sz == 0 return FEC_OK (after FEC_ENODEV where no GPU is visible)."""
    want = capi.FEC_ENODEV if zfec_amd.device_count() == 0 else capi.FEC_OK
    assert update_call(capi.Code(3, 10), [7, 8], [[0]], nstripes=0)[0] == want
    assert update_call(capi.Code(3, 10), [7, 8], [[0], [1]], sz=0)[0] == want


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    ch = capi.uint_array([0, 5])
    with pytest.raises(capi.FecError, match="duplicate block number 8"):
        code.update_batch(0, ctypes.addressof(b), 8, 8, ctypes.addressof(b), 8, 16, [8, 8], ctypes.addressof(ch), 1, 8, 2)
    with pytest.raises(capi.FecError, match="stripe 1, slot 0: changed block 5"):
        code.update_batch(0, ctypes.addressof(b), 8, 8, ctypes.addressof(b), 8, 16, [8, 9], ctypes.addressof(ch), 1, 8, 2)
    with pytest.raises(capi.FecError, match="newb is NULL"):
        code.update_batch(0, 0, 8, 8, ctypes.addressof(b), 8, 16, [8, 9], ctypes.addressof(ch), 1, 8, 2)


# ---- fec_update_rows ---------------------------------------------------------------------

def test_rows_validation():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 16)()
    outp = ctypes.cast(out, ctypes.c_void_p)

    def call(nums, j, num=None, code_ptr=code.ptr, coefs=outp):
        st = L.fec_update_rows(code_ptr, None if nums is None else capi.uint_array(nums),
                               len(nums or []) if num is None else num, j, coefs)
        return st, L.fec_last_error_message().decode()

    for args, match in (
            (dict(nums=[10, 10], j=3, code_ptr=None), "invalid fec_t"),
            (dict(nums=None, j=3, num=0), "block_nums is NULL"),
            (dict(nums=[10, 10], j=3, coefs=None), "coefs is NULL"),
            (dict(nums=[10, 10], j=3, num=0), "num_block_nums is 0"),
            (dict(nums=[10] * 11, j=3), "num_block_nums is 11"),
            (dict(nums=[4, 10, 4], j=3), "block number 10 out of range"),
            (dict(nums=[4, 5, 4], j=3), "duplicate block number 4"),
            (dict(nums=[4, 5, 6], j=3), "changed block 3 is not a primary")):
        st, msg = call(**args)
        assert st == capi.FEC_EINVAL and match in msg, (args, st, msg)
    assert call(list(range(10)), 2)[0] == capi.FEC_OK


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16), (20, 60), (128, 256)])
def test_rows_against_the_oracle(k, m):
    code = capi.Code(k, m)
    enc = oracle.enc_matrix(k, m)
    rng = np.random.default_rng(100 * k + m)
    js = range(k) if k <= 10 else sorted({0, k - 1} | set(rng.integers(0, k, size=6).tolist()))
    shuffled = rng.permutation(m).tolist()  # every block, primaries included, in a random order
    some = rng.permutation(m)[:max(1, m // 3)].tolist()
    for j in js:
        for nums in (list(range(k, m)), shuffled, some, [j], [k]):
            got = np.frombuffer(capi.update_rows(code, nums, j), dtype=np.uint8)
            assert (got == enc[nums, j]).all(), (j, nums)
        # a primary's row of E is a unit row: 1 for the changed block itself, 0 for every other primary
        unit = np.frombuffer(capi.update_rows(code, list(range(k)), j), dtype=np.uint8)
        assert unit[j] == 1 and unit.sum() == 1
        # parity coefficients are never zero (any square submatrix of the parity rows is regular)
        assert np.frombuffer(capi.update_rows(code, list(range(k, m)), j), dtype=np.uint8).all()
    with pytest.raises(capi.FecError, match="changed block %d is not a primary" % k):
        capi.update_rows(code, [k], k)


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    enc = zfec_amd.Encoder(3, 10)
    ns, sz = 4, 16
    par = torch.zeros((ns, 7, sz), dtype=torch.uint8)
    new = torch.zeros((ns, sz), dtype=torch.uint8)
    new2 = torch.zeros((ns, 2, sz), dtype=torch.uint8)
    ch = [0, 1, -1, 2]
    with pytest.raises(zfec_amd.Error, match="parity is required to be a uint8 device tensor \\[nstripes, r, sz\\]"):
        enc.update_batch(par.numpy(), ch, new)
    with pytest.raises(zfec_amd.Error, match="parity is required to be a uint8 device tensor \\[nstripes, r, sz\\]"):
        enc.update_batch(par.reshape(ns * 7, sz), ch, new)
    with pytest.raises(zfec_amd.Error, match="parity is required to be a uint8 device tensor"):
        enc.update_batch(par.to(torch.int16), ch, new)
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        enc.update_batch(par, ch, new, blocknums=[3, 4, 5, 6, 7, 8, 10])
    with pytest.raises(zfec_amd.Error, match="required to be distinct"):
        enc.update_batch(par, ch, new, blocknums=[3, 4, 5, 6, 7, 8, 3])
    with pytest.raises(zfec_amd.Error, match="one row per block num: 7 rows, 2 block nums"):
        enc.update_batch(par, ch, new, blocknums=[8, 9])
    with pytest.raises(zfec_amd.Error, match="parity rows are required to be contiguous along sz"):
        enc.update_batch(torch.zeros((ns, 7, 2 * sz), dtype=torch.uint8)[:, :, ::2], ch, new)
    with pytest.raises(zfec_amd.Error, match="changed is required to be an integer array .* nstripes = 4, not \\(3,\\)"):
        enc.update_batch(par, ch[:3], new)
    with pytest.raises(zfec_amd.Error, match="changed is required to be an integer array"):
        enc.update_batch(par, [0.5, 1, 2, 0], new)
    with pytest.raises(zfec_amd.Error, match="changed is required to be an integer array"):
        enc.update_batch(par, torch.zeros(ns), new)
    with pytest.raises(zfec_amd.Error, match="changed is required to be an integer array"):
        enc.update_batch(par, np.zeros((ns, 1, 1), dtype=np.int64), new)
    with pytest.raises(zfec_amd.Error, match="between 1 and 4 changed blocks per stripe, not 5"):
        enc.update_batch(par, np.zeros((ns, 5), dtype=np.int64), new)
    with pytest.raises(zfec_amd.Error, match="between 1 and 4 changed blocks per stripe, not 0"):
        enc.update_batch(par, np.zeros((ns, 0), dtype=np.int64), new)
    with pytest.raises(zfec_amd.Error, match="primaries in \\[0, k-1\\] = \\[0, 2\\] or -1 \\(none\\), but one was 3"):
        enc.update_batch(par, [0, 1, 3, 2], new)
    with pytest.raises(zfec_amd.Error, match="or -1 \\(none\\), but one was -2"):
        enc.update_batch(par, torch.tensor([[0, 1], [-1, -2], [0, 0], [1, 1]]), new2)
    with pytest.raises(zfec_amd.Error, match="new is required to be a uint8 tensor \\[nstripes, c, sz\\] = \\[4, 2, 16\\]"):
        enc.update_batch(par, [[0, 1]] * ns, new)
    with pytest.raises(zfec_amd.Error, match="new is required to be a uint8 tensor .* or \\[nstripes, sz\\]"):
        enc.update_batch(par, ch, new2)
    with pytest.raises(zfec_amd.Error, match="new is required to be a uint8 tensor"):
        enc.update_batch(par, ch, new.numpy())
    with pytest.raises(zfec_amd.Error, match="old is required to be a uint8 tensor"):
        enc.update_batch(par, ch, new, old=new.to(torch.int32))
    with pytest.raises(zfec_amd.Error, match="old is required to be on parity's device"):
        enc.update_batch(par, ch, new, old=torch.zeros((ns, sz), dtype=torch.uint8, device="meta"))
    with pytest.raises(zfec_amd.Error, match="not a host tensor"):
        enc.update_batch(par, ch, new, old=new)
