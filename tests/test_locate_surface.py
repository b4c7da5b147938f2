"""CPU-side checks of the batched error location (fec_locate_batch,
fec_locate_rows, Decoder.locate_batch): the exports, the validation that runs
before any GPU work and its order, the host-side matrix Q against the model
built from the CPU oracle, the Python preconditions, and the guarantees of the
model itself on the oracle's matrices.  No kernel launches here."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle
from locate_ref import CLEAN, MANY, UNKNOWN, oracle_PQ, verdicts
from test_verify_surface import ORDERED

torch = pytest.importorskip("torch")

CODES = [(1, 3), (2, 3), (3, 10), (4, 12), (4, 40), (10, 16), (20, 60), (33, 36)]


def bases(k, m, seed):
    """Block numbers of all m slots, the first k the basis: the primaries, an
    all-parity basis (where the code has k parity blocks) and a mixed one."""
    rng = np.random.default_rng(seed)
    out = [list(range(m))]
    if m - k >= k:
        par = (k + rng.permutation(m - k)).tolist()
        out.append(par[:k] + rng.permutation(par[k:] + list(range(k))).tolist())
    while True:
        mixed = rng.permutation(m).tolist()
        primary = [b < k for b in mixed[:k]]
        if k == 1 or (any(primary) and not all(primary)):
            break
    out.append(mixed)
    return out


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_locate_batch", "fec_locate_rows"} <= exported
    L = capi.lib()
    P, SZ, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
    assert list(L.fec_locate_batch.argtypes) == list(L.fec_verify_batch.argtypes)
    assert len(L.fec_locate_batch.argtypes) == 11 and L.fec_locate_batch.argtypes[2] is SZ
    assert L.fec_locate_batch.argtypes[8] is P and L.fec_locate_batch.argtypes[10] is U
    assert list(L.fec_locate_rows.argtypes) == list(L.fec_verify_rows.argtypes)
    assert L.fec_locate_batch.restype is ctypes.c_int and L.fec_locate_rows.restype is ctypes.c_int
    assert hasattr(capi.Code, "locate_batch") and hasattr(capi, "locate_rows")
    assert hasattr(zfec_amd.Decoder, "locate_batch")


def test_constants():
    assert (capi.FEC_LOCATE_CLEAN, capi.FEC_LOCATE_MANY, capi.FEC_LOCATE_UNKNOWN) == (CLEAN, MANY, UNKNOWN)
    assert (CLEAN, MANY, UNKNOWN) == (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD)
    as_i32 = np.array([CLEAN, MANY, UNKNOWN], dtype=np.uint32).view(np.int32).tolist()
    assert as_i32 == [zfec_amd.LOCATE_CLEAN, zfec_amd.LOCATE_MANY, zfec_amd.LOCATE_UNKNOWN] == [-1, -2, -3]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zfec_hip.h")).read()
    for name, val in (("CLEAN", "0xFFFFFFFFu"), ("MANY", "0xFFFFFFFEu"), ("UNKNOWN", "0xFFFFFFFDu")):
        assert "#define FEC_LOCATE_%s" % name in header and val in header


# ---- validation before any GPU work ---------------------------------------------------

def locate_call(code, nums, src=True, nums_null=False, mask=True, code_null=False, ns=2, sz=8):
    """fec_locate_batch over pageable host buffers; returns (status, message,
    the culprit words).  `mask` stands for culprit, as in the verify table."""
    L = capi.lib()
    nb = len(nums)
    buf = ctypes.create_string_buffer(max(1, ns * nb * sz))
    words = (ctypes.c_uint * max(1, ns))(*([0xA5A5A5A5] * max(1, ns)))
    st = L.fec_locate_batch(None if code_null else code.ptr, ctypes.addressof(buf) if src else None, sz, nb * sz,
                            None if nums_null else capi.uint_array(nums), nb, sz, ns,
                            ctypes.addressof(words) if mask else None, None, 0)
    return st, L.fec_last_error_message().decode(), list(words)


@pytest.mark.parametrize("kw,match", ORDERED)
def test_validation_order(kw, match):
    """The verify call's table: the same checks in the same order with the same
    messages, `culprit` in place of `mismatch`."""
    kw = dict(kw)
    st, msg, _ = locate_call(capi.Code(3, 10), kw.pop("nums"), **kw)
    assert st == capi.FEC_EINVAL and match.replace("mismatch", "culprit") in msg, msg


def test_nothing_to_check_with_exactly_k_blocks():
    for nums in ([7, 8, 9], []):
        st, msg, _ = locate_call(capi.Code(3, 10), nums)
        assert st == capi.FEC_EINVAL and "nothing to check" in msg, msg


@pytest.mark.parametrize("k,m,nums", [(3, 10, list(range(10))), (3, 10, [9, 4, 0, 7]), (10, 16, list(range(16)))])
def test_valid_arguments_on_pageable_host_memory(k, m, nums):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host blocks this call does not
    stage.  Neither crashes, neither writes a verdict."""
    st, msg, words = locate_call(capi.Code(k, m), nums)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        assert st == capi.FEC_EINVAL and "pageable host memory" in msg and "does not stage" in msg, msg
    assert words == [0xA5A5A5A5] * 2


def test_validation_precedes_enodev_and_empty_calls():
    """A bad block number is reported whether or not a GPU is visible, also in
    a call without stripes."""
    st, msg, _ = locate_call(capi.Code(3, 10), [0, 1, 2, 12], ns=0)
    assert st == capi.FEC_EINVAL and "block number 12 out of range" in msg, msg


def test_empty_calls():
    """nstripes == 0 returns FEC_OK and touches nothing; sz == 0 returns FEC_OK
    with every verdict CLEAN (with a GPU; FEC_ENODEV without one)."""
    code = capi.Code(3, 10)
    have_gpu = zfec_amd.device_count() > 0
    st, msg, words = locate_call(code, list(range(10)), ns=0)
    assert st == (capi.FEC_OK if have_gpu else capi.FEC_ENODEV), msg
    assert words == [0xA5A5A5A5]
    st, msg, words = locate_call(code, list(range(10)), ns=2, sz=0)
    if have_gpu:
        assert st == capi.FEC_OK and words == [CLEAN] * 2, msg
    else:
        assert st == capi.FEC_ENODEV and words == [0xA5A5A5A5] * 2, msg


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w = (ctypes.c_uint * 4)()
    with pytest.raises(capi.FecError, match="duplicate block number 8"):
        code.locate_batch(ctypes.addressof(b), 8, 32, [8, 8, 9, 1], 8, 2, ctypes.addressof(w))
    with pytest.raises(capi.FecError, match="nothing to check"):
        code.locate_batch(ctypes.addressof(b), 8, 24, [7, 8, 9], 8, 2, ctypes.addressof(w))
    with pytest.raises(capi.FecError, match="culprit is NULL"):
        code.locate_batch(ctypes.addressof(b), 8, 32, [7, 8, 9, 1], 8, 2, 0)


# ---- fec_locate_rows ---------------------------------------------------------------------

def test_rows_validation():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 64)()
    outp = ctypes.cast(out, ctypes.c_void_p)
    for nums, match in (([3, 4, 5], "nothing to check"), (list(range(10)) + [3], "11 blocks per stripe"),
                        ([3, 4, 10, 1], "block number 10 out of range"), ([3, 3, 4, 5], "duplicate block number 3")):
        assert L.fec_locate_rows(code.ptr, capi.uint_array(nums), len(nums), outp) == capi.FEC_EINVAL
        assert match in L.fec_last_error_message().decode()
    assert L.fec_locate_rows(code.ptr, None, 4, outp) == capi.FEC_EINVAL
    assert L.fec_locate_rows(code.ptr, capi.uint_array([1, 2, 3, 4]), 4, None) == capi.FEC_EINVAL
    assert L.fec_locate_rows(None, capi.uint_array([1, 2, 3, 4]), 4, outp) == capi.FEC_EINVAL


def test_rows_with_one_check_write_nothing():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 16)(*([0xA5] * 16))
    outp = ctypes.cast(out, ctypes.c_void_p)
    assert L.fec_locate_rows(code.ptr, capi.uint_array([4, 0, 9, 2]), 4, outp) == capi.FEC_OK
    assert list(out) == [0xA5] * 16
    assert capi.locate_rows(code, [4, 0, 9, 2]) == b""


@pytest.mark.parametrize("k,m", CODES)
def test_rows_against_the_model(k, m):
    """Q of the primaries, an all-parity and a mixed basis with all m - k
    checks, and of 10 random splits of a random permutation: the model's
    Q[i][j] = P[i][j] / P[0][j] from the oracle's P, none of it zero."""
    code = capi.Code(k, m)
    rng = np.random.default_rng(2000 * k + m)
    sets = bases(k, m, 7 * k + m)
    for trial in range(10):
        nb = int(rng.integers(k + 1, m + 1))
        sets.append(rng.permutation(m)[:nb].tolist())
    for nums in sets:
        c = len(nums) - k
        raw = capi.locate_rows(code, nums)
        assert len(raw) == (c - 1) * k
        P, Q = oracle_PQ(k, m, tuple(nums))
        got = np.frombuffer(raw, dtype=np.uint8).reshape(c - 1, k)
        assert (got == Q).all(), nums
        assert got.all(), ("zero entry", nums)
        assert (np.frombuffer(capi.verify_rows(code, nums), dtype=np.uint8).reshape(c, k) == P).all()


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    ns, sz = 4, 16
    host = torch.zeros((ns, 5, sz), dtype=torch.uint8)
    good = [7, 0, 9, 2, 4]
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 3"):
        dec.locate_batch(host, [7, 8, 9])
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 11"):
        dec.locate_batch(host, list(range(11)))
    with pytest.raises(zfec_amd.Error, match="required to hold 5 blocks per stripe, not 6"):
        dec.locate_batch(torch.zeros((ns, 6, sz), dtype=torch.uint8), good)
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but got \\[7, 0, 9, 0, 4\\]"):
        dec.locate_batch(host, [7, 0, 9, 0, 4])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        dec.locate_batch(host, [7, 0, 10, 2, 4])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was -1"):
        dec.locate_batch(host, [7, 0, -1, 2, 4])
    with pytest.raises(zfec_amd.Error, match="locate_batch takes a device tensor; host \\(numpy\\) blocks are not"):
        dec.locate_batch(host.numpy(), good)
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        dec.locate_batch(host, good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 5, sz\\]"):
        dec.locate_batch(host.to(torch.int32), good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 5, sz\\]"):
        dec.locate_batch(host.reshape(ns * 5, sz), good)


# ---- the model's guarantees on the oracle's matrices --------------------------------------

GUARANTEE_CODES = [(1, 3), (2, 4), (3, 10), (4, 12), (5, 8), (10, 16)]


def clean_stripes(k, m, nums, ns, sz, seed):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(k, ns * sz), dtype=np.uint8)
    allb = np.concatenate([data, oracle.encode(k, m, data)])[list(nums)]
    return np.ascontiguousarray(allb.reshape(len(nums), ns, sz).transpose(1, 0, 2))


@pytest.mark.parametrize("k,m", GUARANTEE_CODES)
def test_model_guarantees(k, m):
    """On shares of the oracle's encode, for the three bases with all m - k
    checks: clean stripes are CLEAN; every single-slot corruption (one byte, and
    a whole block of random bytes) is located; every pair of slots corrupted at
    different bytes gives MANY; every pair at one byte gives MANY when c >= 3."""
    sz = 24
    nb, c = m, m - k
    pairs = list(itertools.combinations(range(nb), 2))
    rng = np.random.default_rng(31 * k + m)
    for nums in bases(k, m, k + m):
        P, Q = oracle_PQ(k, m, tuple(nums))
        ns = 2 * nb + 2 * len(pairs) + 1
        blocks = clean_stripes(k, m, nums, ns, sz, k * m)
        want = np.full(ns, CLEAN, dtype=np.uint32)
        s = 1  # stripe 0 stays clean
        for j in range(nb):
            blocks[s, j, int(rng.integers(0, sz))] ^= int(rng.integers(1, 256))
            blocks[s + 1, j] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
            want[s] = want[s + 1] = j
            s += 2
        for a, b in pairs:
            xa, xb = rng.permutation(sz)[:2]
            blocks[s, a, xa] ^= int(rng.integers(1, 256))
            blocks[s, b, xb] ^= int(rng.integers(1, 256))
            want[s] = MANY
            blocks[s + 1, a, xa] ^= int(rng.integers(1, 256))
            blocks[s + 1, b, xa] ^= int(rng.integers(1, 256))
            want[s + 1] = MANY if c >= 3 else 0  # c == 2: past the code's distance, not checked
            s += 2
        got = verdicts(P, Q, blocks)
        check = np.ones(ns, dtype=bool)
        if c < 3:
            check[2 * nb + 2::2] = False
        assert (got[check] == want[check]).all(), (nums, np.argwhere(got != want)[:4].tolist())


def test_model_one_check_is_unknown():
    k, m = 3, 10
    nums = (4, 0, 9, 2)
    P, Q = oracle_PQ(k, m, nums)
    blocks = clean_stripes(k, m, nums, 6, 16, 1)
    for s, j in enumerate(range(4)):
        blocks[s + 1, j, 3 * s] ^= 0x40
    assert verdicts(P, Q, blocks).tolist() == [CLEAN, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN, CLEAN]
