"""CPU-side checks of pair location and correction (fec_locate2_batch,
fec_correct2_batch, fec_locate2_rows, fec_correct2_rows and the Decoder
methods): the exports, the constant, the validation that runs before any GPU
work and its order, the two host-side helpers against the model built from the
CPU oracle (tests/pair_ref.py), the Python preconditions, and the guarantees of
the model itself on the oracle's matrices.  No kernel launches here."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from locate_ref import CLEAN, MANY, inv_table, mul_table, oracle_PQ
from pair_ref import NONE, columns, eligible, pair_index, pair_rows, verdicts2
from test_locate_surface import clean_stripes
from test_verify_surface import ORDERED
from verify_ref import gf_matmul

torch = pytest.importorskip("torch")


def shuffled(m, n, seed):
    return np.random.default_rng(seed).permutation(m)[:n].tolist()


# (k, m, block numbers): c = 4 the minimum; 45 pairs in order and a shuffled seven; 66, 120 and 496 pairs
CODES = [(1, 6, [0, 1, 2, 3, 4]), (3, 10, list(range(10))), (3, 10, shuffled(10, 7, 1)), (4, 12, list(range(12))),
         (10, 16, list(range(16))), (20, 60, shuffled(60, 32, 2))]
IDS = ["%d-%d-nb%d" % (k, m, len(nums)) for k, m, nums in CODES]


def gf_rank(a):
    mul, inv = mul_table(), inv_table()
    a = np.array(a, dtype=np.uint8)
    rank = 0
    for col in range(a.shape[1]):
        rows = np.nonzero(a[rank:, col])[0]
        if len(rows) == 0:
            continue
        piv = rank + rows[0]
        a[[rank, piv]] = a[[piv, rank]]
        a[rank] = mul[inv[a[rank, col]]][a[rank]]
        for r in range(a.shape[0]):
            if r != rank and a[r, col]:
                a[r] ^= mul[a[r, col]][a[rank]]
        rank += 1
        if rank == a.shape[0]:
            break
    return rank


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_locate2_batch", "fec_correct2_batch", "fec_locate2_rows", "fec_correct2_rows"} <= exported
    L = capi.lib()
    P, SZ, U, UP = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint)
    assert list(L.fec_locate2_batch.argtypes) == list(L.fec_locate_batch.argtypes)
    assert list(L.fec_correct2_batch.argtypes) == list(L.fec_correct_batch.argtypes)
    assert list(L.fec_locate2_rows.argtypes) == [P, UP, SZ, U, U, P]
    assert list(L.fec_correct2_rows.argtypes) == [P, UP, SZ, U, U, UP, P]
    for name in ("fec_locate2_batch", "fec_correct2_batch", "fec_locate2_rows", "fec_correct2_rows"):
        assert getattr(L, name).restype is ctypes.c_int
    for name in ("locate2_batch", "correct2_batch"):
        assert hasattr(capi.Code, name) and hasattr(zfec_amd.Decoder, name)
    assert hasattr(capi, "locate2_rows") and hasattr(capi, "correct2_rows")


def test_constant():
    assert capi.FEC_LOCATE_NONE == NONE == 0xFFFFFFFC
    assert np.array([NONE], dtype=np.uint32).view(np.int32)[0] == zfec_amd.LOCATE_NONE == -4
    assert "LOCATE_NONE" in zfec_amd.__all__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zfec_hip.h")).read()
    assert "#define FEC_LOCATE_NONE" in header and "0xFFFFFFFCu" in header
    for name in ("fec_locate2_batch", "fec_correct2_batch", "fec_locate2_rows", "fec_correct2_rows"):
        assert "int %s(" % name in header


# ---- validation before any GPU work ---------------------------------------------------

BATCH = ["fec_locate2_batch", "fec_correct2_batch"]


def batch_call(fn, code, nums, src=True, nums_null=False, mask=True, code_null=False, ns=2, sz=8):
    """One of the two calls over pageable host buffers; returns (status,
    message, the 2 * ns culprit words).  `mask` stands for culprit, as in the
    verify table."""
    L = capi.lib()
    nb = len(nums)
    buf = ctypes.create_string_buffer(max(1, ns * nb * sz))
    words = (ctypes.c_uint * max(1, 2 * ns))(*([0xA5A5A5A5] * max(1, 2 * ns)))
    st = getattr(L, fn)(None if code_null else code.ptr, ctypes.addressof(buf) if src else None, sz, nb * sz,
                        None if nums_null else capi.uint_array(nums), nb, sz, ns,
                        ctypes.addressof(words) if mask else None, None, 0)
    return st, L.fec_last_error_message().decode(), list(words), bytes(buf)


@pytest.mark.parametrize("fn", BATCH)
@pytest.mark.parametrize("kw,match", ORDERED)
def test_validation_order(fn, kw, match):
    """The verify call's table: the same checks in the same order, `culprit` in
    place of `mismatch` and, for the correcting call, `blocks` in place of
    `src`."""
    kw = dict(kw)
    st, msg, _, _ = batch_call(fn, capi.Code(3, 10), kw.pop("nums"), **kw)
    match = match.replace("mismatch", "culprit")
    if match == "src" and fn == "fec_correct2_batch":
        match = "blocks"
    assert st == capi.FEC_EINVAL and match in msg, msg


@pytest.mark.parametrize("fn", BATCH)
def test_valid_arguments_on_pageable_host_memory(fn):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host blocks this call does not
    stage.  Neither crashes, neither writes a verdict or a block byte."""
    for k, m, nums in ((3, 10, list(range(10))), (3, 10, [9, 4, 0, 7]), (10, 16, list(range(16)))):
        st, msg, words, buf = batch_call(fn, capi.Code(k, m), nums)
        if zfec_amd.device_count() == 0:
            assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
        else:
            assert st == capi.FEC_EINVAL and "pageable host memory" in msg and "does not stage" in msg, msg
            assert fn in msg, msg
        assert words == [0xA5A5A5A5] * 4 and not any(buf)


@pytest.mark.parametrize("fn", BATCH)
def test_validation_precedes_enodev_and_empty_calls(fn):
    st, msg, _, _ = batch_call(fn, capi.Code(3, 10), [0, 1, 2, 12], ns=0)
    assert st == capi.FEC_EINVAL and "block number 12 out of range" in msg, msg
    st, msg, words, _ = batch_call(fn, capi.Code(3, 10), list(range(10)), ns=0)
    assert st == (capi.FEC_OK if zfec_amd.device_count() else capi.FEC_ENODEV), msg
    assert words == [0xA5A5A5A5]


def test_capi_wrappers_raise():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w = (ctypes.c_uint * 8)()
    for call in (code.locate2_batch, code.correct2_batch):
        with pytest.raises(capi.FecError, match="duplicate block number 8"):
            call(ctypes.addressof(b), 8, 32, [8, 8, 9, 1], 8, 2, ctypes.addressof(w))
        with pytest.raises(capi.FecError, match="nothing to check"):
            call(ctypes.addressof(b), 8, 24, [7, 8, 9], 8, 2, ctypes.addressof(w))
        with pytest.raises(capi.FecError, match="culprit is NULL"):
            call(ctypes.addressof(b), 8, 32, [7, 8, 9, 1], 8, 2, 0)


# ---- fec_locate2_rows / fec_correct2_rows ---------------------------------------------------

@pytest.mark.parametrize("k,m,nums", CODES, ids=IDS)
def test_locate2_rows_properties(k, m, nums):
    """For every pair: N has rank c - 2, N . p_a = N . p_b = 0 and N . p_h != 0
    for every other slot h, so N . s == 0 exactly on span(p_a, p_b)."""
    code = capi.Code(k, m)
    nb, c = len(nums), len(nums) - k
    P, _ = oracle_PQ(k, m, tuple(nums))
    M = columns(P)
    for a, b in itertools.combinations(range(nb), 2):
        raw = capi.locate2_rows(code, nums, a, b)
        assert len(raw) == (c - 2) * c
        N = np.frombuffer(raw, dtype=np.uint8).reshape(c - 2, c)
        assert gf_rank(N) == c - 2, (a, b)
        hit = gf_matmul(N, M).any(axis=0)
        assert hit.tolist() == [h not in (a, b) for h in range(nb)], (a, b)


@pytest.mark.parametrize("k,m,nums", CODES, ids=IDS)
def test_correct2_rows_equal_repair_rows(k, m, nums):
    """For every pair: the sources are the k lowest slots outside the pair, and
    the rows are fec_repair_rows on those sources and, independently, the
    oracle's check rows for them."""
    code = capi.Code(k, m)
    nb = len(nums)
    for a, b in itertools.combinations(range(nb), 2):
        sources, rows = capi.correct2_rows(code, nums, a, b)
        want_sources, want = pair_rows(k, m, nums, a, b)
        assert sources == want_sources, (a, b)
        assert rows == capi.repair_rows(code, [nums[j] for j in sources], [nums[a], nums[b]]), (a, b)
        assert rows == want.tobytes(), (a, b)


def test_correct2_rows_with_two_checks():
    """c = 2 and 3 are enough to rebuild a pair (location needs 4)."""
    k, m = 3, 10
    code = capi.Code(k, m)
    for nums in ([7, 2, 9, 0, 4], [1, 8, 3, 6, 0, 5]):
        for a, b in itertools.combinations(range(len(nums)), 2):
            sources, rows = capi.correct2_rows(code, nums, a, b)
            assert rows == capi.repair_rows(code, [nums[j] for j in sources], [nums[a], nums[b]]), (nums, a, b)


def test_rows_einval():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 256)(*([0xA5] * 256))
    outp = ctypes.cast(out, ctypes.c_void_p)
    src = (ctypes.c_uint * 3)()

    def loc(nums, a, b, rows=outp, code_ptr=code.ptr):
        st = L.fec_locate2_rows(code_ptr, capi.uint_array(nums) if nums is not None else None,
                                len(nums) if nums is not None else 4, a, b, rows)
        return st, L.fec_last_error_message().decode()

    def cor(nums, a, b, sources=src, rows=outp, code_ptr=code.ptr):
        st = L.fec_correct2_rows(code_ptr, capi.uint_array(nums) if nums is not None else None,
                                 len(nums) if nums is not None else 4, a, b, sources, rows)
        return st, L.fec_last_error_message().decode()

    for fn in (loc, cor):
        for nums, match in (([3, 4, 5], "nothing to check"), (list(range(10)) + [3], "11 blocks per stripe"),
                            ([3, 4, 10, 1, 0, 2, 5], "block number 10 out of range"),
                            ([3, 3, 4, 5, 6, 7, 8], "duplicate block number 3")):
            st, msg = fn(nums, 0, 1)
            assert st == capi.FEC_EINVAL and match in msg, msg
        assert fn(None, 0, 1)[0] == capi.FEC_EINVAL
        assert fn(list(range(10)), 0, 1, rows=None)[0] == capi.FEC_EINVAL
        assert fn(list(range(10)), 0, 1, code_ptr=None)[0] == capi.FEC_EINVAL
        for a, b in ((1, 1), (2, 1), (0, 10), (10, 11), (9, 0xFFFFFFFF)):
            st, msg = fn(list(range(10)), a, b)
            assert st == capi.FEC_EINVAL and "is no pair of slots a < b < 10" in msg, (a, b, msg)
        assert fn(list(range(10)), 8, 9)[0] == capi.FEC_OK
    assert cor(list(range(10)), 0, 1, sources=None) == (capi.FEC_EINVAL, "sources is NULL")
    st, msg = loc(list(range(6)), 0, 1)
    assert st == capi.FEC_EINVAL and "3 checks per stripe, a pair needs at least 4" in msg, msg
    assert loc(list(range(7)), 0, 1)[0] == capi.FEC_OK
    st, msg = cor(list(range(4)), 0, 1)
    assert st == capi.FEC_EINVAL and "1 checks per stripe, a pair needs at least 2" in msg, msg
    assert cor(list(range(5)), 0, 1)[0] == capi.FEC_OK
    with pytest.raises(capi.FecError, match="is no pair of slots"):
        capi.locate2_rows(code, list(range(10)), 3, 3)
    with pytest.raises(capi.FecError, match="is no pair of slots"):
        capi.correct2_rows(code, list(range(10)), 3, 10)


# ---- Python preconditions ----------------------------------------------------------------

@pytest.mark.parametrize("what", ["locate2_batch", "correct2_batch"])
def test_python_preconditions(what):
    dec = zfec_amd.Decoder(3, 10)
    call = getattr(dec, what)
    ns, sz = 4, 16
    host = torch.zeros((ns, 7, sz), dtype=torch.uint8)
    good = [7, 0, 9, 2, 4, 1, 5]
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 3"):
        call(host, [7, 8, 9])
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 11"):
        call(host, list(range(11)))
    with pytest.raises(zfec_amd.Error, match="required to hold 7 blocks per stripe, not 8"):
        call(torch.zeros((ns, 8, sz), dtype=torch.uint8), good)
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but got \\[7, 0, 9, 0, 4, 1, 5\\]"):
        call(host, [7, 0, 9, 0, 4, 1, 5])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        call(host, [7, 0, 10, 2, 4, 1, 5])
    with pytest.raises(zfec_amd.Error, match="%s takes a device tensor; host \\(numpy\\) blocks are not" % what):
        call(host.numpy(), good)
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        call(host, good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 7, sz\\]"):
        call(host.to(torch.int32), good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 7, sz\\]"):
        call(host.reshape(ns * 7, sz), good)


# ---- the model's guarantees on the oracle's matrices --------------------------------------

GUARANTEE_CODES = [(1, 6, 5), (2, 7, 7), (3, 10, 7), (3, 10, 10), (4, 12, 12), (5, 9, 9), (10, 16, 16), (20, 60, 32)]


@pytest.mark.parametrize("k,m,nb", GUARANTEE_CODES)
def test_model_guarantees(k, m, nb):
    """On shares of the oracle's encode, with c >= 4: every pair of slots
    corrupted at one byte, at different bytes, and overwritten whole gets that
    pair (every 9th pair of the 496 of K=20, to keep this quick); every single
    error gets its slot and NONE, so it never reaches rule 5; a clean stripe
    is (CLEAN, NONE)."""
    sz = 24
    nums = shuffled(m, nb, 3 * k + m)
    c = nb - k
    assert eligible(k, c)
    P, Q = oracle_PQ(k, m, tuple(nums))
    pairs = list(itertools.combinations(range(nb), 2))
    if len(pairs) > 200:
        pairs = pairs[::9]
    rng = np.random.default_rng(17 * k + m)
    ns = 1 + 2 * nb + 3 * len(pairs)
    blocks = clean_stripes(k, m, nums, ns, sz, k * m + 1)
    want = np.full((2, ns), NONE, dtype=np.uint32)
    want[0] = CLEAN
    s = 1
    for j in range(nb):
        blocks[s, j, int(rng.integers(0, sz))] ^= int(rng.integers(1, 256))
        blocks[s + 1, j] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
        want[0, s] = want[0, s + 1] = j
        s += 2
    for a, b in pairs:
        xa, xb = rng.permutation(sz)[:2]
        blocks[s, a, xa] ^= int(rng.integers(1, 256))
        blocks[s, b, xa] ^= int(rng.integers(1, 256))
        blocks[s + 1, a, xa] ^= int(rng.integers(1, 256))
        blocks[s + 1, b, xb] ^= int(rng.integers(1, 256))
        blocks[s + 2, a] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
        blocks[s + 2, b] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
        want[:, s:s + 3] = np.array([[a], [b]])
        s += 3
    got = verdicts2(P, Q, blocks)
    assert (got == want).all(), (nums, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("k,m,nb", [(2, 7, 7), (3, 10, 10), (5, 10, 10), (10, 16, 16)])
def test_model_refuses_triples(k, m, nb):
    """Three blocks corrupt at one byte with c >= 5: (MANY, NONE), for every
    triple of K=3/M=10 and a sample elsewhere."""
    sz = 8
    nums = shuffled(m, nb, 5 * k + m)
    c = nb - k
    assert c >= 5
    P, Q = oracle_PQ(k, m, tuple(nums))
    triples = list(itertools.combinations(range(nb), 3))
    if (k, m) != (3, 10):
        triples = triples[::max(1, len(triples) // 40)]
    rng = np.random.default_rng(k + m)
    blocks = clean_stripes(k, m, nums, len(triples), sz, 3)
    for s, tr in enumerate(triples):
        x = int(rng.integers(0, sz))
        for j in tr:
            blocks[s, j, x] ^= int(rng.integers(1, 256))
    got = verdicts2(P, Q, blocks)
    assert (got[0] == MANY).all() and (got[1] == NONE).all()


def test_model_pair_pass_off():
    """c = 3, and 33 blocks held: two corrupt blocks stay (MANY, NONE)."""
    for k, m, nb in ((3, 10, 6), (20, 60, 33)):
        nums = shuffled(m, nb, nb)
        assert not eligible(k, nb - k)
        P, Q = oracle_PQ(k, m, tuple(nums))
        blocks = clean_stripes(k, m, nums, 3, 16, 9)
        blocks[1, 0, 3] ^= 1
        blocks[1, nb - 1, 9] ^= 2
        blocks[2, 1, 5] ^= 7
        assert verdicts2(P, Q, blocks).tolist() == [[CLEAN, MANY, 1], [NONE, NONE, NONE]]


def test_pair_index_is_lexicographic():
    for nb in (5, 10, 32):
        assert [pair_index(nb, a, b) for a, b in itertools.combinations(range(nb), 2)] == list(range(nb * (nb - 1) // 2))
