"""CPU-side checks of the batched in-place correction (fec_correct_batch,
fec_correct_rows, Decoder.correct_batch): the exports, the validation that runs
before any GPU work and its order, the host-side correction matrix against the
model built from the CPU oracle (tests/correct_ref.py) and against
fec_repair_rows, the Python preconditions, and the guarantees of the model
itself on the oracle's shares.  No kernel launches here."""
import ctypes
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from correct_ref import correct_rows, corrected
from locate_ref import CLEAN, MANY, UNKNOWN, oracle_PQ, syndromes
from test_locate_surface import CODES, bases, clean_stripes
from test_verify_surface import ORDERED

torch = pytest.importorskip("torch")

assert CODES == [(1, 3), (2, 3), (3, 10), (4, 12), (4, 40), (10, 16), (20, 60), (33, 36)]


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_correct_batch", "fec_correct_rows"} <= exported
    L = capi.lib()
    assert list(L.fec_correct_batch.argtypes) == list(L.fec_locate_batch.argtypes)
    assert len(L.fec_correct_batch.argtypes) == 11
    assert list(L.fec_correct_rows.argtypes) == list(L.fec_locate_rows.argtypes)
    assert L.fec_correct_batch.restype is ctypes.c_int and L.fec_correct_rows.restype is ctypes.c_int


def test_python_attributes():
    assert hasattr(capi.Code, "correct_batch") and hasattr(capi, "correct_rows")
    assert hasattr(zfec_amd.Decoder, "correct_batch")
    doc = zfec_amd.Decoder.correct_batch.__doc__
    assert "IN\n        PLACE" in doc or "in place" in doc.lower()
    assert "k + 3" in doc  # the advice for callers who want double errors refused


def test_header_declares_the_calls():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zfec_hip.h")).read()
    assert "int fec_correct_batch(const fec_t* code," in header
    assert "int fec_correct_rows(const fec_t* code, const unsigned* block_nums, size_t num_block_nums, gf* rows);" \
        in header


# ---- validation before any GPU work ---------------------------------------------------

def correct_call(code, nums, src=True, nums_null=False, mask=True, code_null=False, ns=2, sz=8):
    """fec_correct_batch over pageable host buffers; returns (status, message,
    the culprit words, the block bytes).  `src` stands for blocks and `mask`
    for culprit, as in the verify table."""
    L = capi.lib()
    nb = len(nums)
    buf = ctypes.create_string_buffer(b"\x5a" * max(1, ns * nb * sz), max(1, ns * nb * sz))
    words = (ctypes.c_uint * max(1, ns))(*([0xA5A5A5A5] * max(1, ns)))
    st = L.fec_correct_batch(None if code_null else code.ptr, ctypes.addressof(buf) if src else None, sz, nb * sz,
                             None if nums_null else capi.uint_array(nums), nb, sz, ns,
                             ctypes.addressof(words) if mask else None, None, 0)
    return st, L.fec_last_error_message().decode(), list(words), buf.raw


@pytest.mark.parametrize("kw,match", ORDERED)
def test_validation_order(kw, match):
    """The verify call's table: the same checks in the same order with the same
    messages, `blocks` in place of `src` and `culprit` in place of `mismatch`."""
    kw = dict(kw)
    st, msg, _, _ = correct_call(capi.Code(3, 10), kw.pop("nums"), **kw)
    match = "blocks" if match == "src" else match.replace("mismatch", "culprit")
    assert st == capi.FEC_EINVAL and match in msg, msg


def test_nothing_to_check_with_exactly_k_blocks():
    for nums in ([7, 8, 9], []):
        st, msg, _, _ = correct_call(capi.Code(3, 10), nums)
        assert st == capi.FEC_EINVAL and "nothing to check" in msg, msg


@pytest.mark.parametrize("k,m,nums", [(3, 10, list(range(10))), (3, 10, [9, 4, 0, 7]), (10, 16, list(range(16)))])
def test_valid_arguments_on_pageable_host_memory(k, m, nums):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host blocks this call does not
    stage, in a message that names the call.  Neither crashes, neither writes."""
    st, msg, words, raw = correct_call(capi.Code(k, m), nums)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        assert st == capi.FEC_EINVAL and "fec_correct_batch takes device or page-locked host memory" in msg, msg
        assert "pageable host memory" in msg and "does not stage" in msg, msg
    assert words == [0xA5A5A5A5] * 2 and raw == b"\x5a" * len(raw)


def test_validation_precedes_enodev_and_empty_calls():
    st, msg, _, _ = correct_call(capi.Code(3, 10), [0, 1, 2, 12], ns=0)
    assert st == capi.FEC_EINVAL and "block number 12 out of range" in msg, msg


def test_empty_calls():
    """nstripes == 0 returns FEC_OK and touches nothing; sz == 0 returns FEC_OK
    with every verdict CLEAN (with a GPU; FEC_ENODEV without one)."""
    code = capi.Code(3, 10)
    have_gpu = zfec_amd.device_count() > 0
    st, msg, words, _ = correct_call(code, list(range(10)), ns=0)
    assert st == (capi.FEC_OK if have_gpu else capi.FEC_ENODEV), msg
    assert words == [0xA5A5A5A5]
    st, msg, words, raw = correct_call(code, list(range(10)), ns=2, sz=0)
    if have_gpu:
        assert st == capi.FEC_OK and words == [CLEAN] * 2, msg
    else:
        assert st == capi.FEC_ENODEV and words == [0xA5A5A5A5] * 2, msg
    assert raw == b"\x5a" * len(raw)


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w = (ctypes.c_uint * 4)()
    with pytest.raises(capi.FecError, match="duplicate block number 8"):
        code.correct_batch(ctypes.addressof(b), 8, 32, [8, 8, 9, 1], 8, 2, ctypes.addressof(w))
    with pytest.raises(capi.FecError, match="nothing to check"):
        code.correct_batch(ctypes.addressof(b), 8, 24, [7, 8, 9], 8, 2, ctypes.addressof(w))
    with pytest.raises(capi.FecError, match="culprit is NULL"):
        code.correct_batch(ctypes.addressof(b), 8, 32, [7, 8, 9, 1], 8, 2, 0)


# ---- fec_correct_rows ---------------------------------------------------------------------

def test_rows_validation():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 64)()
    outp = ctypes.cast(out, ctypes.c_void_p)
    for nums, match in (([3, 4, 5], "nothing to check"), (list(range(10)) + [3], "11 blocks per stripe"),
                        ([3, 4, 10, 1], "block number 10 out of range"), ([3, 3, 4, 5], "duplicate block number 3")):
        assert L.fec_correct_rows(code.ptr, capi.uint_array(nums), len(nums), outp) == capi.FEC_EINVAL
        assert match in L.fec_last_error_message().decode()
    assert L.fec_correct_rows(code.ptr, None, 4, outp) == capi.FEC_EINVAL
    assert L.fec_correct_rows(code.ptr, capi.uint_array([1, 2, 3, 4]), 4, None) == capi.FEC_EINVAL
    assert L.fec_correct_rows(None, capi.uint_array([1, 2, 3, 4]), 4, outp) == capi.FEC_EINVAL


def rows_sets(k, m):
    """The primaries, an all-parity basis (where there is one) and a mixed
    basis with all m - k checks, then 6 random splits of a random permutation."""
    rng = np.random.default_rng(3000 * k + m)
    sets = bases(k, m, 7 * k + m)
    for trial in range(6):
        nb = int(rng.integers(k + 1, m + 1))
        sets.append(rng.permutation(m)[:nb].tolist())
    return sets


@pytest.mark.parametrize("k,m", CODES)
def test_rows_against_the_model(k, m):
    code = capi.Code(k, m)
    for nums in rows_sets(k, m):
        nb = len(nums)
        raw = capi.correct_rows(code, nums)
        assert len(raw) == nb * k
        P, _ = oracle_PQ(k, m, tuple(nums))
        R, S = correct_rows(P)
        got = np.frombuffer(raw, dtype=np.uint8).reshape(nb, k)
        assert (got == R).all(), nums
        assert got.all(), ("zero entry", nums)
        assert all(h not in S[h] and len(set(S[h])) == k for h in range(nb))


@pytest.mark.parametrize("k,m", CODES)
def test_rows_are_the_repair_rows(k, m):
    """Row h is fec_repair_rows(present = nums[S_h], targets = {nums[h]})."""
    code = capi.Code(k, m)
    rng = np.random.default_rng(k + m)
    for nums in rows_sets(k, m)[:4]:
        nb = len(nums)
        got = np.frombuffer(capi.correct_rows(code, nums), dtype=np.uint8).reshape(nb, k)
        P, _ = oracle_PQ(k, m, tuple(nums))
        _, S = correct_rows(P)
        hs = range(nb) if nb <= 16 else sorted({0, k - 1, k, nb - 1} | set(rng.integers(0, nb, size=8).tolist()))
        for h in hs:
            want = capi.repair_rows(code, [nums[j] for j in S[h]], [nums[h]])
            assert got[h].tobytes() == want, (nums, h)


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    ns, sz = 4, 16
    host = torch.zeros((ns, 5, sz), dtype=torch.uint8)
    good = [7, 0, 9, 2, 4]
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 3"):
        dec.correct_batch(host, [7, 8, 9])
    with pytest.raises(zfec_amd.Error, match="required to hold 5 blocks per stripe, not 6"):
        dec.correct_batch(torch.zeros((ns, 6, sz), dtype=torch.uint8), good)
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but got \\[7, 0, 9, 0, 4\\]"):
        dec.correct_batch(host, [7, 0, 9, 0, 4])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        dec.correct_batch(host, [7, 0, 10, 2, 4])
    with pytest.raises(zfec_amd.Error, match="correct_batch takes a device tensor; host \\(numpy\\) blocks are not"):
        dec.correct_batch(host.numpy(), good)
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        dec.correct_batch(host, good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 5, sz\\]"):
        dec.correct_batch(host.to(torch.int32), good)


# ---- the model's guarantees on the oracle's shares ----------------------------------------

@pytest.mark.parametrize("k,m", [(1, 3), (2, 4), (3, 10), (4, 12), (5, 8), (10, 16), (3, 4)])
def test_model_properties(k, m):
    """Random corruptions of the oracle's shares, zero to three blocks per
    stripe, at one byte position or spread: whenever the verdict is a slot the
    syndromes of blocks_after are all zero; whenever exactly one block was
    corrupted and c >= 2, blocks_after equals the clean shares; a stripe whose
    verdict is no slot is unchanged."""
    sz, ns = 24, 120
    c = m - k
    rng = np.random.default_rng(17 * k + m)
    slots_seen = 0
    for nums in bases(k, m, k + m):
        P, Q = oracle_PQ(k, m, tuple(nums))
        clean = clean_stripes(k, m, nums, ns, sz, k * m)
        blocks = clean.copy()
        nbad = rng.integers(0, 4, size=ns)
        for s in range(ns):
            hit = rng.permutation(m)[:nbad[s]]
            same = bool(rng.integers(0, 2))
            x0 = int(rng.integers(0, sz))
            for j in hit:
                if rng.integers(0, 3) == 0:
                    blocks[s, j] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
                else:
                    blocks[s, j, x0 if same else int(rng.integers(0, sz))] ^= int(rng.integers(1, 256))
        v, after = corrected(P, Q, blocks)
        sig = syndromes(P, after)
        for s in range(ns):
            if v[s] < m:
                slots_seen += 1
                assert not sig[s].any(), (nums, s, int(v[s]))
                others = [j for j in range(m) if j != v[s]]
                assert (after[s, others] == blocks[s, others]).all()
            else:
                assert v[s] in (CLEAN, MANY, UNKNOWN) and (after[s] == blocks[s]).all()
            if nbad[s] == 0:
                assert v[s] == CLEAN
            if nbad[s] == 1 and c >= 2:
                assert v[s] < m and (after[s] == clean[s]).all(), (nums, s)
            if c == 1:
                assert v[s] in (CLEAN, UNKNOWN)
    assert (slots_seen > 0) == (c >= 2)
