"""CPU-side checks of the batched decode with a pattern per stripe
(fec_decode_batch_mixed, fec_mixed_decode_rows, Decoder.decode_batch_mixed):
the exports, the validation that runs before any GPU work, the host-side
matrices against the CPU oracle, and the Python preconditions.  No kernel
launches here."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

torch = pytest.importorskip("torch")


def gf_matvec(rows, blocks):
    """rows (r, k) applied to blocks (k, n) over GF(2^8) with the oracle's multiply."""
    r, k = rows.shape
    out = np.zeros((r, blocks.shape[1]), dtype=np.uint8)
    for i in range(r):
        for j in range(k):
            c = int(rows[i, j])
            if c:
                out[i] ^= np.array([oracle.gf_mul(c, int(x)) for x in blocks[j]], dtype=np.uint8)
    return out


def shares(k, m, n, seed):
    """data (k, n) and all m blocks of it (m, n)."""
    data = np.random.default_rng(seed).integers(0, 256, size=(k, n), dtype=np.uint8)
    return data, np.concatenate([data, oracle.encode(k, m, data)])


def rows_of(code, pattern):
    k = code.k
    return np.frombuffer(capi.mixed_decode_rows(code, pattern), dtype=np.uint8).reshape(k, k)


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_decode_batch_mixed", "fec_mixed_decode_rows"} <= exported
    L = capi.lib()
    assert L.fec_decode_batch_mixed.argtypes and L.fec_mixed_decode_rows.argtypes
    assert hasattr(capi.Code, "decode_batch_mixed") and hasattr(zfec_amd.Decoder, "decode_batch_mixed")


# ---- validation before any GPU work ---------------------------------------------------

def mixed_call(code, patterns, ids, nstripes=None, src=True, dst=True, npatterns=None, pat_null=False,
               ids_null=False, sz=8):
    """fec_decode_batch_mixed over host buffers; returns (status, message)."""
    L = capi.lib()
    k = code.k
    ns = len(ids) if nstripes is None else nstripes
    buf = ctypes.create_string_buffer(max(1, ns) * k * sz)
    obuf = ctypes.create_string_buffer(max(1, ns) * k * sz)
    flat = [x for p in patterns for x in p]
    st = L.fec_decode_batch_mixed(
        code.ptr, ctypes.addressof(buf) if src else None, sz, k * sz, ctypes.addressof(obuf) if dst else None, sz,
        k * sz, None if pat_null else capi.uint_array(flat), len(patterns) if npatterns is None else npatterns,
        None if ids_null else ctypes.cast(capi.uint_array(ids), ctypes.c_void_p), sz, ns, None, 0)
    return st, L.fec_last_error_message().decode()


GOOD = ([[7, 8, 9], [0, 5, 2]], [0, 1, 1, 0])


@pytest.mark.parametrize("kw,match", [
    (dict(src=False), "NULL buffer"),
    (dict(dst=False), "NULL buffer"),
    (dict(pat_null=True), "patterns is NULL"),
    (dict(ids_null=True), "pattern_of is NULL"),
])
def test_null_arguments(kw, match):
    code = capi.Code(3, 10)
    st, msg = mixed_call(code, *GOOD, **kw)
    assert st == capi.FEC_EINVAL and match in msg, msg


def test_null_code():
    L = capi.lib()
    b = ctypes.create_string_buffer(64)
    st = L.fec_decode_batch_mixed(None, ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 24,
                                  capi.uint_array([7, 8, 9]), 1, ctypes.cast(capi.uint_array([0]), ctypes.c_void_p),
                                  8, 1, None, 0)
    assert st == capi.FEC_EINVAL and "invalid fec_t" in L.fec_last_error_message().decode()


def test_no_patterns_with_stripes():
    st, msg = mixed_call(capi.Code(3, 10), [], [0, 0], npatterns=0)
    assert st == capi.FEC_EINVAL and "npatterns is 0" in msg and "stripe 0" in msg, msg


def test_block_number_out_of_range_names_the_pattern():
    st, msg = mixed_call(capi.Code(3, 10), [[7, 8, 9], [0, 10, 2]], [0, 1])
    assert st == capi.FEC_EINVAL and "pattern 1" in msg and "block number 10 out of range" in msg, msg


def test_duplicate_names_the_pattern():
    st, msg = mixed_call(capi.Code(3, 10), [[7, 8, 9], [0, 1, 2], [4, 6, 4]], [0, 1, 2])
    assert st == capi.FEC_EINVAL and "pattern 2" in msg and "duplicate block number 4" in msg, msg


def test_host_id_out_of_range_names_the_stripe():
    st, msg = mixed_call(capi.Code(3, 10), [[7, 8, 9], [0, 5, 2]], [0, 1, 1, 2, 0])
    assert st == capi.FEC_EINVAL and "stripe 3" in msg and "pattern id 2 out of range" in msg, msg


def test_too_many_patterns():
    st, msg = mixed_call(capi.Code(1, 4), [[1]], [0], npatterns=65537)
    assert st == capi.FEC_EINVAL and "at most 65536" in msg, msg


@pytest.mark.parametrize("k,m", [(3, 10), (5, 9)])
def test_valid_arguments_on_pageable_host_memory(k, m):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host buffers this call does
    not stage.  Neither crashes."""
    pats = [list(range(m - k, m)), list(range(k))]
    st, msg = mixed_call(capi.Code(k, m), pats, [0, 1, 1, 0])
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        assert st == capi.FEC_EINVAL and "pageable host memory" in msg, msg


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    ids = capi.uint_array([0, 0])
    with pytest.raises(capi.FecError, match="pattern 0: duplicate block number 8"):
        code.decode_batch_mixed(ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 24, [[8, 8, 9]],
                                ctypes.addressof(ids), 8, 2)
    with pytest.raises(capi.FecError, match="pattern 1: block number 11 out of range"):
        code.decode_batch_mixed(ctypes.addressof(b), 8, 24, ctypes.addressof(b), 8, 24,
                                np.array([[7, 8, 9], [11, 1, 2]]), ctypes.addressof(ids), 8, 2)


# ---- fec_mixed_decode_rows -------------------------------------------------------------

def test_rows_validation():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 9)()
    for pat, match in (([3, 3, 4], "duplicate block number 3"), ([3, 4, 10], "block number 10 out of range")):
        assert L.fec_mixed_decode_rows(code.ptr, capi.uint_array(pat), ctypes.cast(out, ctypes.c_void_p)) == \
            capi.FEC_EINVAL
        assert match in L.fec_last_error_message().decode()
    assert L.fec_mixed_decode_rows(code.ptr, None, ctypes.cast(out, ctypes.c_void_p)) == capi.FEC_EINVAL
    assert L.fec_mixed_decode_rows(code.ptr, capi.uint_array([1, 2, 3]), None) == capi.FEC_EINVAL
    assert L.fec_mixed_decode_rows(None, capi.uint_array([1, 2, 3]), ctypes.cast(out, ctypes.c_void_p)) == \
        capi.FEC_EINVAL


def test_rows_every_pattern_k3_m10():
    """All 720 ordered 3-subsets of 10: the rows give back the data, and where
    the order obeys fec_decode's slot rule they are the reference's matrix."""
    k, m = 3, 10
    code = capi.Code(k, m)
    data, allb = shares(k, m, 64, seed=11)
    # gf_mul once per (coefficient, byte) pair that occurs: a 256 x 256 table
    mul = np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    n = checked_rule = 0
    for sub in itertools.combinations(range(m), k):
        for pat in itertools.permutations(sub):
            rows = rows_of(code, pat)
            got = np.zeros_like(data)
            for i in range(k):
                for j in range(k):
                    got[i] ^= mul[rows[i, j]][allb[pat[j]]]
            assert (got == data).all(), pat
            if all(b >= k or b == j for j, b in enumerate(pat)):
                assert (rows == oracle.decode_matrix(k, m, list(pat))).all(), pat
                checked_rule += 1
            n += 1
    assert n == 720 and checked_rule >= 120


@pytest.mark.parametrize("k,m", [(4, 8), (5, 9), (20, 60)])
def test_rows_other_codes(k, m):
    code = capi.Code(k, m)
    data, allb = shares(k, m, 64, seed=k)
    rng = np.random.default_rng(100 + k)
    pats = [rng.permutation(m)[:k].tolist() for _ in range(4)]
    pats.append(rng.permutation(k).tolist())             # all primaries, shuffled
    pats.append(rng.permutation(np.arange(m - k, m)).tolist())  # parity only
    for pat in pats:
        assert (gf_matvec(rows_of(code, pat), allb[pat]) == data).all(), pat


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    ns, sz = 4, 16
    host = torch.zeros((ns, 3, sz), dtype=torch.uint8)
    good = [[7, 8, 9], [0, 5, 2], [9, 1, 4], [3, 2, 1]]
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        dec.decode_batch_mixed(host, good)
    with pytest.raises(zfec_amd.Error, match="host \\(numpy\\) blocks are not staged"):
        dec.decode_batch_mixed(host.numpy(), good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 3, sz\\]"):
        dec.decode_batch_mixed(host.reshape(ns * 3, sz), good)
    with pytest.raises(zfec_amd.Error, match="required to hold 3 blocks per stripe, not 4"):
        dec.decode_batch_mixed(torch.zeros((ns, 4, sz), dtype=torch.uint8), good)
    with pytest.raises(zfec_amd.Error, match="integer array \\[nstripes, k\\] = \\[4, 3\\]"):
        dec.decode_batch_mixed(host, good[:3])
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but one stripe has \\[9, 1, 9\\]"):
        dec.decode_batch_mixed(host, [[7, 8, 9], [0, 5, 2], [9, 1, 9], [3, 2, 1]])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        dec.decode_batch_mixed(host, np.array([[7, 8, 9], [0, 5, 2], [10, 1, 4], [3, 2, 1]]))
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 12"):
        dec.decode_batch_mixed(host, torch.tensor([[7, 8, 9], [0, 5, 2], [6, 1, 4], [3, 12, 1]]))
    with pytest.raises(zfec_amd.Error, match="pattern_of is required to hold nstripes = 4 ids, not 3"):
        dec.decode_batch_mixed(host, ([[7, 8, 9], [0, 5, 2]], [0, 1, 1]))
    with pytest.raises(zfec_amd.Error, match="pattern_of ids are required to be in \\[0, 1\\]"):
        dec.decode_batch_mixed(host, ([[7, 8, 9], [0, 5, 2]], [0, 1, 2, 0]))
    with pytest.raises(zfec_amd.Error, match="required to be distinct"):
        dec.decode_batch_mixed(host, ([[7, 8, 9], [5, 5, 2]], [0, 1, 1, 0]))
