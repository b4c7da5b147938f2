"""CPU-side checks of the batched parity verification (fec_verify_batch,
fec_verify_rows, Decoder.verify_batch): the exports, the validation that runs
before any GPU work and its order, the host-side matrix P against the CPU
oracle, and the Python preconditions.  No kernel launches here."""
import ctypes
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle
from verify_ref import gf_matmul, oracle_P

torch = pytest.importorskip("torch")

CODES = [(1, 2), (2, 3), (3, 10), (4, 12), (3, 16), (4, 40), (10, 16), (20, 60), (33, 36)]


# ---- exports ---------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_verify_batch", "fec_verify_rows"} <= exported
    L = capi.lib()
    assert L.fec_verify_batch.argtypes and L.fec_verify_rows.argtypes
    assert L.fec_verify_batch.restype is ctypes.c_int and L.fec_verify_rows.restype is ctypes.c_int
    assert hasattr(capi.Code, "verify_batch") and hasattr(capi, "verify_rows")
    assert hasattr(zfec_amd.Decoder, "verify_batch")


# ---- validation before any GPU work ---------------------------------------------------

def verify_call(code, nums, src=True, nums_null=False, mask=True, code_null=False, ns=2, sz=8):
    """fec_verify_batch over pageable host buffers; returns (status, message)."""
    L = capi.lib()
    nb = len(nums)
    buf = ctypes.create_string_buffer(max(1, ns * nb * sz))
    words = (ctypes.c_uint * max(1, ns * 8))()
    st = L.fec_verify_batch(None if code_null else code.ptr, ctypes.addressof(buf) if src else None, sz, nb * sz,
                            None if nums_null else capi.uint_array(nums), nb, sz, ns,
                            ctypes.addressof(words) if mask else None, None, 0)
    return st, L.fec_last_error_message().decode()


GOOD = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]

# each case is wrong in the way it names AND in every way listed after it, so
# the message shows which check ran first
ORDERED = [
    (dict(code_null=True, src=False, nums=[0, 1]), "invalid fec_t"),
    (dict(src=False, nums=[0, 1]), "src"),
    (dict(nums_null=True, mask=False, nums=[0, 1]), "block_nums is NULL"),
    (dict(mask=False, nums=[0, 1]), "mismatch is NULL"),
    (dict(nums=[0, 99, 99]), "nothing to check"),
    (dict(nums=[0, 0, 99] + list(range(1, 9))), "11 blocks per stripe"),
    (dict(nums=[0, 1, 2, 3, 4, 4, 10]), "block number 10 out of range (n = 10)"),
    (dict(nums=[0, 1, 2, 3, 4, 4]), "duplicate block number 4"),
]


@pytest.mark.parametrize("kw,match", ORDERED)
def test_validation_order(kw, match):
    kw = dict(kw)
    st, msg = verify_call(capi.Code(3, 10), kw.pop("nums"), **kw)
    assert st == capi.FEC_EINVAL and match in msg, msg


def test_nothing_to_check_with_exactly_k_blocks():
    st, msg = verify_call(capi.Code(3, 10), [7, 8, 9])
    assert st == capi.FEC_EINVAL and "nothing to check" in msg, msg
    st, msg = verify_call(capi.Code(3, 10), [])
    assert st == capi.FEC_EINVAL and "nothing to check" in msg, msg


@pytest.mark.parametrize("k,m,nums", [(3, 10, GOOD), (3, 10, [9, 4, 0, 7]), (10, 16, list(range(16)))])
def test_valid_arguments_on_pageable_host_memory(k, m, nums):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host blocks this call does not
    stage.  Neither crashes."""
    st, msg = verify_call(capi.Code(k, m), nums)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        assert st == capi.FEC_EINVAL and "pageable host memory" in msg and "does not stage" in msg, msg


def test_validation_precedes_enodev():
    """A bad block number is reported whether or not a GPU is visible."""
    st, msg = verify_call(capi.Code(3, 10), [0, 1, 2, 12], ns=0)
    assert st == capi.FEC_EINVAL and "block number 12 out of range" in msg, msg


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w = (ctypes.c_uint * 4)()
    with pytest.raises(capi.FecError, match="duplicate block number 8"):
        code.verify_batch(ctypes.addressof(b), 8, 32, [8, 8, 9, 1], 8, 2, ctypes.addressof(w))
    with pytest.raises(capi.FecError, match="nothing to check"):
        code.verify_batch(ctypes.addressof(b), 8, 24, [7, 8, 9], 8, 2, ctypes.addressof(w))


# ---- fec_verify_rows ---------------------------------------------------------------------

def test_rows_validation():
    L = capi.lib()
    code = capi.Code(3, 10)
    out = (ctypes.c_ubyte * 64)()
    outp = ctypes.cast(out, ctypes.c_void_p)
    for nums, match in (([3, 4, 5], "nothing to check"), (list(range(10)) + [3], "11 blocks per stripe"),
                        ([3, 4, 10, 1], "block number 10 out of range"), ([3, 3, 4, 5], "duplicate block number 3")):
        assert L.fec_verify_rows(code.ptr, capi.uint_array(nums), len(nums), outp) == capi.FEC_EINVAL
        assert match in L.fec_last_error_message().decode()
    assert L.fec_verify_rows(code.ptr, None, 4, outp) == capi.FEC_EINVAL
    assert L.fec_verify_rows(code.ptr, capi.uint_array([1, 2, 3, 4]), 4, None) == capi.FEC_EINVAL
    assert L.fec_verify_rows(None, capi.uint_array([1, 2, 3, 4]), 4, outp) == capi.FEC_EINVAL


def test_rows_primaries_against_parity_are_the_encode_rows():
    k, m = 3, 10
    P = np.frombuffer(capi.verify_rows(capi.Code(k, m), range(m)), dtype=np.uint8).reshape(m - k, k)
    assert (P == oracle.enc_matrix(k, m)[k:]).all()


@pytest.mark.parametrize("k,m", CODES)
def test_rows_against_the_oracle(k, m):
    """20 random splits of a random permutation into basis and checks: P is
    E[checks] . inverse(E[basis]) as the oracle builds it, has no zero entry
    (the code is MDS), and maps the basis shares onto the check shares."""
    code = capi.Code(k, m)
    rng = np.random.default_rng(1000 * k + m)
    data = rng.integers(0, 256, size=(k, 33), dtype=np.uint8)
    allb = np.concatenate([data, oracle.encode(k, m, data)])
    for trial in range(20):
        nb = int(rng.integers(k + 1, m + 1))
        nums = rng.permutation(m)[:nb].tolist()
        raw = capi.verify_rows(code, nums)
        assert len(raw) == (nb - k) * k
        P = np.frombuffer(raw, dtype=np.uint8).reshape(nb - k, k)
        assert (P == oracle_P(k, m, nums)).all(), nums
        assert P.all(), ("zero entry", nums)
        assert (gf_matmul(P, allb[nums[:k]]) == allb[nums[k:]]).all(), nums


# ---- Python preconditions ----------------------------------------------------------------

def test_python_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    ns, sz = 4, 16
    host = torch.zeros((ns, 5, sz), dtype=torch.uint8)
    good = [7, 0, 9, 2, 4]
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 3"):
        dec.verify_batch(host, [7, 8, 9])
    with pytest.raises(zfec_amd.Error, match="between k \\+ 1 = 4 and m = 10 block nums, not 11"):
        dec.verify_batch(host, list(range(11)))
    with pytest.raises(zfec_amd.Error, match="required to hold 5 blocks per stripe, not 6"):
        dec.verify_batch(torch.zeros((ns, 6, sz), dtype=torch.uint8), good)
    with pytest.raises(zfec_amd.Error, match="required to be distinct, but got \\[7, 0, 9, 0, 4\\]"):
        dec.verify_batch(host, [7, 0, 9, 0, 4])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was 10"):
        dec.verify_batch(host, [7, 0, 10, 2, 4])
    with pytest.raises(zfec_amd.Error, match="required to be in \\[0, m-1\\] = \\[0, 9\\], but one was -1"):
        dec.verify_batch(host, [7, 0, -1, 2, 4])
    with pytest.raises(zfec_amd.Error, match="host \\(numpy\\) blocks are not staged"):
        dec.verify_batch(host.numpy(), good)
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        dec.verify_batch(host, good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 5, sz\\]"):
        dec.verify_batch(host.to(torch.int32), good)
    with pytest.raises(zfec_amd.Error, match="required to be a uint8 device tensor \\[nstripes, 5, sz\\]"):
        dec.verify_batch(host.reshape(ns * 5, sz), good)
