"""CPU-side checks of the ragged batches (fec_encode_batch_ragged,
fec_decode_batch_ragged, fec_ragged_units, Encoder.encode_ragged,
Decoder.decode_ragged): the exports, the units against numpy, every validation
that runs before any GPU work, in the header's order, and the Python
preconditions.  No kernel launches here."""
import ctypes
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_case as rc

torch = pytest.importorskip("torch")


# ---- exports ---------------------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"fec_encode_batch_ragged", "fec_decode_batch_ragged", "fec_ragged_units"} <= exported
    L = capi.lib()
    assert L.fec_encode_batch_ragged.argtypes and L.fec_decode_batch_ragged.argtypes and L.fec_ragged_units.argtypes
    assert hasattr(capi.Code, "encode_batch_ragged") and hasattr(capi.Code, "decode_batch_ragged")
    assert hasattr(capi, "ragged_units")
    assert hasattr(zfec_amd.Encoder, "encode_ragged") and hasattr(zfec_amd.Decoder, "decode_ragged")


# ---- fec_ragged_units ---------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [
    [], [0, 0, 0, 0], rc.EDGE_SIZES, rc.BOUNDARY_SIZES,
    [int(x) for x in np.random.default_rng(2024).integers(0, 200000, size=100000)],
], ids=["empty", "zeros", "edge", "boundary", "1e5"])
def test_units_agree_with_numpy(sizes):
    got = capi.ragged_units(sizes)
    assert len(got) == len(sizes) + 1 and got == rc.units(sizes)


def test_units_of_the_edge_list():
    assert capi.ragged_units(rc.EDGE_SIZES)[-1] == 108
    assert capi.ragged_units([0, 1, 1023, 1024, 1025]) == [0, 0, 1, 2, 3, 5]


def test_units_null():
    L = capi.lib()
    assert L.fec_ragged_units(None, 0, None) == capi.FEC_EINVAL
    one = (ctypes.c_ulonglong * 1)()
    assert L.fec_ragged_units(None, 0, ctypes.addressof(one)) == capi.FEC_OK and one[0] == 0


# ---- validation before any GPU work ------------------------------------------------------------------

def u64(vals):
    return (ctypes.c_ulonglong * max(1, len(vals)))(*[int(v) % 2**64 for v in vals])


def ragged_call(code, op="enc", sizes=(8, 0, 24), soff=None, doff=None, nums=None, nstripes=None, src=True, dst=True,
                null=(), src_bytes=None, dst_bytes=None, sbs=0, dbs=0, flags=0):
    """fec_encode_batch_ragged / fec_decode_batch_ragged over host buffers in
    the packed layout (unless told); returns (status, message)."""
    L = capi.lib()
    k = code.k
    if nums is None:
        nums = list(range(k, code.m)) if op == "enc" else list(range(code.m - k, code.m))
    r = len(nums) if op == "enc" else (k if flags & capi.FEC_FLAG_ALL_PRIMARIES else sum(1 for x in nums if x >= k))
    sizes = list(sizes)
    start = np.cumsum([0] + sizes)[:-1]
    soff = [k * int(x) for x in start] if soff is None else list(soff)
    doff = [r * int(x) for x in start] if doff is None else list(doff)
    in_len, out_len = k * sum(sizes), r * sum(sizes)
    buf = ctypes.create_string_buffer(max(1, in_len))
    obuf = ctypes.create_string_buffer(max(1, out_len))
    arrays = {"sizes": u64(sizes), "src_offsets": u64(soff), "dst_offsets": u64(doff)}
    ptr = lambda name: None if name in null else ctypes.addressof(arrays[name])
    args = [code.ptr, ctypes.addressof(buf) if src else None, in_len if src_bytes is None else src_bytes, sbs,
            ptr("src_offsets"), ctypes.addressof(obuf) if dst else None, out_len if dst_bytes is None else dst_bytes,
            dbs, ptr("dst_offsets"), ptr("sizes"), None if "nums" in null else capi.uint_array(nums)]
    if op == "enc":
        args.append(len(nums) if "nonums" not in null else 0)
    ns = len(sizes) if nstripes is None else nstripes
    fn = L.fec_encode_batch_ragged if op == "enc" else L.fec_decode_batch_ragged
    st = fn(*(args + [ns, None, flags]))
    return st, L.fec_last_error_message().decode()


def einval(st, msg, *needles):
    assert st == capi.FEC_EINVAL, (st, msg)
    for n in needles:
        assert n in msg, msg


@pytest.mark.parametrize("op", ["enc", "dec"])
def test_null_code(op):
    L = capi.lib()
    b = ctypes.create_string_buffer(64)
    w = u64([0])
    a = ctypes.addressof
    if op == "enc":
        st = L.fec_encode_batch_ragged(None, a(b), 64, 0, a(w), a(b), 64, 0, a(w), a(w), capi.uint_array([3]), 1, 1,
                                       None, 0)
    else:
        st = L.fec_decode_batch_ragged(None, a(b), 64, 0, a(w), a(b), 64, 0, a(w), a(w), capi.uint_array([0, 1, 2]),
                                       1, None, 0)
    assert st == capi.FEC_EINVAL and "invalid fec_t" in L.fec_last_error_message().decode()


@pytest.mark.parametrize("op,fn", [("enc", "fec_encode_batch_ragged"), ("dec", "fec_decode_batch_ragged")])
@pytest.mark.parametrize("kw,name", [
    (dict(src=False), "src"),
    (dict(dst=False), "dst"),
    (dict(null=("sizes",)), "sizes"),
    (dict(null=("src_offsets",)), "src_offsets"),
    (dict(null=("dst_offsets",)), "dst_offsets"),
    (dict(null=("nums",)), None),
])
def test_null_arguments(op, fn, kw, name):
    name = name or ("block_nums" if op == "enc" else "index")
    st, msg = ragged_call(capi.Code(3, 10), op, **kw)
    einval(st, msg, fn, "%s is NULL" % name)


def test_null_comes_before_the_block_numbers():
    st, msg = ragged_call(capi.Code(3, 10), "enc", nums=[3, 10], null=("sizes",))
    einval(st, msg, "sizes is NULL")


def test_encode_block_numbers():
    code = capi.Code(3, 10)
    st, msg = ragged_call(code, "enc", null=("nonums",))
    einval(st, msg, "fec_encode_batch_ragged", "num_block_nums is 0")
    st, msg = ragged_call(code, "enc", nums=[3, 10])
    einval(st, msg, "fec_encode_batch_ragged", "block number 10 out of range (n = 10)")


def test_decode_index_checks_name_the_call():
    code = capi.Code(3, 10)
    for nums, what in (([0, 10, 2], "block number 10 out of range"), ([0, 5, 5], "duplicate block number 5"),
                       ([1, 5, 9], "primary block 1 must be at slot 1")):
        st, msg = ragged_call(code, "dec", nums=nums)
        einval(st, msg, "fec_decode_batch_ragged", what)


def test_block_numbers_come_before_the_stripe_count():
    st, msg = ragged_call(capi.Code(3, 10), "enc", nums=[3, 10], nstripes=2**32)
    einval(st, msg, "block number 10 out of range")


@pytest.mark.parametrize("op", ["enc", "dec"])
def test_too_many_stripes(op):
    # the arrays are not read: the count is refused first (and before the fit of stripe 0, which is wrong here)
    st, msg = ragged_call(capi.Code(3, 10), op, soff=[2**40, 0, 0], nstripes=2**32)
    einval(st, msg, "fec_%sode_batch_ragged" % op, "fewer than 2^32")


def test_no_stripes_is_ok_after_the_argument_checks():
    code = capi.Code(3, 10)
    assert ragged_call(code, "enc", nstripes=0)[0] == capi.FEC_OK
    assert ragged_call(code, "dec", nstripes=0)[0] == capi.FEC_OK
    einval(*ragged_call(code, "enc", nstripes=0, null=("sizes",)) + ("sizes is NULL",))


@pytest.mark.parametrize("op,rows", [("enc", 7), ("dec", 3)])
def test_host_stripe_that_does_not_fit(op, rows):
    code = capi.Code(3, 10)
    sizes = [8, 0, 24]
    fn = "fec_%sode_batch_ragged" % op
    # the packed layout fits exactly: one byte further on either side does not
    st, msg = ragged_call(code, op, sizes)
    assert "does not fit" not in msg, msg
    st, msg = ragged_call(code, op, sizes, soff=[0, 24, 25])
    einval(st, msg, fn, "stripe 2 does not fit src")
    st, msg = ragged_call(code, op, sizes, doff=[0, rows * 8, rows * 8 + 1])
    einval(st, msg, fn, "stripe 2 does not fit dst")
    st, msg = ragged_call(code, op, sizes, src_bytes=3 * 32 - 1)
    einval(st, msg, fn, "stripe 2 does not fit src")
    # the first stripe that does not fit is the one named, src before dst
    st, msg = ragged_call(code, op, sizes, soff=[1000, 24, 25], doff=[4000, 0, 0])
    einval(st, msg, "stripe 0 does not fit src")
    # a zero-size stripe is not looked at
    st, msg = ragged_call(code, op, sizes, soff=[0, 2**63, 24], doff=[0, 2**64 - 1, rows * 8])
    assert "does not fit" not in msg, msg
    # offset + size wraps 2^64
    st, msg = ragged_call(code, op, [16], soff=[2**64 - 8])
    einval(st, msg, "stripe 0 does not fit src")
    st, msg = ragged_call(code, op, [16], doff=[2**64 - 8])
    einval(st, msg, "stripe 0 does not fit dst")
    # (rows - 1) * stride wraps 2^64
    st, msg = ragged_call(code, op, [16], sbs=2**63, src_bytes=2**64 - 1)
    einval(st, msg, "stripe 0 does not fit src")
    st, msg = ragged_call(code, op, [16], dbs=2**63, dst_bytes=2**64 - 1)
    einval(st, msg, "stripe 0 does not fit dst")


@pytest.mark.parametrize("op", ["enc", "dec"])
@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_valid_arguments_on_pageable_host_memory(op, k, m):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU, or (with one) the pageable host arenas this call does not
    stage.  Neither crashes."""
    nums = None if op == "enc" else [m - 1 - j // 2 if j % 2 else j for j in range(k)]
    st, msg = ragged_call(capi.Code(k, m), op, nums=nums, flags=capi.FEC_FLAG_ROW_PADDING)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        einval(st, msg, "fec_%sode_batch_ragged takes device or page-locked host memory" % op,
               "pageable host memory")


def test_decode_with_nothing_missing_is_ok():
    st, msg = ragged_call(capi.Code(3, 10), "dec", nums=[0, 1, 2])
    assert st == capi.FEC_OK, msg


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w = u64([0, 0])
    a = ctypes.addressof
    with pytest.raises(capi.FecError, match="block number 12 out of range"):
        code.encode_batch_ragged(a(b), 64, 0, a(w), a(b), 64, 0, a(w), a(w), [3, 12], 2)
    with pytest.raises(capi.FecError, match="duplicate block number 8"):
        code.decode_batch_ragged(a(b), 64, 0, a(w), a(b), 64, 0, a(w), a(w), [8, 8, 9], 2)
    with pytest.raises(capi.FecError, match="sizes is NULL"):
        code.encode_batch_ragged(a(b), 64, 0, a(w), a(b), 64, 0, a(w), 0, [3], 2)


# ---- Python preconditions ---------------------------------------------------------------------------

def test_python_preconditions():
    enc, dec = zfec_amd.Encoder(3, 10), zfec_amd.Decoder(3, 10)
    data = torch.zeros(96, dtype=torch.uint8)
    E = zfec_amd.Error
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8"):
        enc.encode_ragged(torch.zeros(96, dtype=torch.int32), [8, 24])
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8"):
        enc.encode_ragged(torch.zeros((2, 48), dtype=torch.uint8), [8, 24])
    with pytest.raises(E, match="out is required to be a 1-D contiguous uint8"):
        enc.encode_ragged(data, [8, 24], out=torch.zeros(224, dtype=torch.int8))
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        enc.encode_ragged(data, torch.tensor([8, 24], dtype=torch.int32))
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        enc.encode_ragged(data, torch.zeros((2, 1), dtype=torch.int64))
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        enc.encode_ragged(data, [8, 2.5])
    with pytest.raises(E, match="offsets is required to hold one word per stripe: 2, not 3"):
        enc.encode_ragged(data, [8, 24], offsets=[0, 24, 96])
    with pytest.raises(E, match="out_offsets is required to hold one word per stripe: 2, not 1"):
        dec.decode_ragged(data, [8, 24], [0, 5, 9], out_offsets=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(E, match=r"sizes is required to hold sizes and offsets in \[0, 2\^63\), but one was -8"):
        enc.encode_ragged(data, [-8, 24])
    with pytest.raises(E, match=r"offsets is required to hold sizes and offsets in \[0, 2\^63\), but one was -1"):
        enc.encode_ragged(data, [8, 24], offsets=torch.tensor([0, -1], dtype=torch.int64))
    with pytest.raises(E, match=r"secondary block nums in \[k, m-1\] = \[3, 9\], but one was 2"):
        enc.encode_ragged(data, [8, 24], desired_blocks_nums=[3, 2])
    with pytest.raises(E, match=r"secondary block nums in \[k, m-1\] = \[3, 9\], but one was 10"):
        enc.encode_ragged(data, [8, 24], desired_blocks_nums=[10])
    with pytest.raises(E, match="blocknums is required to hold k = 3 distinct block nums"):
        dec.decode_ragged(data, [8, 24], [0, 5])
    with pytest.raises(E, match="blocknums is required to hold k = 3 distinct block nums"):
        dec.decode_ragged(data, [8, 24], [0, 5, 5])
    with pytest.raises(E, match=r"block nums are required to be in \[0, m-1\] = \[0, 9\], but one was 10"):
        dec.decode_ragged(data, [8, 24], [0, 5, 10])
    with pytest.raises(E, match="decode_ragged requires primary block 1 at slot 1"):
        dec.decode_ragged(data, [8, 24], [1, 5, 9])
    # arrays on mixed devices: a CPU tensor can stand in for neither side's GPU here,
    # so the meta device plays "another device"
    with pytest.raises(E, match="all on the data's device or all on the CPU, but sizes is on cpu and offsets on meta"):
        enc.encode_ragged(data, [8, 24], offsets=torch.zeros(2, dtype=torch.int64, device="meta"))
    # everything else in order: what remains is that the arenas are not on a GPU
    with pytest.raises(E, match="data and out are required to be uint8 tensors on one GPU"):
        enc.encode_ragged(data, [8, 24])
