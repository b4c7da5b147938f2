"""CPU-side checks of the ragged scrub (fec_verify_batch_ragged,
fec_locate_batch_ragged, Decoder.verify_ragged, Decoder.locate_ragged): the
exports, every validation that runs before any GPU work, in the header's order
and with its message, the layout helper against the CPU model, and the Python
preconditions.  No kernel launches here."""
import ctypes
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import locate_ref
import ragged_scrub_case as sc

torch = pytest.importorskip("torch")

FNS = {"verify": "fec_verify_batch_ragged", "locate": "fec_locate_batch_ragged"}
OUT = {"verify": "mismatch", "locate": "culprit"}
both = pytest.mark.parametrize("op", sorted(FNS))


# ---- exports ---------------------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(FNS.values()) <= exported
    L = capi.lib()
    assert L.fec_verify_batch_ragged.argtypes and L.fec_locate_batch_ragged.argtypes
    assert hasattr(capi.Code, "verify_batch_ragged") and hasattr(capi.Code, "locate_batch_ragged")
    assert hasattr(zfec_amd.Decoder, "verify_ragged") and hasattr(zfec_amd.Decoder, "locate_ragged")
    assert capi.FEC_LOCATE_UNFIT == 0xFFFFFFFB and zfec_amd.LOCATE_UNFIT == -5
    assert np.uint32(capi.FEC_LOCATE_UNFIT).astype(np.int32) == zfec_amd.LOCATE_UNFIT
    assert "LOCATE_UNFIT" in zfec_amd.__all__


def test_header_declares_the_calls():
    import os
    header = open(os.path.join(os.path.dirname(zfec_amd.__file__), "..", "include", "zfec_hip.h")).read()
    assert "#define FEC_LOCATE_UNFIT   0xFFFFFFFBu" in header
    for fn in FNS.values():
        assert "int %s(const fec_t* code," % fn in header


# ---- validation before any GPU work ------------------------------------------------------------------

def u64(vals):
    return (ctypes.c_ulonglong * max(1, len(vals)))(*[int(v) % 2**64 for v in vals])


def scrub_call(code, op, sizes=(8, 0, 24), soff=None, nums=None, nstripes=None, null=(), src_bytes=None, sbs=0,
               flags=0):
    """One call over pageable host buffers in the packed layout (unless
    told); returns (status, message)."""
    L = capi.lib()
    nums = sc.NUMS if nums is None else nums
    nb = len(nums)
    sizes = list(sizes)
    start = np.cumsum([0] + sizes)[:-1]
    soff = [nb * int(x) for x in start] if soff is None else list(soff)
    in_len = nb * sum(sizes)
    buf = ctypes.create_string_buffer(max(1, in_len))
    res = (ctypes.c_uint * max(1, len(sizes)))()
    arrays = {"sizes": u64(sizes), "src_offsets": u64(soff)}
    ptr = lambda name: None if name in null else ctypes.addressof(arrays[name])
    ns = len(sizes) if nstripes is None else nstripes
    st = getattr(L, FNS[op])(code.ptr if "code" not in null else None,
                             None if "src" in null else ctypes.addressof(buf),
                             in_len if src_bytes is None else src_bytes, sbs, ptr("src_offsets"), ptr("sizes"),
                             None if "nums" in null else capi.uint_array(nums), nb, ns,
                             None if "out" in null else ctypes.addressof(res), None, flags)
    return st, L.fec_last_error_message().decode()


def einval(st, msg, *needles):
    assert st == capi.FEC_EINVAL, (st, msg)
    for n in needles:
        assert n in msg, msg


@both
def test_null_code(op):
    einval(*scrub_call(capi.Code(3, 10), op, null=("code",)) + (FNS[op], "invalid fec_t"))


@both
def test_invalid_code_comes_first(op):
    einval(*scrub_call(capi.Code(3, 10), op, null=("code", "src", "sizes")) + ("invalid fec_t",))


@both
@pytest.mark.parametrize("null,name", [("src", "src"), ("sizes", "sizes"), ("src_offsets", "src_offsets"),
                                       ("nums", "block_nums"), ("out", None)])
def test_null_arguments(op, null, name):
    st, msg = scrub_call(capi.Code(3, 10), op, null=(null,))
    einval(st, msg, FNS[op], "%s is NULL" % (name or OUT[op]))


@both
def test_nulls_are_named_in_the_headers_order(op):
    code = capi.Code(3, 10)
    order = ["src", "sizes", "src_offsets", "nums", "out"]
    names = ["src", "sizes", "src_offsets", "block_nums", OUT[op]]
    for i in range(len(order)):
        st, msg = scrub_call(code, op, null=tuple(order[i:]))
        einval(st, msg, "%s is NULL" % names[i])


@both
def test_null_comes_before_the_block_numbers(op):
    st, msg = scrub_call(capi.Code(3, 10), op, nums=[0, 1, 2], null=("out",))
    einval(st, msg, "%s is NULL" % OUT[op])


@both
def test_block_number_checks_in_order(op):
    code = capi.Code(3, 10)
    fn = FNS[op]
    einval(*scrub_call(code, op, nums=[0, 1, 2]) + (fn, "nothing to check: 3 blocks per stripe", "k = 3"))
    einval(*scrub_call(code, op, nums=[0, 1]) + (fn, "nothing to check"))
    # nb > n comes before a number out of range and a duplicate
    einval(*scrub_call(code, op, nums=list(range(9)) + [12, 12]) + (fn, "11 blocks per stripe", "only n = 10"))
    # out of range before a duplicate
    einval(*scrub_call(code, op, nums=[5, 5, 1, 10]) + (fn, "block number 10 out of range (n = 10)"))
    einval(*scrub_call(code, op, nums=[5, 5, 1, 9]) + (fn, "duplicate block number 5"))


@both
def test_block_numbers_come_before_the_stripe_count(op):
    st, msg = scrub_call(capi.Code(3, 10), op, nums=[5, 5, 1, 9], nstripes=2**32)
    einval(st, msg, "duplicate block number 5")


@both
def test_too_many_stripes(op):
    # the arrays are not read: the count is refused first (and before the fit of stripe 0, which is wrong here)
    st, msg = scrub_call(capi.Code(3, 10), op, soff=[2**40, 0, 0], nstripes=2**32)
    einval(st, msg, FNS[op], "fewer than 2^32")


@both
def test_no_stripes_is_ok_after_the_argument_checks(op):
    code = capi.Code(3, 10)
    assert scrub_call(code, op, nstripes=0)[0] == capi.FEC_OK
    einval(*scrub_call(code, op, nstripes=0, null=("sizes",)) + ("sizes is NULL",))
    einval(*scrub_call(code, op, nstripes=0, nums=[0, 1, 2]) + ("nothing to check",))


def test_mixed_kinds_message():
    """The check itself needs a GPU to tell the kinds apart (the GPU suite
    provokes it); the wording the header promises is in the library."""
    blob = open(capi.LIB_PATH, "rb").read()
    assert (b"sizes and src_offsets are of mixed memory kinds: both in host memory, or both in device memory on the "
            b"blocks' device") in blob


@both
def test_host_stripe_that_does_not_fit(op):
    code = capi.Code(3, 10)
    nb = len(sc.NUMS)
    sizes = [8, 0, 24]
    fn = FNS[op]
    # the packed layout fits exactly: one byte further does not
    st, msg = scrub_call(code, op, sizes)
    assert "does not fit" not in msg, msg
    st, msg = scrub_call(code, op, sizes, soff=[0, nb * 8, nb * 8 + 1])
    einval(st, msg, fn, "stripe 2 does not fit src", "offset 57", "7 rows 24 apart", "size 24", "src_bytes 224")
    st, msg = scrub_call(code, op, sizes, src_bytes=nb * 32 - 1)
    einval(st, msg, fn, "stripe 2 does not fit src")
    # the fit counts all nb slots, not only the k basis slots
    st, msg = scrub_call(code, op, sizes, src_bytes=nb * 8 + 3 * 24)
    einval(st, msg, fn, "stripe 2 does not fit src")
    # the first stripe that does not fit is the one named
    st, msg = scrub_call(code, op, sizes, soff=[1000, 56, 57])
    einval(st, msg, "stripe 0 does not fit src")
    # a zero-size stripe is not looked at
    st, msg = scrub_call(code, op, sizes, soff=[0, 2**63, nb * 8])
    assert "does not fit" not in msg, msg
    # offset + size wraps 2^64; (rows - 1) * stride wraps 2^64
    einval(*scrub_call(code, op, [16], soff=[2**64 - 8]) + ("stripe 0 does not fit src",))
    einval(*scrub_call(code, op, [16], sbs=2**63, src_bytes=2**64 - 1) + ("stripe 0 does not fit src",))
    # a fixed stride: the last slot must end inside
    st, msg = scrub_call(code, op, [16], sbs=100, src_bytes=6 * 100 + 16)
    assert "does not fit" not in msg, msg
    einval(*scrub_call(code, op, [16], sbs=100, src_bytes=6 * 100 + 15) + ("stripe 0 does not fit src",))


@both
@pytest.mark.parametrize("k,m,nums", [(3, 10, None), (3, 10, [0, 1, 2, 3]), (10, 16, list(range(16))),
                                      (3, 13, list(range(13)))])
def test_valid_arguments_on_pageable_host_memory(op, k, m, nums):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU (FEC_ENODEV), or with one the pageable host arena, which
    this call does not stage.  Neither crashes."""
    st, msg = scrub_call(capi.Code(k, m), op, nums=nums, flags=capi.FEC_FLAG_ROW_PADDING)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        einval(st, msg, "%s takes device or page-locked host memory" % FNS[op], "pageable host memory")


def test_capi_wrapper_raises():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w = u64([0, 0])
    r = (ctypes.c_uint * 2)()
    a = ctypes.addressof
    with pytest.raises(capi.FecError, match="duplicate block number 8"):
        code.verify_batch_ragged(a(b), 64, 0, a(w), a(w), [8, 8, 9, 1], 2, a(r))
    with pytest.raises(capi.FecError, match="fec_locate_batch_ragged: nothing to check"):
        code.locate_batch_ragged(a(b), 64, 0, a(w), a(w), [8, 7, 9], 2, a(r))
    with pytest.raises(capi.FecError, match="fec_verify_batch_ragged: sizes is NULL"):
        code.verify_batch_ragged(a(b), 64, 0, a(w), 0, [8, 7, 9, 1], 2, a(r))
    with pytest.raises(capi.FecError, match="fec_locate_batch_ragged: culprit is NULL"):
        code.locate_batch_ragged(a(b), 64, 0, a(w), a(w), [8, 7, 9, 1], 2, 0)


# ---- the layout helper against the CPU model --------------------------------------------------------------

def test_case_layout_and_model():
    """What the GPU tests compare with: the arena holds each stripe's blocks
    where the descriptors say, background everywhere else, and the model's
    verdicts are what the corruptions mean."""
    sizes = [0, 5, 1024, 0, 33, 2049]
    corrupt = [(1, 0, 4, 0x11), (2, 5, 1023, 0x80), (5, 1, 0, 1), (5, 2, 2048, 7)]
    place = [3, 1, 5, 0, 2, 4]
    for layout in ("packed", "shuffled", "block"):
        case = sc.ScrubCase(3, 10, sc.NUMS, sizes, corrupt, layout=layout, place=place, seed=6)
        P, Q = locate_ref.oracle_PQ(3, 10, tuple(sc.NUMS))
        covered = np.zeros(case.src.shape, dtype=bool)
        for s, sz in enumerate(sizes):
            one = case.stripe_blocks(s)
            assert one.shape == (1, 7, sz)
            if sz:
                assert (locate_ref.bits(P, Q, one)[0][0] == case.bits[s]).all(), (layout, s)
            assert locate_ref.verdicts(P, Q, one)[0] == case.verdict[s], (layout, s)
            for j in range(7):
                o = sc.IN_OFF + case.soff[s] + j * (case.sbs or sz)
                assert not covered[o:o + sz].any(), "blocks overlap"
                covered[o:o + sz] = True
            assert sc.IN_OFF + case.soff[s] + 6 * (case.sbs or sz) + sz <= sc.IN_OFF + case.src_bytes
        assert (case.src[~covered] == sc.BACKGROUND).all()
        # slot 0 corrupt: every check differs, the verdict names the slot; a check slot: its own bit only
        assert case.bits[1].all() and case.verdict[1] == 0
        assert case.bits[2].tolist() == [False, False, True, False] and case.verdict[2] == 5
        assert case.bits[5].all() and case.verdict[5] == sc.MANY
        assert case.verdict[0] == case.verdict[3] == case.verdict[4] == sc.CLEAN and not case.bits[4].any()
        assert case.want_words[:, 0].tolist() == [0, 15, 4, 0, 0, 15]
    wide = sc.ScrubCase(3, 40, list(range(40)), [7, 9], [(1, 39, 2, 5)], seed=1)
    assert wide.words == 2 and wide.want_words.tolist() == [[0, 0], [0, 1 << 4]]
    assert wide.all_bits().tolist() == [0xFFFFFFFF, 0x1F]


def test_cycled_corruptions_cover_what_the_issue_lists():
    sizes = sc.rc.EDGE_SIZES
    cor = sc.cycled_corrupt(sizes, 7)
    assert all(sizes[s] and s % 3 for s, _, _, _ in cor)
    assert {j for _, j, _, _ in cor} == set(range(7))
    assert len({s for s, _, _, _ in cor}) == len(cor) == sum(1 for s, sz in enumerate(sizes) if sz and s % 3)


# ---- Python preconditions ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["verify_ragged", "locate_ragged"])
def test_python_preconditions(method):
    dec = zfec_amd.Decoder(3, 10)
    fn = getattr(dec, method)
    data = torch.zeros(7 * 32, dtype=torch.uint8)
    E = zfec_amd.Error
    nums = sc.NUMS
    with pytest.raises(E, match=r"blocknums is required to hold between k \+ 1 = 4 and m = 10 block nums, not 3"):
        fn(data, [8, 24], [0, 1, 2])
    with pytest.raises(E, match=r"block nums are required to be in \[0, m-1\] = \[0, 9\], but one was 10"):
        fn(data, [8, 24], [0, 1, 2, 10])
    with pytest.raises(E, match="block nums are required to be distinct"):
        fn(data, [8, 24], [0, 1, 2, 2])
    with pytest.raises(TypeError):
        fn(data, [8, 24], 7)
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8"):
        fn(torch.zeros(96, dtype=torch.int32), [8, 24], nums)
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8"):
        fn(torch.zeros((2, 112), dtype=torch.uint8), [8, 24], nums)
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8"):
        fn(np.zeros(224, dtype=np.uint8), [8, 24], nums)
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        fn(data, torch.tensor([8, 24], dtype=torch.int32), nums)
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        fn(data, [8, 2.5], nums)
    with pytest.raises(E, match="offsets is required to hold one word per stripe: 2, not 3"):
        fn(data, [8, 24], nums, offsets=[0, 56, 96])
    with pytest.raises(E, match=r"sizes is required to hold sizes and offsets in \[0, 2\^63\), but one was -8"):
        fn(data, [-8, 24], nums)
    with pytest.raises(E, match=r"offsets is required to hold sizes and offsets in \[0, 2\^63\), but one was -1"):
        fn(data, [8, 24], nums, offsets=torch.tensor([0, -1], dtype=torch.int64))
    mixed = "both on the data's device or both on the CPU, but sizes is on cpu and offsets on meta"
    with pytest.raises(E, match=mixed):
        fn(data, [8, 24], nums, offsets=torch.zeros(2, dtype=torch.int64, device="meta"))
    # everything else in order: what remains is that the arena is not on a GPU
    with pytest.raises(E, match="data is required to be a uint8 tensor on a GPU"):
        fn(data, [8, 24], nums)
