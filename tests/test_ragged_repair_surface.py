"""CPU-side checks of the ragged repair and the ragged in-place correction
(fec_repair_batch_ragged, fec_correct_batch_ragged, Decoder.repair_ragged,
Decoder.correct_ragged): the exports, every validation that runs before any
GPU work, in the header's order and with its message, the stand-alone
validation program under the sanitizers' build flags, the layout helper
against the CPU oracle, and the Python preconditions.  No kernel launches
here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_repair_case as rr
import ragged_scrub_case as sc

torch = pytest.importorskip("torch")

REPAIR, CORRECT = "fec_repair_batch_ragged", "fec_correct_batch_ragged"
ROOT = os.path.join(os.path.dirname(zfec_amd.__file__), "..")
NONE = 0xFFFFFFFF


# ---- exports ---------------------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {REPAIR, CORRECT} <= exported
    L = capi.lib()
    assert len(L.fec_repair_batch_ragged.argtypes) == 18 and len(L.fec_correct_batch_ragged.argtypes) == 12
    assert hasattr(capi.Code, "repair_batch_ragged") and hasattr(capi.Code, "correct_batch_ragged")
    assert hasattr(zfec_amd.Decoder, "repair_ragged") and hasattr(zfec_amd.Decoder, "correct_ragged")


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "zfec_hip.h")).read()
    for fn in (REPAIR, CORRECT):
        assert "int %s(const fec_t* code," % fn in header


def test_the_validation_program_is_a_make_target():
    """tests/c/ragged_repair_validate.cpp has its own main and is built, with
    the library's host objects, under -fsanitize=address,undefined by a
    target beside asan-scrub; nothing goes into LD_PRELOAD."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "asan-repair: build/repair/validate" in mk and "tests/c/ragged_repair_validate.cpp" in mk
    recipe = mk[mk.index("build/repair/validate:"):mk.index("asan-repair:")]
    assert "-fsanitize=address,undefined" in recipe and "LD_PRELOAD" not in recipe
    prog = open(os.path.join(ROOT, "tests", "c", "ragged_repair_validate.cpp")).read()
    assert "int main()" in prog and REPAIR in prog and CORRECT in prog


# ---- fec_repair_batch_ragged: validation before any GPU work ----------------------------------------

def u64(vals):
    return (ctypes.c_ulonglong * max(1, len(vals)))(*[int(v) % 2**64 for v in vals])


PRESENT = [[7, 0, 4], [9, 8, 3]]
TARGETS = [[1, NONE], [0, 2]]


def repair_call(code, sizes=(8, 0, 24), soff=None, doff=None, present=None, targets=None, nt=None, npat=None,
                ids=(0, 1, 1), nstripes=None, null=(), src_bytes=None, dst_bytes=None, sbs=0, dbs=0):
    """One call over pageable host buffers in the packed layout (unless told); returns (status, message)."""
    L = capi.lib()
    k = code.k
    present = PRESENT if present is None else present
    targets = TARGETS if targets is None else targets
    t = len(targets[0]) if nt is None else nt
    sizes = list(sizes)
    start = np.cumsum([0] + sizes)[:-1]
    soff = [k * int(x) for x in start] if soff is None else list(soff)
    doff = [len(targets[0]) * int(x) for x in start] if doff is None else list(doff)
    in_len, out_len = k * sum(sizes), len(targets[0]) * sum(sizes)
    src, dst = ctypes.create_string_buffer(max(1, in_len)), ctypes.create_string_buffer(max(1, out_len))
    arrays = {"sizes": u64(sizes), "src_offsets": u64(soff), "dst_offsets": u64(doff)}
    ptr = lambda name: None if name in null else ctypes.addressof(arrays[name])
    idarr = capi.uint_array(list(ids)) if ids is not None else None
    st = L.fec_repair_batch_ragged(
        code.ptr if "code" not in null else None, None if "src" in null else ctypes.addressof(src),
        in_len if src_bytes is None else src_bytes, sbs, ptr("src_offsets"),
        None if "dst" in null else ctypes.addressof(dst), out_len if dst_bytes is None else dst_bytes, dbs,
        ptr("dst_offsets"), ptr("sizes"),
        None if "present" in null else capi.uint_array([x for p in present for x in p]),
        None if "targets" in null else capi.uint_array([x for p in targets for x in p]), t,
        len(present) if npat is None else npat, None if idarr is None else ctypes.addressof(idarr),
        len(sizes) if nstripes is None else nstripes, None, 0)
    assert bytes(dst.raw) == bytes(len(dst.raw)), "output bytes written by a call that cannot run here"
    return st, L.fec_last_error_message().decode()


def einval(st, msg, *needles):
    assert st == capi.FEC_EINVAL, (st, msg)
    for n in needles:
        assert n in msg, msg


def test_repair_pattern_argument_checks_in_fec_repair_batchs_order():
    code = capi.Code(3, 10)
    # each call breaks everything from one point of the order on: the first broken thing is named
    einval(*repair_call(code, null=("code", "src", "present")) + (REPAIR, "invalid fec_t"))
    einval(*repair_call(code, null=("src", "present", "targets")) + (REPAIR, "NULL buffer"))
    einval(*repair_call(code, null=("dst", "present")) + (REPAIR, "NULL buffer"))
    einval(*repair_call(code, null=("present", "targets"), nt=0) + (REPAIR, "present is NULL"))
    einval(*repair_call(code, null=("targets",), nt=0) + (REPAIR, "targets is NULL"))
    einval(*repair_call(code, nt=0, npat=0) + (REPAIR, "ntargets is 0: a call takes between 1 and 32"))
    einval(*repair_call(code, nt=33, npat=0) + (REPAIR, "ntargets is 33"))
    einval(*repair_call(code, npat=0, ids=None) + (REPAIR, "npatterns is 0: stripe 0 of 3 has no pattern"))
    einval(*repair_call(code, npat=65537, ids=None) + (REPAIR, "65537 patterns: a call takes at most 65536"))
    einval(*repair_call(code, ids=None, present=[[7, 0, 10], [9, 9, 3]]) +
           (REPAIR, "pattern_of is NULL with 2 patterns"))
    # every present number's range, then duplicates, then the targets
    einval(*repair_call(code, present=[[7, 0, 4], [9, 9, 10]], targets=[[1, 10], [0, 2]]) +
           (REPAIR, "pattern 1: block number 10 out of range (n = 10)"))
    einval(*repair_call(code, present=[[7, 0, 4], [9, 9, 3]], targets=[[1, 10], [0, 2]]) +
           (REPAIR, "pattern 1: duplicate block number 9"))
    einval(*repair_call(code, targets=[[1, 10], [0, 2]]) + (REPAIR, "pattern 0: target 10 is neither a block number"))


def test_repair_descriptor_checks_follow_the_patterns():
    code = capi.Code(3, 10)
    three = ("sizes", "src_offsets", "dst_offsets")
    einval(*repair_call(code, null=three, targets=[[1, 10], [0, 2]]) + ("target 10",))
    for i, name in enumerate(three):
        einval(*repair_call(code, null=three[i:]) + (REPAIR, "%s is NULL" % name))
    # NULL arrays come before the stripe count and before "no stripes"
    einval(*repair_call(code, null=("dst_offsets",), nstripes=2**32) + ("dst_offsets is NULL",))
    einval(*repair_call(code, null=("sizes",), nstripes=0) + ("sizes is NULL",))
    assert repair_call(code, nstripes=0)[0] == capi.FEC_OK
    assert repair_call(code, nstripes=0, npat=0)[0] == capi.FEC_OK
    # the count is refused before any array is read (ids and fit are both wrong here)
    einval(*repair_call(code, ids=(9, 9, 9), soff=[2**40, 0, 0], nstripes=2**32) + (REPAIR, "fewer than 2^32"))


def test_mixed_kinds_message():
    """The check itself needs a GPU to tell the kinds apart (the GPU suite
    provokes it); the wording the header promises is in the library."""
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"sizes, src_offsets and dst_offsets are of mixed memory kinds" in blob
    assert b"sizes and offsets are of mixed memory kinds: both in host memory, or both in device memory" in blob


def test_repair_host_side_id_out_of_range_comes_before_the_fit():
    code = capi.Code(3, 10)
    st, msg = repair_call(code, ids=(0, 2, 1), soff=[0, 24, 25])
    einval(st, msg, REPAIR, "stripe 1: pattern id 2 out of range (npatterns = 2)")
    einval(*repair_call(code, ids=(1, 0, 5)) + ("stripe 2: pattern id 5 out of range",))
    # without ids there is nothing to check
    st, msg = repair_call(code, ids=None, present=[PRESENT[0]], targets=[TARGETS[0]])
    assert "pattern id" not in msg and "does not fit" not in msg, msg


def test_repair_host_stripe_that_does_not_fit():
    code = capi.Code(3, 10)
    sizes = [8, 0, 24]
    st, msg = repair_call(code, sizes)  # the packed layout fits both arenas exactly
    assert "does not fit" not in msg, msg
    einval(*repair_call(code, sizes, soff=[0, 24, 25]) +
           (REPAIR, "stripe 2 does not fit src", "offset 25", "3 rows 24 apart", "size 24", "src_bytes 96"))
    einval(*repair_call(code, sizes, src_bytes=95) + (REPAIR, "stripe 2 does not fit src"))
    einval(*repair_call(code, sizes, doff=[0, 16, 17]) +
           (REPAIR, "stripe 2 does not fit dst", "offset 17", "2 rows 24 apart", "size 24", "dst_bytes 64"))
    einval(*repair_call(code, sizes, dst_bytes=63) + (REPAIR, "stripe 2 does not fit dst"))
    # src is looked at first, and the first stripe that does not fit is the one named
    einval(*repair_call(code, sizes, soff=[0, 24, 25], doff=[1000, 16, 16]) + ("stripe 0 does not fit dst",))
    einval(*repair_call(code, sizes, soff=[0, 24, 25], doff=[0, 16, 17]) + ("stripe 2 does not fit src",))
    # the place of a FEC_REPAIR_NONE row must exist although it is not written: stripe 0's row 1 is one
    einval(*repair_call(code, [8], ids=(0,), dst_bytes=15) + ("stripe 0 does not fit dst", "2 rows 8 apart"))
    # a zero-size stripe is not looked at
    st, msg = repair_call(code, sizes, soff=[0, 2**63, 24], doff=[0, 2**63, 16])
    assert "does not fit" not in msg, msg
    # the wrap cases: offset + size, (rows - 1) * stride, on either side
    einval(*repair_call(code, [16], ids=(0,), soff=[2**64 - 8]) + ("stripe 0 does not fit src",))
    einval(*repair_call(code, [16], ids=(0,), doff=[2**64 - 8]) + ("stripe 0 does not fit dst",))
    einval(*repair_call(code, [16], ids=(0,), sbs=2**63, src_bytes=2**64 - 1) + ("stripe 0 does not fit src",))
    einval(*repair_call(code, [16], ids=(0,), dbs=2**64 - 1, dst_bytes=2**64 - 1) + ("stripe 0 does not fit dst",))
    # fixed strides: the last row must end inside
    st, msg = repair_call(code, [16], ids=(0,), sbs=100, dbs=50, src_bytes=216, dst_bytes=66)
    assert "does not fit" not in msg, msg
    einval(*repair_call(code, [16], ids=(0,), sbs=100, dbs=50, src_bytes=215, dst_bytes=66) + ("does not fit src",))
    einval(*repair_call(code, [16], ids=(0,), sbs=100, dbs=50, src_bytes=216, dst_bytes=65) + ("does not fit dst",))


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_repair_valid_arguments_on_pageable_host_memory(k, m):
    """Valid arguments pass every check; what stops the call then is the
    machine: no GPU (FEC_ENODEV, the last check), or with one the pageable
    host arena, which this call does not stage.  Neither crashes."""
    present = PRESENT if k == 3 else [list(range(10)), list(range(6, 16))]
    st, msg = repair_call(capi.Code(k, m), present=present)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        einval(st, msg, "%s takes device or page-locked host memory" % REPAIR, "pageable host memory")


# ---- fec_correct_batch_ragged: fec_locate_batch_ragged's checks under its own name -----------------------------

def correct_call(code, sizes=(8, 0, 24), soff=None, nums=None, nstripes=None, null=(), nbytes=None, bs=0, flags=0):
    L = capi.lib()
    nums = sc.NUMS if nums is None else nums
    nb = len(nums)
    sizes = list(sizes)
    start = np.cumsum([0] + sizes)[:-1]
    soff = [nb * int(x) for x in start] if soff is None else list(soff)
    in_len = nb * sum(sizes)
    buf = ctypes.create_string_buffer(b"\x3c" * max(1, in_len), max(1, in_len))
    res = (ctypes.c_uint * max(1, len(sizes)))(*[0x55] * max(1, len(sizes)))
    arrays = {"sizes": u64(sizes), "offsets": u64(soff)}
    ptr = lambda name: None if name in null else ctypes.addressof(arrays[name])
    st = L.fec_correct_batch_ragged(code.ptr if "code" not in null else None,
                                    None if "blocks" in null else ctypes.addressof(buf),
                                    in_len if nbytes is None else nbytes, bs, ptr("offsets"), ptr("sizes"),
                                    None if "nums" in null else capi.uint_array(nums), nb,
                                    len(sizes) if nstripes is None else nstripes,
                                    None if "out" in null else ctypes.addressof(res), None, flags)
    assert bytes(buf.raw) == b"\x3c" * len(buf.raw) and all(w == 0x55 for w in res), "written by a call that cannot run"
    return st, L.fec_last_error_message().decode()


def test_correct_checks_in_order():
    code = capi.Code(3, 10)
    order = ["blocks", "sizes", "offsets", "nums", "out"]
    names = ["blocks", "sizes", "offsets", "block_nums", "culprit"]
    einval(*correct_call(code, null=("code",) + tuple(order)) + (CORRECT, "invalid fec_t"))
    for i in range(len(order)):
        einval(*correct_call(code, null=tuple(order[i:])) + (CORRECT, "%s is NULL" % names[i]))
    einval(*correct_call(code, nums=[0, 1, 2], null=("out",)) + ("culprit is NULL",))
    einval(*correct_call(code, nums=[0, 1, 2]) + (CORRECT, "nothing to check: 3 blocks per stripe", "k = 3"))
    einval(*correct_call(code, nums=list(range(9)) + [12, 12]) + (CORRECT, "11 blocks per stripe", "only n = 10"))
    einval(*correct_call(code, nums=[5, 5, 1, 10]) + (CORRECT, "block number 10 out of range (n = 10)"))
    einval(*correct_call(code, nums=[5, 5, 1, 9]) + (CORRECT, "duplicate block number 5"))
    einval(*correct_call(code, nums=[5, 5, 1, 9], nstripes=2**32) + ("duplicate block number 5",))
    einval(*correct_call(code, soff=[2**40, 0, 0], nstripes=2**32) + (CORRECT, "fewer than 2^32"))
    assert correct_call(code, nstripes=0)[0] == capi.FEC_OK
    einval(*correct_call(code, nstripes=0, null=("sizes",)) + ("sizes is NULL",))


def test_correct_host_stripe_that_does_not_fit():
    code = capi.Code(3, 10)
    nb = 7
    sizes = [8, 0, 24]
    st, msg = correct_call(code, sizes)
    assert "does not fit" not in msg, msg
    einval(*correct_call(code, sizes, soff=[0, nb * 8, nb * 8 + 1]) +
           (CORRECT, "stripe 2 does not fit blocks", "offset 57", "7 rows 24 apart", "size 24", "bytes 224"))
    einval(*correct_call(code, sizes, nbytes=nb * 32 - 1) + (CORRECT, "stripe 2 does not fit blocks"))
    einval(*correct_call(code, sizes, nbytes=nb * 8 + 3 * 24) + ("stripe 2 does not fit blocks",))  # all nb slots count
    st, msg = correct_call(code, sizes, soff=[0, 2**63, nb * 8])
    assert "does not fit" not in msg, msg
    einval(*correct_call(code, [16], soff=[2**64 - 8]) + ("stripe 0 does not fit blocks",))
    einval(*correct_call(code, [16], bs=2**63, nbytes=2**64 - 1) + ("stripe 0 does not fit blocks",))
    einval(*correct_call(code, [16], bs=100, nbytes=6 * 100 + 15) + ("stripe 0 does not fit blocks",))


@pytest.mark.parametrize("k,m,nums", [(3, 10, None), (3, 10, [0, 1, 2, 3]), (10, 16, list(range(16))),
                                      (3, 13, list(range(13)))])
def test_correct_valid_arguments_on_pageable_host_memory(k, m, nums):
    st, msg = correct_call(capi.Code(k, m), nums=nums, flags=capi.FEC_FLAG_ROW_PADDING)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        einval(st, msg, "%s takes device or page-locked host memory" % CORRECT, "blocks is pageable host memory")


def test_capi_wrappers_raise():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(96)
    w = u64([0, 0])
    r = (ctypes.c_uint * 2)()
    a = ctypes.addressof
    with pytest.raises(capi.FecError, match="fec_correct_batch_ragged: duplicate block number 8"):
        code.correct_batch_ragged(a(b), 96, 0, a(w), a(w), [8, 8, 9, 1], 2, a(r))
    with pytest.raises(capi.FecError, match="fec_correct_batch_ragged: culprit is NULL"):
        code.correct_batch_ragged(a(b), 96, 0, a(w), a(w), [8, 7, 9, 1], 2, 0)
    with pytest.raises(capi.FecError, match="fec_repair_batch_ragged: pattern 0: duplicate block number 7"):
        code.repair_batch_ragged(a(b), 96, 0, a(w), a(b), 96, 0, a(w), a(w), [[7, 7, 1]], [[0, -1]], 0, 2)
    with pytest.raises(capi.FecError, match="fec_repair_batch_ragged: dst_offsets is NULL"):
        code.repair_batch_ragged(a(b), 96, 0, a(w), a(b), 96, 0, 0, a(w), [[7, 0, 1]], [[2, -1]], 0, 2)
    with pytest.raises(capi.FecError, match="present is required to be"):
        code.repair_batch_ragged(a(b), 96, 0, a(w), a(b), 96, 0, a(w), a(w), [[7, 1]], [[0]], 0, 2)
    with pytest.raises(capi.FecError, match="one row per pattern: 2 rows, 1 patterns"):
        code.repair_batch_ragged(a(b), 96, 0, a(w), a(b), 96, 0, a(w), a(w), [[7, 0, 1]], [[0], [1]], 0, 2)


# ---- the layout helper against the CPU oracle ---------------------------------------------------------------

def test_repair_case_layout_and_oracle():
    """What the GPU tests compare with: each stripe's present blocks lie where
    the descriptors say, background everywhere else; the output arena holds
    the oracle's block for every target, the guard byte everywhere else."""
    from oracle import oracle

    sizes = [0, 5, 1024, 0, 33, 2049, 7]
    ids = [0, 1, 2, 3, 4, 5, 3]
    place = [3, 1, 5, 0, 2, 6, 4]
    for layout in ("packed", "shuffled", "block"):
        case = rr.RepairCase(3, 10, sizes, rr.PRESENT, rr.TARGETS, ids, layout=layout, place=place, seed=6, skip={4})
        data = np.random.default_rng(6).integers(0, 256, size=(3, sum(sizes)), dtype=np.uint8)
        allb = np.concatenate([data, oracle.encode(3, 10, data)])
        start = np.cumsum([0] + sizes)
        covered_in = np.zeros(case.src.shape, dtype=bool)
        written = np.zeros(case.want.shape, dtype=bool)
        for s, sz in enumerate(sizes):
            a, b = int(start[s]), int(start[s + 1])
            for j in range(3):
                o = rr.IN_OFF + case.soff[s] + j * (case.sbs or sz)
                assert (case.src[o:o + sz] == allb[rr.PRESENT[ids[s]][j], a:b]).all()
                assert not covered_in[o:o + sz].any(), "blocks overlap"
                covered_in[o:o + sz] = True
            for i, (lo, hi) in enumerate(case.row_spans(s)):
                tg = rr.TARGETS[ids[s]][i]
                assert hi - lo == sz and hi <= rr.OUT_OFF + case.dst_bytes
                if tg == rr.NONE or s == 4:
                    assert (case.want[lo:hi] == rr.GUARD).all()
                else:
                    assert (case.want[lo:hi] == allb[tg, a:b]).all(), (layout, s, i)
                    assert not written[lo:hi].any(), "rows overlap"
                    written[lo:hi] = True
        assert (case.src[~covered_in] == rr.BACKGROUND).all() and (case.want[~written] == rr.GUARD).all()
    # the oracle path itself: decode from parity only, then encode
    data = np.random.default_rng(1).integers(0, 256, size=(3, 50), dtype=np.uint8)
    allb = np.concatenate([data, oracle.encode(3, 10, data)])
    got, rows = rr.oracle_rows(3, 10, np.ascontiguousarray(allb[[9, 4, 6]]), [9, 4, 6], [0, rr.NONE, 8])
    assert (got == data).all() and sorted(rows) == [0, 2]
    assert (rows[0] == data[0]).all() and (rows[2] == allb[8]).all()


# ---- Python preconditions ---------------------------------------------------------------------------

def test_correct_ragged_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    fn = dec.correct_ragged
    data = torch.zeros(7 * 32, dtype=torch.uint8)
    E = zfec_amd.Error
    nums = sc.NUMS
    with pytest.raises(E, match=r"blocknums is required to hold between k \+ 1 = 4 and m = 10 block nums, not 3"):
        fn(data, [8, 24], [0, 1, 2])
    with pytest.raises(E, match="block nums are required to be distinct"):
        fn(data, [8, 24], [0, 1, 2, 2])
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8"):
        fn(torch.zeros((2, 112), dtype=torch.uint8), [8, 24], nums)
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        fn(data, [8, 2.5], nums)
    with pytest.raises(E, match="offsets is required to hold one word per stripe: 2, not 3"):
        fn(data, [8, 24], nums, offsets=[0, 56, 96])
    with pytest.raises(E, match=r"sizes is required to hold sizes and offsets in \[0, 2\^63\), but one was -8"):
        fn(data, [-8, 24], nums)
    with pytest.raises(E, match="data is required to be a uint8 tensor on a GPU"):
        fn(data, [8, 24], nums)


def test_repair_ragged_preconditions():
    dec = zfec_amd.Decoder(3, 10)
    fn = dec.repair_ragged
    data = torch.zeros(3 * 32, dtype=torch.uint8)
    E = zfec_amd.Error
    bn, tg = [[7, 0, 4], [9, 8, 3]], [[1, -1], [0, 2]]
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        fn(data, [8, 2.5], bn, tg)
    with pytest.raises(E, match=r"blocknums is required to be an integer array \[nstripes, k\] = \[2, 3\]"):
        fn(data, [8, 24], [[7, 0], [9, 8]], tg)
    with pytest.raises(E, match=r"targets is required to be an integer array \[nstripes, t\] = \[3, t\]"):
        fn(data, [8, 24, 0], bn + [[0, 1, 2]], tg)
    with pytest.raises(E, match="the block nums of a stripe are required to be distinct"):
        fn(data, [8, 24], [[7, 7, 4], [9, 8, 3]], tg)
    with pytest.raises(E, match=r"block nums are required to be in \[0, m-1\] = \[0, 9\], but one was 10"):
        fn(data, [8, 24], [[7, 0, 10], [9, 8, 3]], tg)
    with pytest.raises(E, match=r"targets are required to be in \[0, m-1\] = \[0, 9\] or -1 \(none\), but one was -2"):
        fn(data, [8, 24], bn, [[1, -2], [0, 2]])
    with pytest.raises(E, match="targets is required to hold between 1 and 32 block nums per stripe, not 33"):
        fn(data, [8, 24], bn, [[0] * 33] * 2)
    # the pattern form
    with pytest.raises(E, match="pattern_of is required to hold nstripes = 2 ids, not 3"):
        fn(data, [8, 24], (bn, [0, 1, 1]), tg)
    with pytest.raises(E, match=r"pattern_of ids are required to be in \[0, 1\]"):
        fn(data, [8, 24], (bn, [0, 2]), tg)
    with pytest.raises(E, match="one row per pattern: 1 rows, 2 patterns"):
        fn(data, [8, 24], (bn, [0, 1]), tg[:1])
    # the arena arguments, as decode_ragged's
    with pytest.raises(E, match="data is required to be a 1-D contiguous uint8 device tensor"):
        fn(torch.zeros((2, 48), dtype=torch.uint8), [8, 24], bn, tg)
    with pytest.raises(E, match="out is required to be a 1-D contiguous uint8 device tensor"):
        fn(data, [8, 24], bn, tg, out=torch.zeros(64, dtype=torch.int32))
    with pytest.raises(E, match="out_offsets is required to hold one word per stripe: 2, not 1"):
        fn(data, [8, 24], bn, tg, out_offsets=[0])
    with pytest.raises(E, match="data and out are required to be uint8 tensors on one GPU"):
        fn(data, [8, 24], bn, tg)
