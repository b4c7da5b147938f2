"""CPU-side checks of the ragged pair location and correction
(fec_locate2_batch_ragged, fec_correct2_batch_ragged, Decoder.locate2_ragged,
Decoder.correct2_ragged): the exports, every validation that runs before any
GPU work, in the header's order and with the call's name in the message, the
stand-alone validation program's make target, the Python preconditions, and the
CPU model the GPU tests compare with (tests/ragged_pairs_case.py) against
itself.  No kernel launches here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_pairs_case as rp
import ragged_scrub_case as sc

torch = pytest.importorskip("torch")

LOCATE2, CORRECT2 = "fec_locate2_batch_ragged", "fec_correct2_batch_ragged"
ROOT = os.path.join(os.path.dirname(zfec_amd.__file__), "..")
# (the call, its arena's name, its offsets' name, its extent's name)
CALLS = [(LOCATE2, "src", "src_offsets", "src_bytes"), (CORRECT2, "blocks", "offsets", "bytes")]


# ---- exports ---------------------------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {LOCATE2, CORRECT2} <= exported
    L = capi.lib()
    assert len(L.fec_locate2_batch_ragged.argtypes) == 12 and len(L.fec_correct2_batch_ragged.argtypes) == 12
    assert L.fec_locate2_batch_ragged.argtypes == L.fec_locate_batch_ragged.argtypes
    assert L.fec_correct2_batch_ragged.argtypes == L.fec_correct_batch_ragged.argtypes
    assert hasattr(capi.Code, "locate2_batch_ragged") and hasattr(capi.Code, "correct2_batch_ragged")
    assert hasattr(zfec_amd.Decoder, "locate2_ragged") and hasattr(zfec_amd.Decoder, "correct2_ragged")


def test_header_declares_the_calls():
    header = " ".join(open(os.path.join(ROOT, "include", "zfec_hip.h")).read().split())
    assert ("int fec_locate2_batch_ragged(const fec_t* code, const gf* src, size_t src_bytes, size_t src_block_stride, "
            "const unsigned long long* src_offsets, const unsigned long long* sizes, const unsigned* block_nums, "
            "size_t num_block_nums, size_t nstripes, unsigned* culprit, void* stream, unsigned flags);") in header
    assert ("int fec_correct2_batch_ragged(const fec_t* code, gf* blocks, size_t bytes, size_t block_stride, "
            "const unsigned long long* offsets, const unsigned long long* sizes, const unsigned* block_nums, "
            "size_t num_block_nums, size_t nstripes, unsigned* culprit, void* stream, unsigned flags);") in header


def test_the_validation_program_is_a_make_target():
    """tests/c/ragged_pairs_validate.cpp has its own main and is built, with
    the library's host objects, under -fsanitize=address,undefined by the
    pattern of asan-scrub; nothing goes into LD_PRELOAD."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "asan-pairs: build/pairs/validate" in mk and "build/pairs/validate" in mk
    recipe = mk[mk.index("build/scrub/validate"):mk.index("asan-scrub:")]
    assert "build/pairs/validate" in recipe and "-fsanitize=address,undefined" in recipe
    assert "LD_PRELOAD" not in recipe
    prog = open(os.path.join(ROOT, "tests", "c", "ragged_pairs_validate.cpp")).read()
    assert "int main()" in prog and LOCATE2 in prog and CORRECT2 in prog


# ---- validation before any GPU work --------------------------------------------------------------------

def u64(vals):
    return (ctypes.c_ulonglong * max(1, len(vals)))(*[int(v) % 2**64 for v in vals])


def pairs_call(fn, code, sizes=(8, 0, 24), soff=None, nums=None, nstripes=None, null=(), nbytes=None, bs=0, flags=0):
    """One call over pageable host memory in the packed layout (unless told);
    returns (status, message).  Neither the arena nor the 2 * nstripes verdict
    words may be written by a call that cannot run here."""
    L = capi.lib()
    nums = sc.NUMS if nums is None else nums
    nb = len(nums)
    sizes = list(sizes)
    start = np.cumsum([0] + sizes)[:-1]
    soff = [nb * int(x) for x in start] if soff is None else list(soff)
    in_len = nb * sum(sizes)
    buf = ctypes.create_string_buffer(b"\x3c" * max(1, in_len), max(1, in_len))
    res = (ctypes.c_uint * max(2, 2 * len(sizes)))(*[0x55] * max(2, 2 * len(sizes)))
    arrays = {"sizes": u64(sizes), "offsets": u64(soff)}
    ptr = lambda name: None if name in null else ctypes.addressof(arrays[name])  # noqa: E731
    st = getattr(L, fn)(code.ptr if "code" not in null else None, None if "arena" in null else ctypes.addressof(buf),
                        in_len if nbytes is None else nbytes, bs, ptr("offsets"), ptr("sizes"),
                        None if "nums" in null else capi.uint_array(nums), nb,
                        len(sizes) if nstripes is None else nstripes,
                        None if "out" in null else ctypes.addressof(res), None, flags)
    assert bytes(buf.raw) == b"\x3c" * len(buf.raw) and all(w == 0x55 for w in res), "written by a call that cannot run"
    return st, L.fec_last_error_message().decode()


def einval(st, msg, *needles):
    assert st == capi.FEC_EINVAL, (st, msg)
    for n in needles:
        assert n in msg, msg


@pytest.mark.parametrize("fn,arena,offsets,extent", CALLS)
def test_checks_in_header_order(fn, arena, offsets, extent):
    code = capi.Code(3, 10)
    order = ["arena", "sizes", "offsets", "nums", "out"]
    names = [arena, "sizes", offsets, "block_nums", "culprit"]
    # each call breaks everything from one point of the order on: the first broken thing is named
    einval(*pairs_call(fn, code, null=("code",) + tuple(order)) + (fn + ":", "invalid fec_t"))
    for i in range(len(order)):
        einval(*pairs_call(fn, code, null=tuple(order[i:])) + (fn + ":", "%s is NULL" % names[i]))
    einval(*pairs_call(fn, code, nums=[0, 1, 2], null=("out",)) + ("culprit is NULL",))
    einval(*pairs_call(fn, code, nums=[0, 1, 2]) + (fn + ":", "nothing to check: 3 blocks per stripe", "k = 3"))
    einval(*pairs_call(fn, code, nums=list(range(9)) + [12, 12]) + (fn + ":", "11 blocks per stripe", "only n = 10"))
    einval(*pairs_call(fn, code, nums=[5, 5, 1, 10]) + (fn + ":", "block number 10 out of range (n = 10)"))
    einval(*pairs_call(fn, code, nums=[5, 5, 1, 9]) + (fn + ":", "duplicate block number 5"))
    # the block numbers come before the stripe count, the count before any array is read
    einval(*pairs_call(fn, code, nums=[5, 5, 1, 9], nstripes=2**32) + ("duplicate block number 5",))
    einval(*pairs_call(fn, code, soff=[2**40, 0, 0], nstripes=2**32) + (fn + ":", "fewer than 2^32"))
    # no stripes: FEC_OK, but only after the pointers
    assert pairs_call(fn, code, nstripes=0)[0] == capi.FEC_OK
    einval(*pairs_call(fn, code, nstripes=0, null=("sizes",)) + ("sizes is NULL",))


@pytest.mark.parametrize("fn,arena,offsets,extent", CALLS)
def test_host_stripe_that_does_not_fit(fn, arena, offsets, extent):
    code = capi.Code(3, 10)
    nb = 7
    sizes = [8, 0, 24]
    st, msg = pairs_call(fn, code, sizes)
    assert "does not fit" not in msg, msg
    einval(*pairs_call(fn, code, sizes, soff=[0, nb * 8, nb * 8 + 1]) +
           (fn + ":", "stripe 2 does not fit " + arena, "offset 57", "7 rows 24 apart", "size 24", extent + " 224"))
    einval(*pairs_call(fn, code, sizes, nbytes=nb * 32 - 1) + (fn + ":", "stripe 2 does not fit " + arena))
    einval(*pairs_call(fn, code, sizes, nbytes=nb * 8 + 3 * 24) + ("stripe 2 does not fit",))  # all nb slots count
    st, msg = pairs_call(fn, code, sizes, soff=[0, 2**63, nb * 8])  # a zero-size stripe is not looked at
    assert "does not fit" not in msg, msg
    einval(*pairs_call(fn, code, [16], soff=[2**64 - 8]) + ("stripe 0 does not fit",))
    einval(*pairs_call(fn, code, [16], bs=2**63, nbytes=2**64 - 1) + ("stripe 0 does not fit",))
    einval(*pairs_call(fn, code, [16], bs=100, nbytes=6 * 100 + 15) + ("stripe 0 does not fit",))


@pytest.mark.parametrize("k,m,nums", [(3, 10, None), (3, 10, [0, 1, 2, 3]), (3, 10, [7, 0, 4, 1, 9, 2]),
                                      (10, 16, list(range(14))), (3, 13, list(range(13)))])
@pytest.mark.parametrize("fn,arena,offsets,extent", CALLS)
def test_valid_arguments_on_pageable_host_memory(fn, arena, offsets, extent, k, m, nums):
    """Valid arguments pass every check, whichever path the shape would take;
    what stops the call then is the machine: no GPU (FEC_ENODEV, the last
    check), or with one the pageable host arena.  Neither crashes."""
    st, msg = pairs_call(fn, capi.Code(k, m), nums=nums)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        einval(st, msg, "%s takes device or page-locked host memory" % fn, "%s is pageable host memory" % arena)


def test_messages_in_the_library():
    """Checks that need a GPU to fire (the GPU suite provokes them): the call's name travels with the message."""
    blob = open(capi.LIB_PATH, "rb").read()
    assert LOCATE2.encode() + b"\0" in blob and CORRECT2.encode() + b"\0" in blob


def test_capi_wrappers_raise():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(96)
    w = u64([0, 0])
    r = (ctypes.c_uint * 4)()
    a = ctypes.addressof
    with pytest.raises(capi.FecError, match="fec_locate2_batch_ragged: duplicate block number 8"):
        code.locate2_batch_ragged(a(b), 96, 0, a(w), a(w), [8, 8, 9, 1], 2, a(r))
    with pytest.raises(capi.FecError, match="fec_locate2_batch_ragged: culprit is NULL"):
        code.locate2_batch_ragged(a(b), 96, 0, a(w), a(w), [8, 7, 9, 1], 2, 0)
    with pytest.raises(capi.FecError, match="fec_correct2_batch_ragged: duplicate block number 8"):
        code.correct2_batch_ragged(a(b), 96, 0, a(w), a(w), [8, 8, 9, 1], 2, a(r))
    with pytest.raises(capi.FecError, match="fec_correct2_batch_ragged: sizes is NULL"):
        code.correct2_batch_ragged(a(b), 96, 0, a(w), 0, [8, 7, 9, 1], 2, a(r))


# ---- Python preconditions ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["locate2_ragged", "correct2_ragged"])
def test_python_preconditions(method):
    dec = zfec_amd.Decoder(3, 10)
    fn = getattr(dec, method)
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


# ---- the model against itself ------------------------------------------------------------------------

@pytest.mark.parametrize("order", sorted(rp.ORDERS))
def test_two_corrupt_slots_always_give_their_pair(order):
    """The main case of the GPU tests: every stripe with exactly two corrupt
    slots gets that pair from the model, whatever the placement, every single
    its slot, everything else (CLEAN, NONE); all 21 pairs and all five
    placements occur in the one call, beside clean, single-slot and zero-size
    stripes; the model's blocks after the correction are the never-corrupted
    ones; and the 70001-byte stripes have one corrupt byte in their first unit
    and one in their last."""
    case, clean, model, pairs, singles = rp.main_case(order)
    assert case.nb == 7 and case.c == 4 and case.sizes.count(0) == 8
    for s in range(case.ns):
        if s in pairs:
            assert model.pair_of(s) == pairs[s][0], (order, s, pairs[s], model.planes[:, s])
            assert len({j for t, j, _, _ in case.corrupt if t == s}) == 2
        elif s in singles:
            assert tuple(model.planes[:, s]) == (singles[s], rp.NONE), (order, s)
        else:
            assert tuple(model.planes[:, s]) == (rp.CLEAN, rp.NONE), (order, s)
    assert {p for p, _ in pairs.values()} == {(a, b) for a in range(7) for b in range(a + 1, 7)}
    assert {kind for _, kind in pairs.values()} == set(rp.PLACEMENTS)
    assert singles and len(pairs) + len(singles) < case.ns - case.sizes.count(0)
    for s in model.healed():
        assert (model.after[s] == clean.stripe_blocks(s)[0]).all(), (order, s)
    n = sc.IN_OFF + case.src_bytes
    assert (model.expected_arena()[:n] == clean.src[:n]).all()
    assert (model.expected_arena(heal=False)[:n] == case.src[:n]).all()
    big = [s for s, sz in enumerate(case.sizes) if sz == 70001]
    assert len(big) == 2
    for s in big:
        assert sorted(p for t, _, p, _ in case.corrupt if t == s) == [0, 70000] and pairs[s][1] == "first and last"
    # the placements are what their names say, wherever the stripe is long enough
    for s, (_, kind) in pairs.items():
        sz = case.sizes[s]
        ps = sorted(set(p for t, _, p, _ in case.corrupt if t == s))
        if kind == "same byte":
            assert len(ps) == 1
        elif kind == "one unit" and (sz - 1) % 1024:  # (a last unit of one byte has no two)
            assert len(ps) == 2 and ps[0] // 1024 == ps[1] // 1024
        elif kind == "overlapped chunk" and sz > 16:
            assert all(sz - 16 <= p < sz for p in ps)
        elif kind == "whole blocks":
            assert ps == list(range(sz))


def test_unfit_stripes_in_the_model():
    sizes = [900, 33, 2048, 300]
    cor = rp.place_pair(0, 1, 4, 900, "first and last", 0) + rp.place_pair(3, 0, 6, 300, "same byte", 1)
    case = sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, seed=3)
    model = rp.Model(case, unfit=(3,))
    assert model.planes.T.tolist() == [[1, 4], [rp.CLEAN, rp.NONE], [rp.CLEAN, rp.NONE], [rp.UNFIT, rp.NONE]]
    assert model.healed() == [0]
    want = model.expected_arena()
    o = sc.IN_OFF + case.soff[3]
    assert (want[o:o + 7 * 300] == case.src[o:o + 7 * 300]).all()  # as on entry, corrupt bytes included
