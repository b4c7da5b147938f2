"""CPU-side checks of the ragged parity update (fec_update_batch_ragged,
capi.Code.update_batch_ragged, Encoder.update_ragged): the export, every
validation that runs before any GPU work, in the header's order and with its
message, the stand-alone validation program under the sanitizers' build flags,
the layout helper against the CPU oracle by hand, and the Python
preconditions.  No kernel launches here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_update_case as ru

rc = ru.rc
torch = pytest.importorskip("torch")

FN = "fec_update_batch_ragged"
ROOT = os.path.join(os.path.dirname(zfec_amd.__file__), "..")
NONE = capi.FEC_UPDATE_NONE


# ---- exports ---------------------------------------------------------------------------------

def test_symbol_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert FN in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert len(capi.lib().fec_update_batch_ragged.argtypes) == 18
    assert hasattr(capi.Code, "update_batch_ragged") and hasattr(zfec_amd.Encoder, "update_ragged")


def test_header_declares_the_call():
    header = open(os.path.join(ROOT, "include", "zfec_hip.h")).read()
    assert "int %s(const fec_t* code," % FN in header


def test_the_validation_program_is_a_make_target():
    """tests/c/ragged_update_validate.cpp has its own main and is built, with
    the library's host objects, under -fsanitize=address,undefined by
    asan-update beside asan-scrub and asan-repair; nothing goes into
    LD_PRELOAD."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "asan-update: build/update/validate" in mk and "tests/c/ragged_update_validate.cpp" in mk
    recipe = mk[mk.index("build/update/validate"):mk.index("asan-scrub:")]
    assert "tests/c/ragged_%_validate.cpp" in recipe
    assert "-fsanitize=address,undefined" in recipe and "LD_PRELOAD" not in recipe
    run = mk[mk.index("asan-update:"):mk.index("# The no-GPU Python tests")]
    assert "./$<" in run and "LD_PRELOAD" not in run
    prog = open(os.path.join(ROOT, "tests", "c", "ragged_update_validate.cpp")).read()
    assert "int main()" in prog and FN in prog


# ---- validation before any GPU work ---------------------------------------------------------------

def u64(vals):
    return (ctypes.c_ulonglong * max(1, len(vals)))(*[int(v) % 2**64 for v in vals])


NUMS = [7, 4]
CHANGED = [[0, NONE], [1, 1], [2, 0]]


def call(code, sizes=(8, 0, 24), ioff=None, roff=None, nums=None, nnums=None, changed=None, nc=None, nstripes=None,
         null=(), in_bytes=None, row_bytes=None, ibs=0, rbs=0, flags=0):
    """One call over pageable host buffers in the packed layout (unless told); returns (status, message)."""
    L = capi.lib()
    nums = NUMS if nums is None else nums
    changed = CHANGED if changed is None else changed
    c, r = len(changed[0]), len(nums)
    sizes = list(sizes)
    start = np.cumsum([0] + sizes)[:-1]
    ioff = [c * int(x) for x in start] if ioff is None else list(ioff)
    roff = [r * int(x) for x in start] if roff is None else list(roff)
    in_len, row_len = c * sum(sizes), r * sum(sizes)
    old, new = ctypes.create_string_buffer(max(1, in_len)), ctypes.create_string_buffer(max(1, in_len))
    rows = ctypes.create_string_buffer(b"\x55" * max(1, row_len), max(1, row_len))
    arrays = {"sizes": u64(sizes), "in_offsets": u64(ioff), "row_offsets": u64(roff)}
    ptr = lambda name: None if name in null else ctypes.addressof(arrays[name])
    charr = capi.uint_array([x for row in changed for x in row])
    st = L.fec_update_batch_ragged(
        code.ptr if "code" not in null else None, None if "oldb" in null else ctypes.addressof(old),
        None if "newb" in null else ctypes.addressof(new), in_len if in_bytes is None else in_bytes, ibs,
        ptr("in_offsets"), None if "rows" in null else ctypes.addressof(rows),
        row_len if row_bytes is None else row_bytes, rbs, ptr("row_offsets"), ptr("sizes"),
        None if "block_nums" in null else capi.uint_array(nums), r if nnums is None else nnums,
        None if "changed" in null else ctypes.addressof(charr), c if nc is None else nc,
        len(sizes) if nstripes is None else nstripes, None, flags)
    assert bytes(rows.raw) == b"\x55" * len(rows.raw), "rows written by a call that cannot run here"
    return st, L.fec_last_error_message().decode()


def einval(st, msg, *needles):
    assert st == capi.FEC_EINVAL, (st, msg)
    for n in needles:
        assert n in msg, msg


def test_update_argument_checks_in_fec_update_batchs_order():
    code = capi.Code(3, 10)
    # each call breaks everything from one point of the order on: the first broken thing is named
    order = ["newb", "rows", "block_nums", "changed"]
    einval(*call(code, null=["code"] + order) + (FN, "invalid fec_t"))
    for i, name in enumerate(order):
        einval(*call(code, null=order[i:], nnums=0) + (FN, "%s is NULL" % name))
    einval(*call(code, nnums=0, nc=0) + (FN, "num_block_nums is 0: a call updates between 1 and n = 10"))
    einval(*call(code, nums=list(range(10)) + [12], nc=0) + (FN, "num_block_nums is 11"))
    einval(*call(code, nums=[7, 7, 10], nc=0) + (FN, "block number 10 out of range (n = 10)"))
    einval(*call(code, nums=[7, 7], nc=0) + (FN, "duplicate block number 7"))
    three = ("sizes", "in_offsets", "row_offsets")
    einval(*call(code, nc=0, null=three) + (FN, "nchanged is 0: a stripe carries between 1 and 4"))
    einval(*call(code, nc=5, null=three) + (FN, "nchanged is 5"))
    # oldb may be NULL: the deltas form
    st, msg = call(code, null=("oldb",))
    assert "NULL" not in msg, msg


def test_descriptor_checks_follow():
    code = capi.Code(3, 10)
    three = ("sizes", "in_offsets", "row_offsets")
    for i, name in enumerate(three):
        einval(*call(code, null=three[i:]) + (FN, "%s is NULL" % name))
    # NULL arrays come before the stripe count and before "no stripes"
    einval(*call(code, null=("row_offsets",), nstripes=2**32) + ("row_offsets is NULL",))
    einval(*call(code, null=("sizes",), nstripes=0) + ("sizes is NULL",))
    assert call(code, nstripes=0)[0] == capi.FEC_OK
    # the count is refused before any array is read (numbers and fit are both wrong here)
    einval(*call(code, changed=[[9, 9]] * 3, ioff=[2**40, 0, 0], nstripes=2**32) + (FN, "fewer than 2^32"))


def test_mixed_kinds_message():
    """The check itself needs a GPU to tell the kinds apart (the GPU suite
    provokes it); the wording the header promises is in the library."""
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"sizes, in_offsets and row_offsets are of mixed memory kinds" in blob


def test_bad_host_side_number_comes_before_the_fit():
    code = capi.Code(3, 10)
    st, msg = call(code, changed=[[0, NONE], [1, 3], [2, 0]], ioff=[0, 16, 17])
    einval(st, msg, FN, "stripe 1, slot 1: changed block 3 is neither a primary (k = 3) nor FEC_UPDATE_NONE")
    einval(*call(code, changed=[[0, NONE], [1, 1], [0xFFFFFFFE, 0]]) + ("stripe 2, slot 0: changed block 4294967294",))
    st, msg = call(code, changed=[[NONE, NONE]] * 3)
    assert "changed block" not in msg and "does not fit" not in msg, msg


def test_host_stripe_that_does_not_fit():
    code = capi.Code(3, 10)
    sizes = [8, 0, 24]
    st, msg = call(code, sizes)  # the packed layout fits both arenas exactly
    assert "does not fit" not in msg, msg
    einval(*call(code, sizes, ioff=[0, 16, 17]) +
           (FN, "stripe 2 does not fit the inputs", "offset 17", "2 rows 24 apart", "size 24", "in_bytes 64"))
    einval(*call(code, sizes, in_bytes=63) + (FN, "stripe 2 does not fit the inputs"))
    einval(*call(code, sizes, roff=[0, 16, 17]) +
           (FN, "stripe 2 does not fit the rows", "offset 17", "2 rows 24 apart", "size 24", "row_bytes 64"))
    einval(*call(code, sizes, row_bytes=63) + (FN, "stripe 2 does not fit the rows"))
    # the inputs are looked at first, and the first stripe that does not fit is the one named
    einval(*call(code, sizes, ioff=[0, 16, 17], roff=[1000, 16, 16]) + ("stripe 0 does not fit the rows",))
    einval(*call(code, sizes, ioff=[0, 16, 17], roff=[0, 16, 17]) + ("stripe 2 does not fit the inputs",))
    # the place of a FEC_UPDATE_NONE slot must exist although it is not read: stripe 0's slot 1 is one
    einval(*call(code, [8], changed=[[0, NONE]], in_bytes=15) + ("stripe 0 does not fit the inputs", "2 rows 8 apart"))
    # a zero-size stripe is not looked at
    st, msg = call(code, sizes, ioff=[0, 2**63, 16], roff=[0, 2**63, 16])
    assert "does not fit" not in msg, msg
    # the wrap cases: offset + size, (slots - 1) * stride, on either side
    one = [[0, NONE]]
    einval(*call(code, [16], changed=one, ioff=[2**64 - 8]) + ("stripe 0 does not fit the inputs",))
    einval(*call(code, [16], changed=one, roff=[2**64 - 8]) + ("stripe 0 does not fit the rows",))
    einval(*call(code, [16], changed=[[0, NONE, 1]], ibs=2**63, in_bytes=2**64 - 1) +
           ("stripe 0 does not fit the inputs",))
    einval(*call(code, [16], changed=one, rbs=2**64 - 1, row_bytes=2**64 - 1) + ("stripe 0 does not fit the rows",))
    einval(*call(code, [16], changed=one, nums=[7, 4, 0], rbs=2**63, row_bytes=2**64 - 1) +
           ("stripe 0 does not fit the rows",))
    # fixed strides: the last slot and the last row must end inside
    st, msg = call(code, [16], changed=one, ibs=100, rbs=50, in_bytes=116, row_bytes=66)
    assert "does not fit" not in msg, msg
    einval(*call(code, [16], changed=one, ibs=100, rbs=50, in_bytes=115, row_bytes=66) + ("does not fit the inputs",))
    einval(*call(code, [16], changed=one, ibs=100, rbs=50, in_bytes=116, row_bytes=65) + ("does not fit the rows",))


@pytest.mark.parametrize("k,m", [(3, 10), (20, 24)])
def test_valid_arguments_on_pageable_host_memory(k, m):
    """Valid arguments pass every check, for any code; what stops the call
    then is the machine: no GPU (FEC_ENODEV, the last check), or with one the
    pageable host arena, which this call does not stage.  Neither crashes."""
    st, msg = call(capi.Code(k, m), flags=capi.FEC_FLAG_ROW_PADDING)
    if zfec_amd.device_count() == 0:
        assert st == capi.FEC_ENODEV and "no GPU" in msg, msg
    else:
        einval(st, msg, "%s takes device or page-locked host memory" % FN, "pageable host memory")


def test_capi_method_raises_the_librarys_message():
    code = capi.Code(3, 10)
    b = ctypes.create_string_buffer(64)
    w, ch = u64([8, 24]), capi.uint_array([0, 1])
    a = ctypes.addressof
    with pytest.raises(capi.FecError, match="fec_update_batch_ragged: stripe 1 does not fit the rows"):
        code.update_batch_ragged(0, a(b), 64, 0, a(w), a(b), 40, 0, a(w), a(w), [7], a(ch), 1, 2)
    with pytest.raises(capi.FecError, match="fec_update_batch_ragged: duplicate block number 7"):
        code.update_batch_ragged(0, a(b), 64, 0, a(w), a(b), 64, 0, a(w), a(w), [7, 7], a(ch), 1, 2)
    with pytest.raises(capi.FecError, match="fec_update_batch_ragged: in_offsets is NULL"):
        code.update_batch_ragged(0, a(b), 64, 0, 0, a(b), 64, 0, a(w), a(w), [7], a(ch), 1, 2)


# ---- fec_ragged_units agreement ---------------------------------------------------------------------

def test_units_agree_with_the_helper():
    """The sizes the GPU tail tests are built on: the library's prefix sum of
    units is the helper's, and the tail units fall where the tests say."""
    sizes = [4100, 3077, 3080, 3000]
    assert capi.ragged_units(sizes) == rc.units(sizes) == [0, 5, 9, 13, 16]
    assert rc.wave_ranges(16, 4) == [(0, 4), (4, 8), (8, 12), (12, 16)]
    for sizes in (rc.EDGE_SIZES, rc.BOUNDARY_SIZES, [2049, 2056, 2063, 4100, 1025, 1030, 1039] * 3, [0, 0], []):
        assert capi.ragged_units(sizes) == rc.units(sizes)


# ---- the layout helper against the CPU oracle, by hand ----------------------------------------------

def test_update_case_layout_and_oracle_by_hand():
    """What the GPU tests compare with, on a tiny K=2/M=5 case: the slots lie
    where the descriptors say; rows0 and want differ, row by row, by exactly
    sum over the live slots of E[nums[i]][j] * delta -- each term taken from
    the oracle as its encoding of the stripe whose only nonzero primary is j,
    holding the delta (the code is linear); stripes that are to be skipped,
    none slots, gaps and the tail do not change."""
    k, m, nums = 2, 5, [3, 0, 4]
    sizes = [0, 5, 33, 0, 7, 9]
    changed = [[0, 1], [1, ru.NONE], [ru.NONE, ru.NONE], [0, 0], [0, 0], [1, 0]]
    place = [3, 1, 4, 0, 5, 2]
    for form in ("delta", "oldnew"):
        for layout in ("packed", "shuffled", "block"):
            case = ru.UpdateCase(k, m, sizes, nums, changed, form=form, layout=layout, place=place, seed=3, skip={5})
            assert (case.oldb is None) == (form == "delta")
            assert case.rows0.shape == case.want.shape and case.newb.size == ru.IN_OFF + case.in_bytes + ru.TAIL
            assert case.ibs == (sum(sizes) + 7 if layout == "block" else 0)
            covered = np.zeros(case.rows0.shape, dtype=bool)
            covered_in = np.zeros(case.newb.shape, dtype=bool)
            for s, sz in enumerate(sizes):
                d = []  # this stripe's deltas as the inputs hold them
                for i in range(2):
                    o = ru.IN_OFF + case.ioff[s] + i * (case.ibs or sz)
                    assert o + sz <= ru.IN_OFF + case.in_bytes and not covered_in[o:o + sz].any()
                    covered_in[o:o + sz] = True
                    x = case.newb[o:o + sz]
                    d.append(x if form == "delta" else x ^ case.oldb[o:o + sz])
                for i, (lo, hi) in enumerate(case.row_spans(s)):
                    assert hi - lo == sz and hi <= ru.OUT_OFF + case.row_bytes and not covered[lo:hi].any()
                    covered[lo:hi] = True
                    expect = np.zeros(sz, dtype=np.uint8)
                    for slot, j in enumerate(changed[s]):
                        if j != ru.NONE and s != 5 and sz:
                            prim = np.zeros((k, sz), dtype=np.uint8)
                            prim[j] = d[slot]
                            expect ^= ru.all_blocks(k, m, prim)[nums[i]]
                    assert (case.rows0[lo:hi] ^ case.want[lo:hi] == expect).all(), (form, layout, s, i)
            assert (case.rows0[~covered] == ru.GUARD).all() and (case.want[~covered] == ru.GUARD).all()
            assert (case.newb[~covered_in] == ru.BACKGROUND).all()
            # by hand: stripe 1 changes primary 1 only, so the stored primary 0 (row 1) stays and
            # the parity rows move; stripe 4 names primary 0 twice, so row 1 moves by both deltas
            lo, hi = case.row_spans(1)[1]
            assert (case.rows0[lo:hi] == case.want[lo:hi]).all()
            lo, hi = case.row_spans(1)[0]
            assert (case.rows0[lo:hi] != case.want[lo:hi]).any()
            lo, hi = case.row_spans(4)[1]
            o = ru.IN_OFF + case.ioff[4]
            step = case.ibs or 7
            two = case.newb[o:o + 7] ^ case.newb[o + step:o + step + 7]
            if form == "oldnew":
                two = two ^ case.oldb[o:o + 7] ^ case.oldb[o + step:o + step + 7]
            assert (case.rows0[lo:hi] ^ case.want[lo:hi] == two).all()
    # dead slots count as none
    a = ru.UpdateCase(k, m, [9], nums, [[0, 1]], dead={(0, 1)}, seed=4)
    b = ru.UpdateCase(k, m, [9], nums, [[0, ru.NONE]], seed=4)
    assert (a.want == b.want).all() and (a.rows0 == b.rows0).all() and not (a.want == a.rows0).all()


# ---- Python preconditions ---------------------------------------------------------------------------

def test_update_ragged_preconditions():
    enc = zfec_amd.Encoder(3, 10)
    fn = enc.update_ragged
    E = zfec_amd.Error
    par, new = torch.zeros(7 * 32, dtype=torch.uint8), torch.zeros(32, dtype=torch.uint8)
    with pytest.raises(E, match="parity is required to be a 1-D contiguous uint8 device tensor"):
        fn(torch.zeros((2, 112), dtype=torch.uint8), [8, 24], [0, 1], new)
    with pytest.raises(E, match="new is required to be a 1-D contiguous uint8 device tensor"):
        fn(par, [8, 24], [0, 1], torch.zeros(32, dtype=torch.int32))
    with pytest.raises(E, match="old is required to be a 1-D contiguous uint8 device tensor"):
        fn(par, [8, 24], [0, 1], new, old=np.zeros(32, dtype=np.uint8))
    with pytest.raises(E, match=r"update_ragged block nums are required to be in \[0, m-1\] = \[0, 9\], but one was 10"):
        fn(par, [8, 24], [0, 1], new, blocknums=[3, 10])
    with pytest.raises(E, match="update_ragged block nums are required to be distinct"):
        fn(par, [8, 24], [0, 1], new, blocknums=[3, 3])
    with pytest.raises(E, match="sizes is required to be a 1-D int64 tensor"):
        fn(par, [8, 2.5], [0, 1], new)
    with pytest.raises(E, match="offsets is required to hold one word per stripe: 2, not 3"):
        fn(par, [8, 24], [0, 1], new, offsets=[0, 56, 96])
    with pytest.raises(E, match="in_offsets is required to hold one word per stripe: 2, not 1"):
        fn(par, np.array([8, 24]), [0, 1], new, in_offsets=np.array([0]))
    with pytest.raises(E, match=r"changed is required to be an integer array \[nstripes\] or \[nstripes, c\] with "
                                r"nstripes = 2"):
        fn(par, [8, 24], [0, 1, 2], new)
    with pytest.raises(E, match="update_ragged takes between 1 and 4 changed blocks per stripe, not 5"):
        fn(par, [8, 24], [[0] * 5] * 2, new)
    with pytest.raises(E, match=r"changed block nums are required to be primaries in \[0, k-1\] = \[0, 2\] or -1 "
                                r"\(none\), but one was 3"):
        fn(par, [8, 24], [0, 3], new)
    with pytest.raises(E, match="old is required to be an arena of new's size: 32 bytes, not 31"):
        fn(par, [8, 24], [0, 1], new, old=torch.zeros(31, dtype=torch.uint8))
    with pytest.raises(E, match="parity is required to be a 1-D contiguous uint8 device tensor, not a host tensor"):
        fn(par, [8, 24], [0, 1], new)
