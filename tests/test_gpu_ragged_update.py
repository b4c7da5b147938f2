"""The ragged parity update on the GPU (fec_update_batch_ragged;
zfec_amd/csrc/kernels.hip matupdate_ragged<C,R> for every code): every stripe
its own size and its own changed blocks.  The whole row arena -- the stored
blocks before the change, the guard byte in every gap and in the tail -- is
compared after the call with what the CPU oracle expects
(tests/ragged_update_case.py): encode, apply the changes to the primaries,
encode again.  The inputs must come back unchanged.

The kernel XORs into its output, so every byte of a row must belong to exactly
one lane of exactly one unit.  In the ragged walk a stripe of 1024 w + t bytes,
0 < t < 16, can have its tail unit as the first unit of one wave's range and
the unit before it as the last of the previous wave's: test_tail_unit_* land
exactly there and say so with the walk's own arithmetic."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import far_arena
import ragged_update_case as ru
from test_gpu_update import encode_all, random_changed

rc = ru.rc
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NONE = ru.NONE


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def words(vals, where):
    """nstripes 8-byte words in host (numpy) or device (torch) memory: (keep-alive, address)."""
    a = np.array([int(v) % 2**64 for v in vals], dtype=np.uint64)
    if where == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t, t.data_ptr()


def num_words(changed, where):
    """nstripes x c uint32 numbers (-1: FEC_UPDATE_NONE) in host or device memory."""
    a = np.ascontiguousarray(np.asarray(changed, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    if where == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int32)).cuda()
    return t, t.data_ptr()


def launch(case, desc="host", chw="host", pinned=False, ioff=None, roff=None, sizes=None, changed=None, tail=0,
           flags=capi.FEC_FLAG_ASYNC, rows=None):
    """One call over fresh copies of the case's arenas, which end `tail` bytes
    past what the case holds (or over `rows`, a device tensor a previous call
    left); returns (the whole row tensor on the host, the last kernel's name).
    The inputs must come back unchanged."""
    pad_in = np.full(tail, ru.BACKGROUND, dtype=np.uint8)
    new_h = np.concatenate([case.newb, pad_in])
    old_h = np.concatenate([case.oldb, pad_in]) if case.oldb is not None else None
    row_h = np.concatenate([case.rows0, np.full(tail, ru.GUARD, dtype=np.uint8)])
    place = (lambda a: torch.from_numpy(a.copy()).pin_memory()) if pinned else (lambda a: torch.from_numpy(a.copy()).cuda())
    new, old = place(new_h), place(old_h) if old_h is not None else None
    if rows is None:
        rows = place(row_h)
    keep = [words(case.sizes if sizes is None else sizes, desc), words(case.ioff if ioff is None else ioff, desc),
            words(case.roff if roff is None else roff, desc), num_words(case.changed if changed is None else changed, chw)]
    capi.Code(case.k, case.m).update_batch_ragged(
        old.data_ptr() + ru.IN_OFF if old is not None else 0, new.data_ptr() + ru.IN_OFF, case.in_bytes, case.ibs,
        keep[1][1], rows.data_ptr() + ru.OUT_OFF, case.row_bytes, case.rbs, keep[2][1], keep[0][1], case.nums,
        keep[3][1], case.c, case.ns, stream=torch.cuda.current_stream().cuda_stream, flags=flags)
    name = capi.last_kernel_name()
    torch.cuda.synchronize()
    assert (new.cpu().numpy() == new_h).all(), "the new blocks were written"
    assert old is None or (old.cpu().numpy() == old_h).all(), "the old blocks were written"
    got = rows.cpu().numpy()
    assert (got[case.want.size:] == ru.GUARD).all(), "bytes written past the arena"
    return got[:case.want.size], name


def check(case, got, what):
    assert (got == case.want).all(), (what, case.explain(got))


def parity(k, m):
    return list(range(k, m))


# ---- 1. the edge sizes of K=3/M=10, all 7 parity rows ------------------------------------------------

PERM = [int(x) for x in np.random.default_rng(11).permutation(len(rc.EDGE_SIZES))]
ORDERS = {"listed": rc.EDGE_SIZES, "reversed": rc.EDGE_SIZES[::-1], "permuted": [rc.EDGE_SIZES[i] for i in PERM],
          "boundary": rc.BOUNDARY_SIZES}
_cases = {}


def edge_changed(sizes, C, seed):
    """Per-stripe random numbers with some none slots; the first two nonempty
    stripes are all-none and the same block in every slot."""
    ch = random_changed(np.random.default_rng(seed), 3, len(sizes), C)
    full = [s for s, sz in enumerate(sizes) if sz]
    ch[full[0]], ch[full[1]] = NONE, 2
    return ch


def base_case(order, C, form, layout="packed"):
    """Each case (and the oracle's arena) is computed once and shared, unchanged, by the tests that run it."""
    key = (order, C, form, layout)
    if key not in _cases:
        sizes = ORDERS[order]
        place = [int(x) for x in np.random.default_rng(5).permutation(len(sizes))]
        _cases[key] = ru.UpdateCase(3, 10, sizes, parity(3, 10), edge_changed(sizes, C, 7 * C + len(order)), form=form,
                                    layout=layout, place=place, seed=sorted(ORDERS).index(order))
    return _cases[key]


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("form", ["delta", "oldnew"])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_edge_and_boundary_sizes(knobs, order, C, form, cap):
    """With ZFEC_HIP_GRID_CAP=1 the launch is one workgroup whose four waves
    each cross many stripes: a carried number, mask or table pointer shows."""
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = base_case(order, C, form)
    assert (case.changed == NONE).all(axis=1).any() and (case.changed == NONE).any(axis=1).sum() > 1
    got, name = launch(case)
    assert name == "matupdate_ragged<%d,7>" % C
    check(case, got, (order, C, form, cap))


# ---- 2. the tail unit in another wave's range ----------------------------------------------------------

TAIL4 = [4100, 3077, 3080, 3000]           # 5 + 4 + 4 + 3 units: ranges of four under one workgroup
TAIL5 = [5124, 4101, 4104, 4000]           # 6 + 5 + 5 + 4 units: ranges of five
CYCLE = [2049, 2056, 2063, 4100, 1025, 1030, 1039]


def tail_units(sizes):
    """(unit, stripe, t) of every stripe's byte-tail unit: sizes 1024 w + t, 0 < t < 16."""
    us = rc.units(sizes)
    return [(us[s + 1] - 1, s, sz % 1024) for s, sz in enumerate(sizes) if 0 < sz % 1024 < 16]


def test_tail_units_begin_other_waves_ranges():
    """The arrangement the next test depends on, from the walk's own
    arithmetic: under one workgroup (4 waves) units 4, 8 and 12 of TAIL4 are
    the byte tails of stripes 0, 1 and 2 (t = 4, 5, 8), each the FIRST unit of
    a wave's range, the unit before it -- the same stripe's last whole one --
    being the LAST of the previous wave's, reached three steps in; TAIL5 does
    the same at ranges of five (units 5, 10, 15; four steps in)."""
    for sizes, ustart, per in ((TAIL4, [0, 5, 9, 13, 16], 4), (TAIL5, [0, 6, 11, 16, 20], 5)):
        us = capi.ragged_units(sizes)
        assert us == rc.units(sizes) == ustart
        ranges = rc.wave_ranges(us[-1], 4)
        assert ranges == [(g * per, (g + 1) * per) for g in range(4)]
        assert tail_units(sizes) == [(per, 0, 4), (2 * per, 1, 5), (3 * per, 2, 8)]
        for g, (unit, s, t) in enumerate(tail_units(sizes), start=1):
            assert ranges[g][0] == unit and ranges[g - 1][1] == unit, "the tail does not begin wave %d's range" % g
            assert rc.stripe_of(us, unit) == rc.stripe_of(us, unit - 1) == s and us[s + 1] == unit + 1
            assert unit - 1 - ranges[g - 1][0] == per - 1
    # the cycle: every stripe of it ends with a byte tail in a unit of its own
    assert len(tail_units([CYCLE[s % 7] for s in range(64)])) == 64


@pytest.mark.parametrize("form", ["delta", "oldnew"])
@pytest.mark.parametrize("sizes", [TAIL4, TAIL5], ids=["ranges-of-4", "ranges-of-5"])
def test_tail_unit_first_of_a_waves_range(knobs, sizes, form):
    """One workgroup.  An overlapped last chunk would re-read, from the wave
    that owns the tail, the 16 - t bytes before it, which the previous wave
    updates three (or four) steps later or has updated already: wrong bytes at
    sz - 16 .. of those stripes."""
    knobs(ZFEC_HIP_GRID_CAP=1)
    changed = random_changed(np.random.default_rng(2), 3, len(sizes), 2, none=0.0)
    case = ru.UpdateCase(3, 10, sizes, parity(3, 10), changed, form=form, seed=21)
    got, name = launch(case)
    assert name == "matupdate_ragged<2,7>"
    check(case, got, (sizes, form))


_cycle = {}


@pytest.mark.parametrize("form", ["delta", "oldnew"])
@pytest.mark.parametrize("cap", [None, 2, 1])
def test_tail_units_in_a_cycle_of_sizes(knobs, cap, form):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    if form not in _cycle:
        sizes = [CYCLE[s % 7] for s in range(64)]
        changed = random_changed(np.random.default_rng(3), 3, 64, 2, none=0.0)
        _cycle[form] = ru.UpdateCase(3, 10, sizes, parity(3, 10), changed, form=form, seed=22)
    got, name = launch(_cycle[form])
    assert name == "matupdate_ragged<2,7>"
    check(_cycle[form], got, (cap, form))


# ---- 3. every <C,R> --------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", range(1, 9))
@pytest.mark.parametrize("C", range(1, 5))
def test_every_shape(knobs, C, R):
    """<C,R> for C = 1..4, R = 1..8 under one workgroup, so that waves cross
    stripes; stored rows include a primary, and some slots are none."""
    k, m = 4, 12
    rng = np.random.default_rng(100 * C + R)
    nums = [int(x) for x in rng.permutation(m)[:R]]
    sizes = [0, 1, 17, 1030, 2049, 900]
    changed = random_changed(rng, k, len(sizes), C, none=0.2)
    changed[2] = 1
    case = ru.UpdateCase(k, m, sizes, nums, changed, form="oldnew" if (C + R) % 2 else "delta", seed=100 * C + R)
    knobs(ZFEC_HIP_GRID_CAP=1)
    got, name = launch(case)
    assert name == "matupdate_ragged<%d,%d>" % (C, R)
    check(case, got, (C, R))


# ---- 4. row groups and wide codes ------------------------------------------------------------------------

MIXED = [1025, 0, 17, 2049, 1, 3000, 1024, 4100]
WIDE = {"4_20": (4, 20, list(range(4, 20))),                       # 16 rows: 8 + 8
        "10_16": (10, 16, [12, 3, 15, 10, 0, 13, 11, 14, 7]),      # primaries among the rows: 8 + 1
        "20_24": (20, 24, [20, 21, 22, 23]),
        "20_60": (20, 60, list(range(20, 60)))}                    # 40 rows: five groups


@pytest.mark.parametrize("chw", ["host", "dev"])
@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_row_groups_and_wide_codes(shape, desc, chw):
    """Every code takes the one fused path: each launch is matupdate_ragged,
    nothing is cut into runs, and the last group may have fewer than 8 rows."""
    k, m, nums = WIDE[shape]
    rng = np.random.default_rng(len(shape) + k)
    changed = random_changed(rng, k, len(MIXED), 2)
    case = ru.UpdateCase(k, m, MIXED, nums, changed, form="oldnew", seed=31)
    got, name = launch(case, desc, chw)
    last = len(nums) % 8 or 8
    assert name == "matupdate_ragged<2,%d>" % last, "the last row group's launch: no run of uniform calls"
    check(case, got, (shape, desc, chw))


def test_device_side_arrays_do_not_synchronise():
    """K=20/M=24 with descriptors and numbers on the device and
    FEC_FLAG_ASYNC: the call returns while an earlier long kernel of the stream
    is still queued (the sibling calls cut such a code into runs and wait)."""
    k, m = 20, 24
    changed = random_changed(np.random.default_rng(4), k, len(MIXED), 2)
    case = ru.UpdateCase(k, m, MIXED, parity(k, m), changed, seed=32)
    new = torch.from_numpy(case.newb.copy()).cuda()
    rows = torch.from_numpy(case.rows0.copy()).cuda()
    keep = [words(case.sizes, "dev"), words(case.ioff, "dev"), words(case.roff, "dev"), num_words(case.changed, "dev")]
    code = capi.Code(k, m)
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    torch.cuda._sleep(40_000_000)  # some tens of milliseconds of device time ahead of the call
    code.update_batch_ragged(0, new.data_ptr() + ru.IN_OFF, case.in_bytes, 0, keep[1][1], rows.data_ptr() + ru.OUT_OFF,
                             case.row_bytes, 0, keep[2][1], keep[0][1], case.nums, keep[3][1], case.c, case.ns,
                             stream=torch.cuda.current_stream().cuda_stream, flags=capi.FEC_FLAG_ASYNC)
    done.record()
    returned_early = not done.query()
    assert capi.last_kernel_name() == "matupdate_ragged<2,4>"
    torch.cuda.synchronize()
    check(case, rows.cpu().numpy(), "async")
    assert returned_early, "the call waited for the stream"


# ---- 5. layouts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("layout", ["packed", "shuffled", "block"])
def test_layouts(knobs, layout, cap):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = base_case("permuted", 2, "oldnew", layout)
    assert case.ibs == (sum(case.sizes) + 7 if layout == "block" else 0)
    assert layout == "block" or case.ioff != case.roff, "input and row offsets are to differ"
    got, name = launch(case)
    assert name == "matupdate_ragged<2,7>"
    check(case, got, (layout, cap))


# ---- 6. device-side misuse leaves bytes alone ------------------------------------------------------------------

SIZES13 = [900, 33, 2048, 300, 1025, 17, 4000, 250, 1, 1500, 200, 64, 700]


@pytest.mark.parametrize("cap", [None, 1])
def test_bad_device_side_descriptors_leave_their_stripe_untouched(knobs, cap):
    """Stripes with an input offset past the arena, a size that overruns the
    rows, a size of 2^63, a wrapping offset, and a none slot whose place does
    not exist: each is neither read nor written, its neighbours are right,
    status FEC_OK.  The tensors end 8 KiB past the extents the call declares."""
    bad = {1: "in", 3: "rows", 5: "size", 7: "none slot", 10: "wrap"}
    changed = random_changed(np.random.default_rng(6), 3, len(SIZES13), 2, none=0.0)
    changed[7] = [1, NONE]
    case = ru.UpdateCase(3, 10, SIZES13, parity(3, 10), changed, form="oldnew", seed=13, skip=set(bad))
    ioff, roff, szs = list(case.ioff), list(case.roff), list(SIZES13)
    ioff[1] = case.in_bytes + 100
    roff[3] = case.row_bytes - 7 * SIZES13[3] + 1  # its last row ends one byte past the extent
    szs[5] = 2**63
    ioff[7] = case.in_bytes - 2 * SIZES13[7] + 1   # slot 0 fits; the none slot's place ends one byte past
    ioff[10] = 2**64 - 8
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    got, name = launch(case, "dev", "dev", ioff=ioff, roff=roff, sizes=szs, tail=8192)
    assert name == "matupdate_ragged<2,7>"
    check(case, got, ("bad descriptors", cap))
    for s in bad:  # and said once more, stripe by stripe
        for a, b in case.row_spans(s):
            assert (got[a:b] == case.rows0[a:b]).all(), (s, bad[s])


def test_a_wrapping_stride_product_leaves_every_stripe_untouched():
    """(slots - 1) * B wraps 2^64 with a fixed row stride of 2^63 + 8 and three
    rows: no stripe fits, nothing is written."""
    changed = random_changed(np.random.default_rng(7), 3, 4, 1, none=0.0)
    case = ru.UpdateCase(3, 10, [64, 1030, 17, 5], [3, 4, 5], changed, seed=14, skip={0, 1, 2, 3})
    case.rbs = 2**63 + 8
    got, name = launch(case, "dev", "dev")
    check(case, got, "wrapping stride")


@pytest.mark.parametrize("cap", [None, 1])
def test_bad_device_side_numbers_are_none_slots(knobs, cap):
    """k, 255, 0x7FFFFFFF and 0xFFFFFFFE in device memory: the slot is a none,
    the stripe's other slot still counts, every other stripe is right."""
    sizes = SIZES13[:8]
    changed = random_changed(np.random.default_rng(8), 3, len(sizes), 2, none=0.0)
    spoilt = {(0, 1): 3, (2, 0): 255, (4, 1): 0x7FFFFFFF, (6, 0): 0xFFFFFFFE}
    case = ru.UpdateCase(3, 10, sizes, parity(3, 10), changed, seed=15, dead=set(spoilt))
    sent = changed.copy()
    for (s, i), v in spoilt.items():
        sent[s, i] = v
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    got, name = launch(case, "dev", "dev", changed=sent)
    assert name == "matupdate_ragged<2,7>"
    check(case, got, ("bad numbers", cap))
    # host-side numbers of the same kind are refused, naming stripe and slot
    with pytest.raises(capi.FecError, match="fec_update_batch_ragged: stripe 0, slot 1: changed block 3 is neither"):
        launch(case, "dev", "host", changed=sent)


def test_the_same_misuse_with_host_arrays_is_refused():
    changed = random_changed(np.random.default_rng(6), 3, len(SIZES13), 2, none=0.0)
    changed[7] = [1, NONE]
    case = ru.UpdateCase(3, 10, SIZES13, parity(3, 10), changed, form="oldnew", seed=13)
    E = capi.FecError

    def spoil(which, s, v):
        arr = list(getattr(case, which) if which != "sizes" else case.sizes)
        arr[s] = v
        return {which: arr}

    with pytest.raises(E, match="fec_update_batch_ragged: stripe 1 does not fit the inputs"):
        launch(case, **spoil("ioff", 1, case.in_bytes + 100))
    with pytest.raises(E, match="fec_update_batch_ragged: stripe 3 does not fit the rows"):
        launch(case, **spoil("roff", 3, case.row_bytes - 7 * SIZES13[3] + 1))
    with pytest.raises(E, match="fec_update_batch_ragged: stripe 5 does not fit the inputs"):
        launch(case, **spoil("sizes", 5, 2**63))
    with pytest.raises(E, match="fec_update_batch_ragged: stripe 7 does not fit the inputs"):
        launch(case, **spoil("ioff", 7, case.in_bytes - 2 * SIZES13[7] + 1))
    with pytest.raises(E, match="fec_update_batch_ragged: stripe 10 does not fit the inputs"):
        launch(case, **spoil("ioff", 10, 2**64 - 8))


# ---- 7. equivalence ------------------------------------------------------------------------------------------

SMALL = [0, 1, 17, 1025, 2049, 900, 0, 3000]


@pytest.mark.parametrize("form", ["delta", "oldnew"])
def test_equals_update_batch_per_stripe(form):
    changed = random_changed(np.random.default_rng(9), 3, len(SMALL), 2)
    case = ru.UpdateCase(3, 10, SMALL, parity(3, 10), changed, form=form, seed=16)
    got, _ = launch(case)
    check(case, got, "ragged")
    code = capi.Code(3, 10)
    new = torch.from_numpy(case.newb.copy()).cuda()
    old = torch.from_numpy(case.oldb.copy()).cuda() if case.oldb is not None else None
    rows = torch.from_numpy(case.rows0.copy()).cuda()
    for s, sz in enumerate(case.sizes):
        if sz:
            w = np.ascontiguousarray(changed[s] & 0xFFFFFFFF, dtype=np.uint32)
            code.update_batch(old.data_ptr() + ru.IN_OFF + case.ioff[s] if old is not None else 0,
                              new.data_ptr() + ru.IN_OFF + case.ioff[s], sz, 0,
                              rows.data_ptr() + ru.OUT_OFF + case.roff[s], sz, 0, case.nums, w.ctypes.data, 2, sz, 1,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == got).all()


def test_two_updates_compose():
    """A second ragged update over the rows the first left: the rows hold the
    encoding of the primaries after both changes."""
    k, m, nums = 3, 10, parity(3, 10)
    rng = np.random.default_rng(10)
    a = ru.UpdateCase(k, m, SMALL, nums, random_changed(rng, k, len(SMALL), 2), seed=17)
    b = ru.UpdateCase(k, m, SMALL, nums, random_changed(rng, k, len(SMALL), 1), seed=18)
    assert a.roff == b.roff and a.rows0.size == b.rows0.size
    rows = torch.from_numpy(a.rows0.copy()).cuda()
    launch(a, rows=rows)
    got, name = launch(b, rows=rows)
    assert name == "matupdate_ragged<1,7>"
    # rows0_a ^ (want_a ^ rows0_a) ^ (want_b ^ rows0_b): the code is linear, the gaps cancel to the guard
    want = a.want ^ b.want ^ b.rows0
    assert (got == want).all()
    assert not (got == a.want).all()


def test_verify_ragged_is_clean_after_an_update_of_full_stripes():
    """Whole stripes (all m blocks stored, the primaries among the rows): after
    the update fec_verify_batch_ragged finds every stripe consistent, and
    before it the changed ones were not."""
    k, m = 3, 10
    nums = list(range(m))
    changed = random_changed(np.random.default_rng(11), k, len(SMALL), 2)
    changed[3] = [0, 2]
    case = ru.UpdateCase(k, m, SMALL, nums, changed, seed=19)
    got, name = launch(case)
    assert name == "matupdate_ragged<2,2>"  # 10 rows: 8 + 2
    check(case, got, "full stripes")
    arena = torch.from_numpy(got).cuda()
    sz_w, off_w = words(case.sizes, "host"), words(case.roff, "host")
    mism = torch.zeros(case.ns, dtype=torch.int32, device="cuda")
    capi.Code(k, m).verify_batch_ragged(arena.data_ptr() + ru.OUT_OFF, case.row_bytes, 0, off_w[1], sz_w[1], nums,
                                        case.ns, mism.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (mism.cpu().numpy() == 0).all()


# ---- 8. refusals and corner calls ----------------------------------------------------------------------------

def test_page_locked_host_blocks():
    changed = random_changed(np.random.default_rng(12), 3, len(SMALL), 2)
    case = ru.UpdateCase(3, 10, SMALL, parity(3, 10), changed, form="oldnew", seed=20)
    got, name = launch(case, pinned=True, flags=0)
    assert name == "matupdate_ragged<2,7>"
    check(case, got, "page-locked")


def small_case():
    return ru.UpdateCase(3, 10, SMALL, parity(3, 10), random_changed(np.random.default_rng(13), 3, len(SMALL), 2),
                         seed=23)


def raw_call(case, new_ptr, rows_ptr, szw, iow, row, chw):
    capi.Code(case.k, case.m).update_batch_ragged(0, new_ptr, case.in_bytes, 0, iow, rows_ptr, case.row_bytes, 0, row,
                                                  szw, case.nums, chw, case.c, case.ns,
                                                  stream=torch.cuda.current_stream().cuda_stream)


def test_mixed_descriptor_kinds_are_refused():
    case = small_case()
    new, rows = torch.from_numpy(case.newb.copy()).cuda(), torch.from_numpy(case.rows0.copy()).cuda()
    hs, hi, dr = words(case.sizes, "host"), words(case.ioff, "host"), words(case.roff, "dev")
    ch = num_words(case.changed, "host")
    with pytest.raises(capi.FecError, match="fec_update_batch_ragged: sizes, in_offsets and row_offsets are of mixed"):
        raw_call(case, new.data_ptr() + ru.IN_OFF, rows.data_ptr() + ru.OUT_OFF, hs[1], hi[1], dr[1], ch[1])
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == case.rows0).all()


def test_pageable_host_blocks_are_refused():
    case = small_case()
    new = case.newb.copy()
    rows = torch.from_numpy(case.rows0.copy()).cuda()
    hs, hi, hr = words(case.sizes, "host"), words(case.ioff, "host"), words(case.roff, "host")
    ch = num_words(case.changed, "host")
    with pytest.raises(capi.FecError, match="fec_update_batch_ragged takes device or page-locked host memory: newb"):
        raw_call(case, new.ctypes.data + ru.IN_OFF, rows.data_ptr() + ru.OUT_OFF, hs[1], hi[1], hr[1], ch[1])


def test_declines_under_graph_capture():
    case = small_case()
    new, rows = torch.from_numpy(case.newb.copy()).cuda(), torch.from_numpy(case.rows0.copy()).cuda()
    keep = [words(case.sizes, "dev"), words(case.ioff, "dev"), words(case.roff, "dev"), num_words(case.changed, "dev")]
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="fec_update_batch_ragged: the stream is being captured into a graph"):
                raw_call(case, new.data_ptr() + ru.IN_OFF, rows.data_ptr() + ru.OUT_OFF, keep[0][1], keep[1][1],
                         keep[2][1], keep[3][1])
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == case.rows0).all()  # nothing was enqueued
    got, name = launch(case)  # a normal call afterwards works
    check(case, got, "after the capture")


def test_all_zero_sizes_launch_nothing():
    """No kernel runs (the last kernel's name stays what an earlier call left)
    and nothing is written; nstripes == 0 is FEC_OK too."""
    marker = ru.UpdateCase(3, 10, [64], [5], [[1]], seed=1)
    _, before = launch(marker)
    assert before == "matupdate_ragged<1,1>"
    case = ru.UpdateCase(3, 10, [0, 0, 0], parity(3, 10), [[0, 1], [2, NONE], [1, 1]], seed=24)
    got, name = launch(case)
    assert name == before
    check(case, got, "all-zero sizes")
    empty = ru.UpdateCase(3, 10, [], parity(3, 10), np.zeros((0, 2), dtype=np.int64), seed=25)
    got, name = launch(empty)
    assert name == before and (got == empty.rows0).all()


# ---- 9. offsets past 2^32 ------------------------------------------------------------------------------------

def test_far_stripes():
    """70 stripes of 4097 bytes just under 64 MiB apart in both arenas
    (far_arena.far_stripes): rows straddle bytes 2^31 and 2^32 from the base, so
    offsets[s] + i * B needs all 64 bits on both sides.  Old/new form, C = 2."""
    k, m, sz, ns, C = 3, 10, 4097, far_arena.NS, 2
    r = m - k
    rng = np.random.default_rng(far_arena.SEED)
    data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
    changed = random_changed(rng, k, ns, C)
    changed[32], changed[64], changed[69] = [0, 2], [1, 1], [-1, 2]
    old = rng.integers(0, 256, size=(ns, C, sz), dtype=np.uint8)
    new = rng.integers(0, 256, size=(ns, C, sz), dtype=np.uint8)
    after = data.copy()
    for s in range(ns):
        for i in range(C):
            if changed[s, i] >= 0:
                after[s, changed[s, i]] ^= old[s, i] ^ new[s, i]
    before_rows, want = encode_all(k, m, data)[:, k:], encode_all(k, m, after)[:, k:]
    src = far_arena.Arena(torch, far_arena.BACKGROUND, far_arena.SRC_ODD)
    dst = far_arena.Arena(torch, far_arena.GUARD, far_arena.DST_ODD)
    lin = far_arena.Layout("far_stripes", 2 * C, sz)  # old slots, then new slots, one stripe stride
    lout = far_arena.Layout("far_stripes", r, sz)
    assert lout.straddlers(2**31) and lout.straddlers(2**32) and lin.straddlers(2**32)
    try:
        src.place(lin, np.concatenate([old, new], axis=1))
        dst.place(lout, before_rows)
        total = src.total()
        keep = [words([sz] * ns, "dev"), words([s * lin.ss for s in range(ns)], "dev"),
                words([s * lout.ss for s in range(ns)], "dev"), num_words(changed, "dev")]
        capi.Code(k, m).update_batch_ragged(src.base, src.base + C * lin.bs, lin.sub(0, C).extent, lin.bs, keep[1][1],
                                            dst.base, lout.extent, lout.bs, keep[2][1], keep[0][1], parity(k, m),
                                            keep[3][1], C, ns, stream=torch.cuda.current_stream().cuda_stream)
        assert capi.last_kernel_name() == "matupdate_ragged<2,7>"
        dst.check(lout, want, "far_stripes")
        far_arena.judge_source(total, src.total(), "far_stripes")
    finally:
        src.t = dst.t = None
        torch.cuda.empty_cache()


# ---- 10. Encoder.update_ragged --------------------------------------------------------------------------------

def test_python_method():
    k, m = 3, 10
    enc = zfec_amd.Encoder(k, m)
    rng = np.random.default_rng(3)
    sizes = [int(x) for x in rng.integers(0, 2500, size=24)]
    changed = random_changed(rng, k, 24, 2)
    for form in ("delta", "oldnew"):
        case = ru.UpdateCase(k, m, sizes, parity(k, m), changed, form=form, seed=26)
        new = torch.from_numpy(case.newb.copy()).cuda()[ru.IN_OFF:ru.IN_OFF + case.in_bytes]
        old = torch.from_numpy(case.oldb.copy()).cuda()[ru.IN_OFF:ru.IN_OFF + case.in_bytes] if form == "oldnew" else None
        want = case.want[ru.OUT_OFF:ru.OUT_OFF + case.row_bytes]
        fresh = lambda: torch.from_numpy(case.rows0.copy()).cuda()[ru.OUT_OFF:ru.OUT_OFF + case.row_bytes]
        dev = lambda x: torch.tensor(x, device="cuda")
        forms = {"list": (sizes, case.roff, case.ioff, changed.tolist()),
                 "numpy": (np.array(sizes), np.array(case.roff), np.array(case.ioff), changed),
                 "host tensor": (torch.tensor(sizes), torch.tensor(case.roff), torch.tensor(case.ioff),
                                 torch.from_numpy(changed)),
                 "device tensor": (dev(sizes), dev(case.roff), dev(case.ioff), torch.from_numpy(changed).cuda()),
                 "device descriptors, host numbers": (dev(sizes), dev(case.roff), dev(case.ioff), changed)}
        for what, (szs, roff, ioff, ch) in forms.items():
            par = fresh()
            out = enc.update_ragged(par, szs, ch, new, old=old, offsets=roff, in_offsets=ioff)
            assert out is par and capi.last_kernel_name() == "matupdate_ragged<2,7>", what
            assert (out.cpu().numpy() == want).all(), (form, what)
        # default offsets: the packed layouts without gaps
        packed_in = lambda a: torch.from_numpy(np.concatenate(
            [a[ru.IN_OFF + case.ioff[s]:][:2 * sz] for s, sz in enumerate(sizes)])).cuda()
        packed_rows = lambda a: np.concatenate([a[ru.OUT_OFF + case.roff[s]:][:7 * sz] for s, sz in enumerate(sizes)])
        out = enc.update_ragged(torch.from_numpy(packed_rows(case.rows0)).cuda(), sizes, changed, packed_in(case.newb),
                                old=packed_in(case.oldb) if form == "oldnew" else None)
        assert (out.cpu().numpy() == packed_rows(case.want)).all(), form
    # one changed block per stripe as a 1-D changed, explicit blocknums with a primary among them
    nums = [9, 0, 4]
    one = rng.integers(0, k, size=24)
    case = ru.UpdateCase(k, m, sizes, nums, one.reshape(24, 1), seed=27)
    par = torch.from_numpy(case.rows0.copy()).cuda()[ru.OUT_OFF:ru.OUT_OFF + case.row_bytes]
    new = torch.from_numpy(case.newb.copy()).cuda()[ru.IN_OFF:ru.IN_OFF + case.in_bytes]
    enc.update_ragged(par, sizes, one, new, blocknums=nums, offsets=case.roff, in_offsets=case.ioff)
    assert capi.last_kernel_name() == "matupdate_ragged<1,3>"
    assert (par.cpu().numpy() == case.want[ru.OUT_OFF:ru.OUT_OFF + case.row_bytes]).all()
    # the library's checks come through as Errors; nothing to do is not one
    bad = list(case.roff)
    bad[2] = case.row_bytes
    assert sizes[2] > 0
    with pytest.raises(zfec_amd.Error, match="stripe 2 does not fit the rows"):
        enc.update_ragged(par, sizes, one, new, blocknums=nums, offsets=bad, in_offsets=case.ioff)
    with pytest.raises(zfec_amd.Error, match="but one was 3"):
        enc.update_ragged(par, sizes, [3] * 24, new, blocknums=nums)
    with pytest.raises(zfec_amd.Error, match="all on parity's device or all on the CPU"):
        enc.update_ragged(par, torch.tensor(sizes, device="cuda"), one, new, blocknums=nums, offsets=case.roff)
    with pytest.raises(zfec_amd.Error, match="new is required to be on parity's device"):
        enc.update_ragged(par, sizes, one, new.cpu(), blocknums=nums)
    assert enc.update_ragged(par, [], [], new) is par
