"""The ragged scrub on the GPU (fec_verify_batch_ragged / fec_locate_batch_ragged;
zfec_amd/csrc/kernels.hip matverify_ragged<K,R>, matlocate_ragged<K,R> and
ragged_unfit for k <= 4, runs of uniform launches for the other shapes): every
stripe its own size, its mismatch bits and its verdict compared with the CPU
model per stripe (tests/ragged_scrub_case.py), the source compared byte for
byte before and after, and the result words surrounded by guard words that
must keep their fill."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import far_arena
import ragged_scrub_case as sc

rc = sc.rc
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD_WORD, LEAD_W, TAIL_W = 0xDEADBEEF, 3, 5
OPS = ["verify", "locate"]


def words(vals, desc):
    """nstripes 8-byte words in host (numpy) or device (torch) memory: (keep-alive, address)."""
    a = np.array([int(v) % 2**64 for v in vals], dtype=np.uint64)
    if desc == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t, t.data_ptr()


def call(code, op, src_ptr, src_bytes, sbs, soff, sizes, nums, desc="host", res="dev", per=1):
    """One call with guarded result words in device or host memory; returns
    ((ns, per) uint32, the last kernel's name)."""
    ns = len(sizes)
    fill = np.full(LEAD_W + ns * per + TAIL_W, GUARD_WORD, dtype=np.uint32)
    if res == "dev":
        out = torch.from_numpy(fill.view(np.int32)).cuda()
        ptr = out.data_ptr() + 4 * LEAD_W
    else:
        out = fill
        ptr = out.ctypes.data + 4 * LEAD_W
    keep = [words(sizes, desc), words(soff, desc)]
    fn = code.verify_batch_ragged if op == "verify" else code.locate_batch_ragged
    fn(src_ptr, src_bytes, sbs, keep[1][1], keep[0][1], nums, ns, ptr,
       stream=torch.cuda.current_stream().cuda_stream)
    if res == "dev":
        torch.cuda.synchronize()
        out = out.cpu().numpy().view(np.uint32)
    # (host-side result words: the call is synchronous)
    assert (out[:LEAD_W] == GUARD_WORD).all() and (out[LEAD_W + ns * per:] == GUARD_WORD).all(), "guard words written"
    return out[LEAD_W:LEAD_W + ns * per].reshape(ns, per).copy(), capi.last_kernel_name()


def launch(case, op, desc="host", res="dev", soff=None, sizes=None, tail=sc.TAIL, pinned=False):
    """One call over a fresh copy of the case's arena, which ends `tail` bytes
    past the extent the call declares; the source must come back unchanged."""
    host = np.concatenate([case.src[:sc.IN_OFF + case.src_bytes], np.full(tail, sc.BACKGROUND, dtype=np.uint8)])
    src = torch.from_numpy(host).pin_memory() if pinned else torch.from_numpy(host).cuda()
    got, name = call(capi.Code(case.k, case.m), op, src.data_ptr() + sc.IN_OFF, case.src_bytes, case.sbs,
                     case.soff if soff is None else soff, case.sizes if sizes is None else sizes, case.nums, desc, res,
                     case.words if op == "verify" else 1)
    torch.cuda.synchronize()
    assert (src.cpu().numpy() == host).all(), "the source was written"
    return got, name


def expect(case, op):
    return case.want_words if op == "verify" else case.verdict.reshape(-1, 1)


def check(case, op, got, what, want=None):
    want = expect(case, op) if want is None else want
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not bad.size, (what, op, "wrong stripes", bad[:8].tolist(), "sizes", [case.sizes[s] for s in bad[:8]],
                          "got", got[bad[:8]].tolist(), "want", want[bad[:8]].tolist())


# ---- the edge sizes of K=3/M=10 -------------------------------------------------------------------

PERM = [int(x) for x in np.random.default_rng(11).permutation(len(rc.EDGE_SIZES))]
ORDERS = {"listed": rc.EDGE_SIZES, "reversed": rc.EDGE_SIZES[::-1], "permuted": [rc.EDGE_SIZES[i] for i in PERM]}
_cases = {}


def edge_case(order, dirty):
    """Each case (and its model) is computed once and shared, unchanged, by the grids that run it."""
    key = (order, dirty)
    if key not in _cases:
        sizes = ORDERS[order]
        cor = sc.cycled_corrupt(sizes, len(sc.NUMS), last_byte_of=70001) if dirty else ()
        _cases[key] = sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, seed=2 * sorted(ORDERS).index(order) + dirty)
    return _cases[key]


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_clean_edge_sizes(knobs, order, op, cap):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = edge_case(order, False)
    got, name = launch(case, op)
    assert name == "mat%s_ragged<3,4>" % op
    assert (got == (0 if op == "verify" else sc.CLEAN)).all(), (order, op, cap, got.reshape(-1).tolist())


def test_the_corruptions_are_the_ones_meant():
    """Every slot and every listed position is hit, and in the reversed order
    the last byte of the 70001-byte stripe -- in the overlapped last chunk --
    is among them (in the listed order that stripe is number 21, a clean one)."""
    for order in ORDERS:
        case = edge_case(order, True)
        assert {j for _, j, _, _ in case.corrupt} == set(range(7))
        for s, sz in enumerate(case.sizes):
            hit = [c for c in case.corrupt if c[0] == s]
            assert len(hit) == (1 if sz and s % 3 else 0)
        kinds = set()
        for s, _, p, _ in case.corrupt:
            sz = case.sizes[s]
            kinds |= {name for name, q in (("first", 0), ("last", sz - 1), ("1023", 1023), ("1024", 1024),
                                           ("sz-17", sz - 17)) if p == q}
        assert kinds == {"first", "last", "1023", "1024", "sz-17"}, (order, kinds)
    rev = edge_case("reversed", True)
    big = rev.sizes.index(70001)
    assert big % 3 and (big, 70000) in {(s, p) for s, _, p, _ in rev.corrupt}


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_one_corrupt_byte_per_dirty_stripe(knobs, order, op, cap):
    """Bits and verdicts equal the model's for every stripe; every stripe with
    s % 3 == 0 stays clean, so no bit is carried across a stripe boundary."""
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = edge_case(order, True)
    got, name = launch(case, op)
    assert name == "mat%s_ragged<3,4>" % op
    check(case, op, got, (order, cap))
    assert (got[0::3] == (0 if op == "verify" else sc.CLEAN)).all(), (order, op, cap)
    if op == "locate":  # one corrupt block with c >= 2 checks is always named
        for s, j, _, _ in case.corrupt:
            assert got[s, 0] == j, (s, j, got[s, 0])


# ---- a stripe spanning two waves ---------------------------------------------------------------------

def test_two_waves_one_stripe(knobs):
    """Under ZFEC_HIP_GRID_CAP=1 the launch has 4 waves of 27 units and the
    70001-byte stripe is units 38-106.  Basis slot 0 is corrupt in unit 40
    (wave 1) and basis slot 1 in unit 60 (wave 2): each wave alone would name
    its slot, the OR over the waves is MANY."""
    us = capi.ragged_units(rc.EDGE_SIZES)
    big = rc.EDGE_SIZES.index(70001)
    assert us[-1] == 108 and (us[big], us[big + 1] - 1) == (38, 106)
    ranges = rc.wave_ranges(108, 4)
    assert ranges == [(0, 27), (27, 54), (54, 81), (81, 108)]
    p0, p1 = 2 * 1024 + 5, 22 * 1024 + 7
    assert (us[big] + p0 // 1024, us[big] + p1 // 1024) == (40, 60)
    assert ranges[1][0] <= 40 < ranges[1][1] and ranges[2][0] <= 60 < ranges[2][1]
    case = sc.ScrubCase(3, 10, sc.NUMS, rc.EDGE_SIZES, [(big, 0, p0, 0x5A), (big, 1, p1, 0xC3)], seed=21)
    assert case.verdict[big] == sc.MANY and case.bits[big].all()
    knobs(ZFEC_HIP_GRID_CAP=1)
    v, _ = launch(case, "verify")
    check(case, "verify", v, "two waves")
    assert v[big, 0] == 0xF and v[big - 1, 0] == 0 and v[big + 1, 0] == 0
    l, _ = launch(case, "locate")
    check(case, "locate", l, "two waves")
    assert l[big, 0] == sc.MANY and l[big - 1, 0] == sc.CLEAN and l[big + 1, 0] == sc.CLEAN
    # each wave's part alone names its slot (the model, then the kernel)
    for j, p in ((0, p0), (1, p1)):
        one = sc.ScrubCase(3, 10, sc.NUMS, rc.EDGE_SIZES, [(big, j, p, 0x5A)], seed=21)
        assert one.verdict[big] == j
        got, _ = launch(one, "locate")
        check(one, "locate", got, ("one wave's part", j))


@pytest.mark.parametrize("op", OPS)
def test_ranges_that_begin_on_a_stripe_boundary(knobs, op):
    """BOUNDARY_SIZES under ZFEC_HIP_GRID_CAP=1: ranges begin at units 27 and
    54, each the first stripe after a run of zero-size stripes, and at unit 81
    in the middle of a stripe; one corruption in each of those three."""
    ub = capi.ragged_units(rc.BOUNDARY_SIZES)
    assert ub[-1] == 108
    s27, s54, s81 = (rc.stripe_of(ub, u) for u in (27, 54, 81))
    assert (ub[s27], rc.BOUNDARY_SIZES[s27 - 1]) == (27, 0) and (ub[s54], rc.BOUNDARY_SIZES[s54 - 1]) == (54, 0)
    assert ub[s81] < 81 < ub[s81 + 1]
    cor = [(s27, 4, 0, 9), (s54, 1, 1023, 0x80), (s81, 6, 1024, 1)]  # the last in the split stripe's second unit
    case = sc.ScrubCase(3, 10, sc.NUMS, rc.BOUNDARY_SIZES, cor, seed=22)
    knobs(ZFEC_HIP_GRID_CAP=1)
    got, _ = launch(case, op)
    check(case, op, got, "boundary")


# ---- every k, row groups, one check --------------------------------------------------------------------

SIZES40 = [int(x) for x in np.random.default_rng(40).integers(0, 3001, size=40)]


@pytest.mark.parametrize("k,m,nums,vname,lname", [
    (1, 2, [0, 1], "matverify_ragged<1,1>", "matverify_ragged<1,1>"),
    (2, 4, [0, 1, 2, 3], "matverify_ragged<2,2>", "matlocate_ragged<2,2>"),
    (3, 10, list(range(10)), "matverify_ragged<3,7>", "matlocate_ragged<3,7>"),
    (4, 12, list(range(12)), "matverify_ragged<4,8>", "matlocate_ragged<4,8>"),
    (3, 13, list(range(13)), "matverify_ragged<3,2>", None),  # c = 10: groups of 8 and 2; the location in runs
    (3, 10, [7, 0, 4, 1], "matverify_ragged<3,1>", "matverify_ragged<3,1>"),  # c = 1: UNKNOWN
])
def test_every_k_and_row_groups(k, m, nums, vname, lname):
    cor = sc.third_corrupt(SIZES40, len(nums), seed=k * 16 + m)
    case = sc.ScrubCase(k, m, nums, SIZES40, cor, seed=100 + k * 16 + m)
    dirty = sorted({s for s, _, _, _ in cor})
    assert len(dirty) >= 12
    v, name = launch(case, "verify")
    assert name == vname
    check(case, "verify", v, (k, m))
    l, name = launch(case, "locate")
    if lname is None:
        assert name and "_ragged" not in name, name
    else:
        assert name == lname
    check(case, "locate", l, (k, m))
    if len(nums) == k + 1:
        assert (l[dirty, 0] == sc.UNKNOWN).all()


# ---- layouts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
def test_layouts(op):
    place = [int(x) for x in np.random.default_rng(5).permutation(len(SIZES40))]
    cor = sc.third_corrupt(SIZES40, 7, seed=77)
    results = []
    for lay in ("packed", "shuffled", "block"):
        case = sc.ScrubCase(3, 10, sc.NUMS, SIZES40, cor, seed=77, layout=lay, place=place)
        assert case.sbs == (sum(SIZES40) + 7 if lay == "block" else 0)
        got, _ = launch(case, op)
        check(case, op, got, lay)
        results.append(got)
    assert (results[0] == results[1]).all() and (results[0] == results[2]).all()


# ---- descriptor arrays on the host and on the device ------------------------------------------------

@pytest.fixture(scope="module")
def many_small():
    sizes = [s % 41 for s in range(70001)]
    rng = np.random.default_rng(50)
    cor = []
    for s in sorted(int(x) for x in rng.choice(70001, size=80, replace=False)):
        if sizes[s] and len(cor) < 50:
            cor.append((s, int(rng.integers(0, 7)), int(rng.integers(0, sizes[s])), int(rng.integers(1, 256))))
    assert len(cor) == 50
    return sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, seed=41)


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("op", OPS)
def test_host_and_device_descriptors_agree(knobs, many_small, op, cap):
    """70 001 stripes of 0 to 40 bytes, past any one tile of ragged_scan: all
    clean except 50."""
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    host, name_h = launch(many_small, op, "host")
    dev, name_d = launch(many_small, op, "dev")
    assert name_h == name_d == "mat%s_ragged<3,4>" % op
    check(many_small, op, host, ("host arrays", cap))
    check(many_small, op, dev, ("device arrays", cap))
    assert (host == dev).all()
    clean = 0 if op == "verify" else sc.CLEAN
    assert int((host != clean).any(axis=1).sum()) == 50


def test_mixed_descriptor_kinds_are_refused():
    case = edge_case("listed", False)
    src = torch.from_numpy(case.src.copy()).cuda()
    out = torch.zeros(case.ns, dtype=torch.int32, device="cuda")
    hs, ds = words(case.sizes, "host"), words(case.soff, "dev")
    code = capi.Code(3, 10)
    for fn, name in ((code.verify_batch_ragged, "fec_verify_batch_ragged"),
                     (code.locate_batch_ragged, "fec_locate_batch_ragged")):
        with pytest.raises(capi.FecError, match=name + ": sizes and src_offsets are of mixed memory kinds"):
            fn(src.data_ptr() + sc.IN_OFF, case.src_bytes, 0, ds[1], hs[1], case.nums, case.ns, out.data_ptr())


# ---- device-side descriptors that do not fit ---------------------------------------------------------

@pytest.mark.parametrize("k,m,nums", [(3, 10, sc.NUMS), (10, 16, list(range(16)))], ids=["fused", "runs"])
@pytest.mark.parametrize("op", OPS)
def test_unfit_stripes_are_marked(op, k, m, nums):
    """The arena is declared 8 KiB short of its true end and three device-side
    descriptors point past the declared extent, into that allocated tail; a
    fourth has a size larger than the extent (ragged_scan gives it no units).
    All four come back marked -- every check bit, or FEC_LOCATE_UNFIT -- with
    status FEC_OK, every other stripe is as the model says and the source is
    unchanged.  Whether the kernel read the skipped bytes cannot be observed
    from outside: nothing points outside the tensor, so a missing fit test
    would show only where the bytes read there happen to disagree, which for
    the stripes placed on background they do (0x3C rows are no codeword)."""
    nb = len(nums)
    sizes = [900, 33, 2048, 300, 1025, 17, 4000, 250, 1, 1500, 200, 64]
    cor = [(0, 1, 899, 3), (4, nb - 1, 1024, 0x40), (9, 0, 7, 1), (9, 2, 1400, 2)]
    case = sc.ScrubCase(k, m, nums, sizes, cor, seed=12)
    soff, szs = list(case.soff), list(sizes)
    soff[3] = case.src_bytes + 100                     # begins past the extent
    soff[7] = case.src_bytes - nb * sizes[7] + 1       # its last slot ends one byte past it
    soff[10] = case.src_bytes                          # begins exactly at it
    szs[5] = case.src_bytes + 1                        # larger than the whole arena
    assert soff[3] + nb * sizes[3] <= case.src_bytes + 8192
    got, name = launch(case, op, "dev", soff=soff, sizes=szs, tail=8192 + sc.TAIL)  # raises unless FEC_OK
    if k <= 4:
        assert name == "mat%s_ragged<3,4>" % op
    want = expect(case, op).copy()
    for s in (3, 5, 7, 10):
        want[s] = case.all_bits() if op == "verify" else sc.UNFIT
    check(case, op, got, "unfit", want)


# ---- offsets past 2 GiB and 4 GiB ---------------------------------------------------------------------

def test_far_offsets():
    """Five packed stripes placed so that, from the base, one straddles 2^31,
    one 2^32 and one begins past 2^32; two of them hold a corrupt byte past
    the edge.  A truncated offset would read background (far_arena's rule: every
    alias lies inside the arena), which is no codeword, so the clean stripes
    would come back dirty.  The arena's byte sum must not change."""
    k, m, nums = 3, 10, sc.NUMS
    nb = len(nums)
    sizes = [3001, 1, 4097, 0, 2500]
    offs = [2**31 - 1000, 2**31 + 2**20 + 7, 2**32 - 2000, 12345, 2**32 + 2**28 + 3]
    for o, edge in ((offs[0], 2**31), (offs[2], 2**32)):
        assert o < edge < o + min(sizes[0], sizes[2])  # slot 0 straddles it
    cor = [(0, 0, 2000, 0x21), (4, 5, 2499, 0x80)]
    assert offs[0] + 2000 > 2**31
    case = sc.ScrubCase(k, m, nums, sizes, cor, seed=31)
    assert case.verdict.tolist() == [0, sc.CLEAN, sc.CLEAN, sc.CLEAN, 5]
    src = far_arena.Arena(torch, far_arena.BACKGROUND, far_arena.SRC_ODD)
    for s, sz in enumerate(sizes):
        if sz:
            src.place(far_arena.Layout("far_pair", nb, sz, 1, offs[s], (sz, 0)), case.stripe_blocks(s))
    before = src.total()
    code = capi.Code(k, m)
    for desc in ("host", "dev"):
        for op in OPS:
            got, name = call(code, op, src.base, far_arena.SPAN, 0, offs, sizes, nums, desc, "dev",
                             case.words if op == "verify" else 1)
            assert name == "mat%s_ragged<3,4>" % op
            check(case, op, got, ("far offsets", desc))
    far_arena.judge_source(before, src.total(), "far offsets")


# ---- wider codes: runs of uniform launches -------------------------------------------------------------

@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("op", OPS)
def test_wide_code_runs(op, desc):
    sizes = [4096] * 5 + [2048] * 3 + [0] + [5000]
    cor = [(1, 3, 4095, 1), (4, 12, 0, 0xFF), (6, 0, 100, 2), (6, 15, 2047, 4), (9, 9, 4999, 0x10)]
    case = sc.ScrubCase(10, 16, list(range(16)), sizes, cor, seed=16)
    assert case.verdict.tolist() == [sc.CLEAN, 3, sc.CLEAN, sc.CLEAN, 12, sc.CLEAN, sc.MANY, sc.CLEAN, sc.CLEAN, 9]
    got, name = launch(case, op, desc)
    assert name and "_ragged" not in name, name
    check(case, op, got, (op, desc))


# ---- other memory, and the Python methods ----------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k,m,nums", [(3, 10, sc.NUMS), (10, 16, list(range(16)))], ids=["fused", "runs"])
def test_result_words_in_host_memory(op, k, m, nums):
    sizes = SIZES40[:16]
    case = sc.ScrubCase(k, m, nums, sizes, sc.third_corrupt(sizes, len(nums), seed=8), seed=8)
    for desc in ("host", "dev"):
        got, _ = launch(case, op, desc, res="host")  # synchronous: read without a sync of ours
        check(case, op, got, ("host result", desc))


@pytest.mark.parametrize("op", OPS)
def test_page_locked_host_source(op):
    sizes = SIZES40[:16]
    case = sc.ScrubCase(3, 10, sc.NUMS, sizes, sc.third_corrupt(sizes, 7, seed=9), seed=9)
    got, name = launch(case, op, pinned=True)
    assert name == "mat%s_ragged<3,4>" % op
    check(case, op, got, "page-locked source")


def test_pageable_host_source_is_refused():
    case = edge_case("listed", False)
    host = case.src.copy()
    out = torch.zeros(case.ns, dtype=torch.int32, device="cuda")
    hs, ho = words(case.sizes, "host"), words(case.soff, "host")
    with pytest.raises(capi.FecError, match="fec_verify_batch_ragged takes device or page-locked host memory"):
        capi.Code(3, 10).verify_batch_ragged(host.ctypes.data + sc.IN_OFF, case.src_bytes, 0, ho[1], hs[1], case.nums,
                                             case.ns, out.data_ptr())


def test_python_methods():
    k, m, nums = 3, 10, sc.NUMS
    dec = zfec_amd.Decoder(k, m)
    sizes = [int(x) for x in np.random.default_rng(3).integers(0, 2500, size=24)]
    cor = sc.third_corrupt(sizes, 7, seed=3)
    # the default offsets are the packed layout without gaps: build it from the case's stripes
    case = sc.ScrubCase(k, m, nums, sizes, cor, seed=4)
    packed = np.concatenate([case.stripe_blocks(s).reshape(-1) for s in range(len(sizes))])
    data = torch.from_numpy(packed).cuda()
    want_bits = torch.from_numpy(case.bits)
    want_verdict = torch.from_numpy(case.verdict.view(np.int32).copy())
    bits = dec.verify_ragged(data, sizes, nums)                          # sizes as a CPU list
    assert bits.dtype == torch.bool and tuple(bits.shape) == (24, 4) and bits.is_cuda
    assert torch.equal(bits.cpu(), want_bits)
    verdict = dec.locate_ragged(data, sizes, nums)
    assert verdict.dtype == torch.int32 and tuple(verdict.shape) == (24,) and verdict.is_cuda
    assert torch.equal(verdict.cpu(), want_verdict)
    assert zfec_amd.LOCATE_CLEAN in verdict.tolist() and zfec_amd.LOCATE_MANY in verdict.tolist()
    dsizes = torch.tensor(sizes, dtype=torch.int64, device="cuda")       # sizes as a device tensor
    assert torch.equal(dec.verify_ragged(data, dsizes, nums).cpu(), want_bits)
    assert torch.equal(dec.locate_ragged(data, dsizes, nums).cpu(), want_verdict)
    # explicit offsets: the case's own arena, gaps and all, from 5 bytes in
    arena = torch.from_numpy(case.src.copy()).cuda()[sc.IN_OFF:sc.IN_OFF + case.src_bytes]
    doffs = torch.tensor(case.soff, dtype=torch.int64, device="cuda")
    assert torch.equal(dec.verify_ragged(arena, dsizes, nums, offsets=doffs).cpu(), want_bits)
    assert torch.equal(dec.locate_ragged(arena, sizes, nums, offsets=case.soff).cpu(), want_verdict)
    # a device-side descriptor that does not fit: every bit, LOCATE_UNFIT
    bad = doffs.clone()
    bad[2] = case.src_bytes
    assert sizes[2] > 0
    assert dec.verify_ragged(arena, dsizes, nums, offsets=bad)[2].all()
    assert int(dec.locate_ragged(arena, dsizes, nums, offsets=bad)[2]) == zfec_amd.LOCATE_UNFIT
    with pytest.raises(zfec_amd.Error, match="stripe 2 does not fit src"):
        dec.locate_ragged(arena, sizes, nums, offsets=bad.tolist())
    # no stripes
    assert tuple(dec.verify_ragged(data, [], nums).shape) == (0, 4)
    assert tuple(dec.locate_ragged(data, [], nums).shape) == (0,)
