"""The ragged in-place correction on the GPU (fec_correct_batch_ragged;
zfec_amd/csrc/kernels.hip matcorrect_ragged<K> after the ragged location for
k <= 4 and at most 8 checks, the uniform correction per run for other shapes).
The verdicts are compared with the CPU model's (tests/ragged_scrub_case.py),
and the WHOLE arena after the call with the arena that was never corrupted:
corrected stripes restored, every other byte as on entry, gaps and tail
included.  The result words sit between guard words that must keep their
fill."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_scrub_case as sc

rc = sc.rc
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD_WORD, LEAD_W, TAIL_W = 0xDEADBEEF, 3, 5


def words(vals, desc):
    """nstripes 8-byte words in host (numpy) or device (torch) memory: (keep-alive, address)."""
    a = np.array([int(v) % 2**64 for v in vals], dtype=np.uint64)
    if desc == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t, t.data_ptr()


def heal(case, desc="host", res="dev", soff=None, sizes=None, tail=sc.TAIL, pinned=False):
    """One call over a fresh copy of the case's arena, which ends `tail` bytes
    past the extent the call declares, with guarded verdict words in device or
    host memory.  Returns (verdicts (ns,), the last kernel's name, the arena
    afterwards, the device tensor that holds it)."""
    ns = case.ns
    host = np.concatenate([case.src[:sc.IN_OFF + case.src_bytes], np.full(tail, sc.BACKGROUND, dtype=np.uint8)])
    arena = torch.from_numpy(host.copy()).pin_memory() if pinned else torch.from_numpy(host).cuda()
    fill = np.full(LEAD_W + ns + TAIL_W, GUARD_WORD, dtype=np.uint32)
    if res == "dev":
        out = torch.from_numpy(fill.view(np.int32)).cuda()
        ptr = out.data_ptr() + 4 * LEAD_W
    else:
        out = fill
        ptr = out.ctypes.data + 4 * LEAD_W
    keep = [words(case.sizes if sizes is None else sizes, desc), words(case.soff if soff is None else soff, desc)]
    capi.Code(case.k, case.m).correct_batch_ragged(arena.data_ptr() + sc.IN_OFF, case.src_bytes, case.sbs, keep[1][1],
                                                   keep[0][1], case.nums, ns, ptr,
                                                   stream=torch.cuda.current_stream().cuda_stream)
    name = capi.last_kernel_name()
    if res == "dev":
        torch.cuda.synchronize()
        out = out.cpu().numpy().view(np.uint32)
    # (host-side verdict words: the call is synchronous)
    assert (out[:LEAD_W] == GUARD_WORD).all() and (out[LEAD_W + ns:] == GUARD_WORD).all(), "guard words written"
    torch.cuda.synchronize()
    return out[LEAD_W:LEAD_W + ns].copy(), name, arena.cpu().numpy(), arena


def pair(sizes, corrupt, k=3, m=10, nums=sc.NUMS, seed=0, **kw):
    """(the corrupted case, the same arena never corrupted)."""
    return (sc.ScrubCase(k, m, nums, sizes, corrupt, seed=seed, **kw),
            sc.ScrubCase(k, m, nums, sizes, (), seed=seed, **kw))


def expected_arena(case, clean, tail=sc.TAIL, healed=None):
    """The arena on entry with every stripe whose model verdict is a slot
    (`healed`: those stripes, where a test knows better) taken from the clean
    arena instead."""
    n = sc.IN_OFF + case.src_bytes
    want = np.concatenate([case.src[:n], np.full(tail, sc.BACKGROUND, dtype=np.uint8)])
    if healed is None:
        healed = [s for s in range(case.ns) if case.verdict[s] < case.nb]
    for s in healed:
        sz = case.sizes[s]
        for j in range(case.nb):
            o = sc.IN_OFF + case.soff[s] + j * (case.sbs or sz)
            want[o:o + sz] = clean.src[o:o + sz]
    return want


def judge(case, clean, verdicts, after, what, want_verdict=None, **kw):
    want_verdict = case.verdict if want_verdict is None else want_verdict
    bad = np.flatnonzero(verdicts != want_verdict)
    assert not bad.size, (what, "wrong verdicts at", bad[:8].tolist(), verdicts[bad[:8]].tolist(),
                          want_verdict[bad[:8]].tolist())
    want = expected_arena(case, clean, **kw)
    diff = np.flatnonzero(after != want)
    assert not diff.size, (what, "arena differs at", diff[:8].tolist(), "stripe offsets", case.soff[:8])


def no_bit_left(case, arena):
    """fec_verify_batch_ragged over the healed arena (still on the device)."""
    ns = case.ns
    out = torch.full((ns, case.words), -1, dtype=torch.int32, device="cuda")
    keep = [words(case.sizes, "host"), words(case.soff, "host")]
    capi.Code(case.k, case.m).verify_batch_ragged(arena.data_ptr() + sc.IN_OFF, case.src_bytes, case.sbs, keep[1][1],
                                                  keep[0][1], case.nums, ns, out.data_ptr(),
                                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any(), "a healed stripe is still inconsistent"


# ---- one corrupt byte per dirty stripe, the edge sizes of K=3/M=10 -------------------------------------

PERM = [int(x) for x in np.random.default_rng(11).permutation(len(rc.EDGE_SIZES))]
ORDERS = {"listed": rc.EDGE_SIZES, "reversed": rc.EDGE_SIZES[::-1], "permuted": [rc.EDGE_SIZES[i] for i in PERM]}
_cases = {}


def edge_pair(order):
    """Each pair (and its model) is computed once and shared, unchanged, by the tests that run it."""
    if order not in _cases:
        sizes = ORDERS[order]
        cor = sc.cycled_corrupt(sizes, len(sc.NUMS), last_byte_of=70001)
        _cases[order] = pair(sizes, cor, seed=30 + sorted(ORDERS).index(order))
    return _cases[order]


def test_the_corruptions_are_the_ones_meant():
    """On the CPU: the model's verdict for every corrupted stripe is its slot
    (no stripe is exempt from the byte-for-byte check), every slot and every
    position kind occurs, and the reversed order has the last byte of the
    70001-byte stripe among the corruptions."""
    for order in ORDERS:
        case, clean = edge_pair(order)
        assert {j for _, j, _, _ in case.corrupt} == set(range(7))
        kinds = set()
        for s, j, p, _ in case.corrupt:
            assert case.verdict[s] == j, (order, s, j, case.verdict[s])
            sz = case.sizes[s]
            kinds |= {name for name, q in (("first", 0), ("last", sz - 1), ("1023", 1023), ("1024", 1024),
                                           ("sz-17", sz - 17)) if p == q}
        assert kinds == {"first", "last", "1023", "1024", "sz-17"}, (order, kinds)
        dirty = {s for s, _, _, _ in case.corrupt}
        assert all(case.verdict[s] == sc.CLEAN for s in range(case.ns) if s not in dirty)
        assert (clean.verdict == sc.CLEAN).all() and (clean.src != case.src).sum() == len(case.corrupt)
    rev = edge_pair("reversed")[0]
    big = rev.sizes.index(70001)
    assert (big, 70000) in {(s, p) for s, _, p, _ in rev.corrupt}


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_one_corrupt_byte_per_dirty_stripe_is_healed(knobs, order, desc, cap):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case, clean = edge_pair(order)
    verdicts, name, after, arena = heal(case, desc)
    assert name == "matcorrect_ragged<3>"
    judge(case, clean, verdicts, after, (order, desc, cap))
    assert (after[:sc.IN_OFF + case.src_bytes] == clean.src[:sc.IN_OFF + case.src_bytes]).all()
    no_bit_left(case, arena)


@pytest.mark.parametrize("res", ["dev", "host"])
@pytest.mark.parametrize("desc", ["host", "dev"])
def test_verdict_words_in_host_and_device_memory(desc, res):
    case, clean = edge_pair("permuted")
    verdicts, name, after, _ = heal(case, desc, res)
    assert name == "matcorrect_ragged<3>"
    judge(case, clean, verdicts, after, (desc, res))


def test_page_locked_host_arena():
    case, clean = edge_pair("listed")
    verdicts, name, after, _ = heal(case, pinned=True)
    assert name == "matcorrect_ragged<3>"
    judge(case, clean, verdicts, after, "page-locked")


def test_clean_arena_is_left_alone(knobs):
    _, clean = edge_pair("listed")
    for cap in (None, 1):
        if cap is not None:
            knobs(ZFEC_HIP_GRID_CAP=cap)
        verdicts, name, after, _ = heal(clean)
        assert name == "matcorrect_ragged<3>"
        judge(clean, clean, verdicts, after, ("clean", cap))


# ---- stripes that must not be rewritten ------------------------------------------------------------------

def test_two_corrupt_blocks_are_refused():
    sizes = [900, 2049, 17, 5000, 64]
    case, clean = pair(sizes, [(1, 0, 5, 1), (1, 4, 2048, 2), (3, 6, 4999, 0x80), (4, 2, 0, 9), (4, 3, 63, 9)], seed=41)
    assert case.verdict.tolist() == [sc.CLEAN, sc.MANY, sc.CLEAN, 6, sc.MANY]
    verdicts, _, after, _ = heal(case)
    judge(case, clean, verdicts, after, "MANY")
    n = sc.IN_OFF + case.src_bytes
    for s in (1, 4):  # byte-identical to entry
        o = sc.IN_OFF + case.soff[s]
        assert (after[o:o + 7 * sizes[s]] == case.src[o:o + 7 * sizes[s]]).all()
    assert (after[:n] != case.src[:n]).sum() == 1  # the one healed byte


def test_two_waves_one_stripe(knobs):
    """Under ZFEC_HIP_GRID_CAP=1 the launch has 4 waves of 27 units and the
    70001-byte stripe is units 38-106.  Slot 0 is corrupt in unit 40 (wave 1)
    and slot 1 in unit 60 (wave 2): each wave alone would name its slot, the
    verdict formed over all waves is MANY and the stripe is untouched."""
    us = capi.ragged_units(rc.EDGE_SIZES)
    big = rc.EDGE_SIZES.index(70001)
    assert us[-1] == 108 and (us[big], us[big + 1] - 1) == (38, 106)
    ranges = rc.wave_ranges(108, 4)
    p0, p1 = 2 * 1024 + 5, 22 * 1024 + 7
    assert ranges[1][0] <= us[big] + p0 // 1024 < ranges[1][1] and ranges[2][0] <= us[big] + p1 // 1024 < ranges[2][1]
    case, clean = pair(rc.EDGE_SIZES, [(big, 0, p0, 0x5A), (big, 1, p1, 0xC3)], seed=21)
    assert case.verdict[big] == sc.MANY
    knobs(ZFEC_HIP_GRID_CAP=1)
    verdicts, _, after, _ = heal(case)
    judge(case, clean, verdicts, after, "two waves")
    assert (after[:sc.IN_OFF + case.src_bytes] == case.src[:sc.IN_OFF + case.src_bytes]).all()
    # each wave's part alone is healed, across the wave boundary inside the stripe
    for j, p in ((0, p0), (1, p1)):
        one, _ = pair(rc.EDGE_SIZES, [(big, j, p, 0x5A)], seed=21)
        assert one.verdict[big] == j
        verdicts, _, after, _ = heal(one)
        judge(one, clean, verdicts, after, ("one wave's part", j))


def test_one_check_rewrites_nothing():
    nums = [7, 0, 4, 1]
    sizes = [900, 17, 2049, 0, 64]
    case, clean = pair(sizes, [(0, 1, 5, 1), (2, 3, 2048, 2)], nums=nums, seed=42)
    assert case.verdict.tolist() == [sc.UNKNOWN, sc.CLEAN, sc.UNKNOWN, sc.CLEAN, sc.CLEAN]
    for desc in ("host", "dev"):
        verdicts, name, after, _ = heal(case, desc)
        assert name == "matverify_ragged<3,1>"
        judge(case, clean, verdicts, after, ("c = 1", desc))
        assert (after[:sc.IN_OFF + case.src_bytes] == case.src[:sc.IN_OFF + case.src_bytes]).all()


@pytest.mark.parametrize("cap", [None, 1])
def test_tiny_stripes_do_not_reach_the_next_slot(knobs, cap):
    """Sizes 1, 3 and 15 in the packed layout: slot h + 1 begins where slot h
    ends, and after the last slot come 13 to 15 bytes of background and the
    next stripe.  The byte-wise store must end with the slot."""
    sizes = [1, 3, 15, 1, 3, 15, 1, 3, 15]
    cor = [(s, [0, 5, 6][s // 3], sizes[s] - 1, 0x11 + s) for s in range(9)]
    case, clean = pair(sizes, cor, seed=43)
    assert [int(v) for v in case.verdict] == [0, 0, 0, 5, 5, 5, 6, 6, 6]
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    verdicts, name, after, _ = heal(case)
    assert name == "matcorrect_ragged<3>"
    judge(case, clean, verdicts, after, ("tiny", cap))
    for s, sz in enumerate(sizes):  # said once more: the byte after the last slot
        end = sc.IN_OFF + case.soff[s] + 7 * sz
        assert after[end] == sc.BACKGROUND, s


@pytest.mark.parametrize("cap", [None, 1])
def test_unfit_device_side_descriptors(knobs, cap):
    """The arena is declared 8 KiB short of its true end; three device-side
    descriptors do not fit the declared extent (one has a size past it).
    Their verdict is FEC_LOCATE_UNFIT and nothing is written for them: the
    bytes they point at, and the corrupt bytes of the stripes they stand for,
    are as on entry.  Every other dirty stripe is healed."""
    sizes = [900, 33, 2048, 300, 1025, 17, 4000, 250, 1, 1500, 200, 64]
    cor = [(0, 1, 899, 3), (3, 2, 7, 1), (4, 6, 1024, 0x40), (5, 0, 16, 2), (9, 0, 7, 1), (10, 4, 100, 8), (11, 5, 63, 1)]
    case, clean = pair(sizes, cor, seed=44)
    for s, j, _, _ in cor:
        assert case.verdict[s] == j
    soff, szs = list(case.soff), list(sizes)
    soff[3] = case.src_bytes + 100               # begins past the extent, in the tail
    szs[5] = case.src_bytes + 1                  # larger than the whole arena
    soff[10] = case.src_bytes - 7 * sizes[10] + 1  # its last slot ends one byte past the extent
    assert soff[3] + 7 * sizes[3] <= case.src_bytes + 8192
    want_verdict = case.verdict.copy()
    want_verdict[[3, 5, 10]] = sc.UNFIT
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    verdicts, name, after, _ = heal(case, "dev", soff=soff, sizes=szs, tail=8192 + sc.TAIL)
    assert name == "matcorrect_ragged<3>"
    judge(case, clean, verdicts, after, ("unfit", cap), want_verdict=want_verdict, tail=8192 + sc.TAIL,
          healed=[0, 4, 9, 11])


# ---- every k, 2 and 8 checks; wider codes -----------------------------------------------------------------

@pytest.mark.parametrize("c", [2, 8])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_k_with_two_and_eight_checks(knobs, k, c):
    m = k + 8
    nums = list(range(k + c))[::-1] if c == 8 else list(range(k + c))  # any slot order
    sizes = [0, 1, 17, 1025, 2049]
    nb = k + c
    cor = [(s, (3 * s + k) % nb, sizes[s] - 1 if s % 2 else 0, 0x21 + s) for s in range(1, 5)]
    case, clean = pair(sizes, cor, k=k, m=m, nums=nums, seed=50 + 10 * k + c)
    for s, j, _, _ in cor:
        assert case.verdict[s] == j, (k, c, s, j, case.verdict[s])
    knobs(ZFEC_HIP_GRID_CAP=1)
    verdicts, name, after, arena = heal(case)
    assert name == "matcorrect_ragged<%d>" % k
    judge(case, clean, verdicts, after, (k, c))
    no_bit_left(case, arena)


@pytest.mark.parametrize("desc", ["host", "dev"])
def test_wide_code_runs(desc):
    """K=10/M=16: the location is cut into runs, each followed by the uniform correction."""
    sizes = [4096] * 3 + [2048] * 2 + [0] + [5000]
    cor = [(1, 3, 4095, 1), (2, 12, 0, 0xFF), (3, 0, 100, 2), (3, 15, 2047, 4), (6, 9, 4999, 0x10)]
    case, clean = pair(sizes, cor, k=10, m=16, nums=list(range(16)), seed=16)
    assert case.verdict.tolist() == [sc.CLEAN, 3, 12, sc.MANY, sc.CLEAN, sc.CLEAN, 9]
    verdicts, name, after, arena = heal(case, desc)
    assert name == "rows_correct"
    judge(case, clean, verdicts, after, ("runs", desc))


def test_location_with_more_than_eight_checks_runs():
    """K=3 with 10 checks: the ragged location is cut into runs, and so is the correction."""
    sizes = [1025, 1025, 17, 0, 300]
    cor = [(0, 12, 1024, 1), (2, 1, 16, 7), (4, 5, 0, 0x33)]
    case, clean = pair(sizes, cor, k=3, m=13, nums=list(range(13)), seed=17)
    assert case.verdict.tolist() == [12, sc.CLEAN, 1, sc.CLEAN, 5]
    verdicts, name, after, _ = heal(case)
    assert name == "matcorrect_reg<3>"
    judge(case, clean, verdicts, after, "c = 10")


# ---- the Python method -------------------------------------------------------------------------------------

def test_python_method():
    k, m, nums = 3, 10, sc.NUMS
    dec = zfec_amd.Decoder(k, m)
    sizes = [int(x) for x in np.random.default_rng(3).integers(0, 2500, size=24)]
    cor = sc.cycled_corrupt(sizes, 7)
    case, clean = pair(sizes, cor, seed=4)
    n = sc.IN_OFF + case.src_bytes
    want_verdict = torch.from_numpy(case.verdict.view(np.int32).copy())
    # explicit offsets, descriptors on the CPU and on the device
    for dev in (False, True):
        full = torch.from_numpy(case.src.copy()).cuda()
        arena = full[sc.IN_OFF:n]
        szs = torch.tensor(sizes, device="cuda") if dev else sizes
        offs = torch.tensor(case.soff, device="cuda") if dev else case.soff
        verdict = dec.correct_ragged(arena, szs, nums, offsets=offs)
        assert verdict.dtype == torch.int32 and tuple(verdict.shape) == (24,) and verdict.is_cuda
        assert torch.equal(verdict.cpu(), want_verdict)
        assert (full.cpu().numpy() == clean.src).all()
        assert not dec.verify_ragged(arena, szs, nums, offsets=offs).any()
    # default offsets: the packed layout without gaps
    packed = torch.from_numpy(np.concatenate([case.stripe_blocks(s).reshape(-1) for s in range(24)])).cuda()
    want = np.concatenate([clean.stripe_blocks(s).reshape(-1) for s in range(24)])
    assert torch.equal(dec.correct_ragged(packed, sizes, nums).cpu(), want_verdict)
    assert (packed.cpu().numpy() == want).all()
    assert tuple(dec.correct_ragged(packed, [], nums).shape) == (0,)
    with pytest.raises(zfec_amd.Error, match="fec_correct_batch_ragged: stripe 2 does not fit blocks"):
        bad = list(case.soff)
        bad[2] = case.src_bytes
        assert sizes[2] > 0
        dec.correct_ragged(torch.from_numpy(case.src.copy()).cuda()[sc.IN_OFF:n], sizes, nums, offsets=bad)
