"""The ragged pair location on the GPU (fec_locate2_batch_ragged;
zfec_amd/csrc/kernels.hip pairs_locate_ragged behind matlocate_ragged<K,R> and
locate2_finish for k <= 4 and 4 to 8 checks, the single-block ragged location
below 4 checks, one fec_locate2_batch per run for other shapes).  Both verdict
planes are compared with the CPU model's (tests/ragged_pairs_case.py) between
guard words, and the whole arena afterwards with the arena on entry.

The check_* functions take `heal` and are shared with
test_gpu_ragged_correct2.py, which runs the same cases through
fec_correct2_batch_ragged."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_pairs_case as rp
import ragged_scrub_case as sc

rc = sc.rc
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def fn_name(heal):
    return "fec_correct2_batch_ragged" if heal else "fec_locate2_batch_ragged"


def kernel(heal):
    """fec_last_kernel_name() where the ragged pair pass ran."""
    return "pairs_correct_ragged" if heal else "pairs_locate_ragged"


def run_kernel(heal):
    """... and after a run of a shape the ragged location cuts, where the uniform pair pass ran."""
    return "pairs_correct" if heal else "pairs_locate"


def single_call(case, heal, desc="host"):
    """The single-block ragged call over the same arena: (verdicts (ns,), its kernel's name)."""
    arena = torch.from_numpy(case.src.copy()).cuda()
    out = torch.full((case.ns,), 0x55, dtype=torch.int32, device="cuda")
    keep = [rp.words(case.sizes, desc), rp.words(case.soff, desc)]
    code = capi.Code(case.k, case.m)
    fn = code.correct_batch_ragged if heal else code.locate_batch_ragged
    fn(arena.data_ptr() + sc.IN_OFF, case.src_bytes, case.sbs, keep[1][1], keep[0][1], case.nums, case.ns,
       out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    name = capi.last_kernel_name()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), name


def healed_is_clean(model, clean, after):
    """After a correction: every stripe with a slot or pair verdict holds the never-corrupted blocks."""
    case = model.case
    for s in model.healed():
        sz = case.sizes[s]
        for j in range(case.nb):
            o = sc.IN_OFF + case.soff[s] + j * (case.sbs or sz)
            assert (after[o:o + sz] == clean.src[o:o + sz]).all(), (s, j)


# ---- the main case ---------------------------------------------------------------------------------------

def check_main(heal, order, layout, desc):
    case, clean, model, pairs, singles = rp.main_case(order, layout)
    assert len(pairs) >= 21 and singles
    planes, name, after, arena = rp.call(case, heal, desc)
    assert name == kernel(heal)
    rp.judge(model, planes, after, (order, layout, desc), heal)
    for s, (ab, _) in pairs.items():
        assert tuple(planes[:, s]) == ab
    if heal:
        healed_is_clean(model, clean, after)
        rp.no_bit_left(model, arena)


@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("layout", ["packed", "shuffled", "block"])
@pytest.mark.parametrize("order", sorted(rp.ORDERS))
def test_every_pair_every_placement(order, layout, desc):
    check_main(False, order, layout, desc)


def check_result_memory(heal, desc, res):
    case, clean, model, _, _ = rp.main_case("permuted")
    planes, name, after, _ = rp.call(case, heal, desc, res)
    assert name == kernel(heal)
    rp.judge(model, planes, after, (desc, res), heal)


@pytest.mark.parametrize("res", ["dev", "pinned", "host"])
@pytest.mark.parametrize("desc", ["host", "dev"])
def test_verdict_words_in_device_pinned_and_host_memory(desc, res):
    check_result_memory(False, desc, res)


def check_pinned_arena(heal):
    case, clean, model, _, _ = rp.main_case("listed")
    planes, name, after, _ = rp.call(case, heal, pinned=True)
    assert name == kernel(heal)
    rp.judge(model, planes, after, "page-locked", heal)


def test_page_locked_host_arena():
    check_pinned_arena(False)


def check_clean(heal):
    _, clean, _, _, _ = rp.main_case("listed")
    model = rp.Model(clean)
    assert (model.planes[0] == rp.CLEAN).all() and (model.planes[1] == rp.NONE).all()
    for desc in ("host", "dev"):
        planes, name, after, _ = rp.call(clean, heal, desc)
        assert name == kernel(heal)  # the pair pass ran, over an empty list
        rp.judge(model, planes, after, ("clean", desc), heal)
        assert (after[:sc.IN_OFF + clean.src_bytes] == clean.src[:sc.IN_OFF + clean.src_bytes]).all()


def test_clean_data():
    check_clean(False)


# ---- device-side descriptors that do not fit ------------------------------------------------------------------

def unfit_case():
    """Twelve stripes, pairs in seven of them; three device-side descriptors do
    not fit the declared extent: offset + size past it, a 64-bit sum that
    wraps, and a stripe that would fit but for its last slot's last byte."""
    sizes = [900, 33, 2048, 300, 1025, 17, 4000, 250, 1, 1500, 200, 64]
    cor = []
    for n, (s, a, b, kind) in enumerate([(0, 1, 4, "first and last"), (3, 2, 5, "same byte"), (4, 0, 6, "one unit"),
                                         (5, 0, 3, "overlapped chunk"), (9, 1, 2, "same byte"),
                                         (10, 4, 6, "first and last"), (11, 3, 5, "whole blocks")]):
        cor += rp.place_pair(s, a, b, sizes[s], kind, n)
    cor.append((7, 6, 249, 0x40))  # a single slot beside them
    case = sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, seed=44)
    soff, szs = list(case.soff), list(sizes)
    soff[3] = case.src_bytes - 7 * sizes[3] + 100  # ends past the extent, in the tail
    soff[5] = 2**64 - 8                            # offset + size wraps
    soff[10] = case.src_bytes - 7 * sizes[10] + 1  # its last slot ends one byte past the extent
    model = rp.Model(case, unfit=(3, 5, 10))
    assert model.planes.T.tolist() == [[1, 4], [rp.CLEAN, rp.NONE], [rp.CLEAN, rp.NONE], [rp.UNFIT, rp.NONE], [0, 6],
                                       [rp.UNFIT, rp.NONE], [rp.CLEAN, rp.NONE], [6, rp.NONE], [rp.CLEAN, rp.NONE],
                                       [1, 2], [rp.UNFIT, rp.NONE], [3, 5]]
    return case, model, soff, szs


def check_unfit(heal, knobs, cap):
    """(UNFIT, NONE), beside pair stripes in the same call, and neither read
    nor written although their bytes are corrupt: the arena, with 8 KiB of
    tail past the declared extent, is as the model expects it."""
    case, model, soff, szs = unfit_case()
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    planes, name, after, _ = rp.call(case, heal, "dev", soff=soff, sizes=szs, tail=8192 + sc.TAIL)
    assert name == kernel(heal)
    rp.judge(model, planes, after, ("unfit", cap), heal, tail=8192 + sc.TAIL)
    for s in (3, 5, 10):  # said once more: as on entry, corrupt bytes included
        o = sc.IN_OFF + case.soff[s]
        assert (after[o:o + 7 * case.sizes[s]] == case.src[o:o + 7 * case.sizes[s]]).all()
    with pytest.raises(capi.FecError, match="%s: stripe 3 does not fit" % fn_name(heal)):
        rp.call(case, heal, "host", soff=soff, sizes=szs, tail=8192 + sc.TAIL)


@pytest.mark.parametrize("cap", [None, 1])
def test_unfit_device_side_descriptors(knobs, cap):
    check_unfit(False, knobs, cap)


# ---- triples: five checks refuse them -------------------------------------------------------------------------

def triples_case():
    sizes = [2049, 17, 900, 0, 1025, 64]
    cor = [(0, 0, 5, 1), (0, 4, 5, 2), (0, 7, 5, 0x80),           # three slots at one byte
           (2, 1, 0, 9), (2, 3, 450, 9), (2, 6, 899, 9),          # three slots at three bytes
           (5, 2, 63, 0x11)]                                      # a single slot
    cor += rp.place_pair(4, 2, 7, 1025, "first and last", 3)      # pairs beside them
    cor += rp.place_pair(1, 0, 5, 17, "overlapped chunk", 4)
    case = sc.ScrubCase(3, 10, rp.NUMS8, sizes, cor, seed=45)
    model = rp.Model(case)  # (verdicts2 asserts, on the CPU, that at most one pair survives)
    assert model.planes.T.tolist() == [[rp.MANY, rp.NONE], [0, 5], [rp.MANY, rp.NONE], [rp.CLEAN, rp.NONE], [2, 7],
                                       [2, rp.NONE]]
    return case, model


def check_triples(heal, desc):
    case, model = triples_case()
    assert case.c == 5
    planes, name, after, _ = rp.call(case, heal, desc)
    assert name == kernel(heal)
    rp.judge(model, planes, after, ("triples", desc), heal)
    for s in (0, 2):  # nothing is written
        o = sc.IN_OFF + case.soff[s]
        assert (after[o:o + 8 * case.sizes[s]] == case.src[o:o + 8 * case.sizes[s]]).all()


@pytest.mark.parametrize("desc", ["host", "dev"])
def test_three_corrupt_slots_are_refused(desc):
    check_triples(False, desc)


# ---- below the pair pass --------------------------------------------------------------------------------------

def check_few_checks(heal, c):
    """Plane 0 is fec_locate_batch_ragged's (the correct call:
    fec_correct_batch_ragged's) verdicts, plane 1 all NONE, the kernel the
    single-block call's."""
    nums = sc.NUMS[:3 + c]
    sizes = [900, 0, 17, 2049, 64, 1]
    cor = [(0, 1, 5, 1), (2, 3, 16, 2), (3, 0, 7, 3), (3, 2, 2048, 4), (5, 4, 0, 5)]
    case = sc.ScrubCase(3, 10, nums, sizes, cor, seed=46 + c)
    model = rp.Model(case)
    assert (model.planes[1] == rp.NONE).all() and (model.planes[0] == case.verdict).all()
    for desc in ("host", "dev"):
        single, single_name = single_call(case, heal, desc)
        planes, name, after, _ = rp.call(case, heal, desc)
        assert name == single_name and "pairs" not in name
        assert name == ("matcorrect_ragged<3>" if heal else "matlocate_ragged<3,%d>" % c)
        assert (planes[0] == single).all() and (planes[1] == rp.NONE).all()
        rp.judge(model, planes, after, (c, desc), heal)


@pytest.mark.parametrize("c", [2, 3])
def test_fewer_than_four_checks(c):
    check_few_checks(False, c)


# ---- the grid-stride walk over the list -----------------------------------------------------------------------

_tiny = {}


def tiny_case(with_big):
    """300 stripes of 1 to 40 bytes, every one a pair; with_big: a 70001-byte
    pair stripe among them, one corrupt byte in its first unit and one in its last."""
    if with_big not in _tiny:
        sizes = [int(x) for x in np.random.default_rng(47).integers(1, 41, size=300)]
        if with_big:
            sizes[137] = 70001
        allp = [(a, b) for a in range(7) for b in range(a + 1, 7)]
        cor = []
        for s, sz in enumerate(sizes):
            a, b = allp[s % 21]
            kind = "first and last" if sz == 70001 else rp.PLACEMENTS[s % 5]
            cor += rp.place_pair(s, b, a, sz, kind, s) if s % 2 else rp.place_pair(s, a, b, sz, kind, s)
        case = sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, seed=48)
        model = rp.Model(case)
        assert all(model.pair_of(s) == allp[s % 21] for s in range(300))
        _tiny[with_big] = (case, sc.ScrubCase(3, 10, sc.NUMS, sizes, (), seed=48), model)
    return _tiny[with_big]


def check_grid_stride(heal, knobs, cap, with_big):
    """ZFEC_HIP_GRID_CAP = 1 and 3: one and three workgroups walk 1200 work
    items (three: an item's share is not the same in every step of a wave),
    and the 70001-byte stripe's 69 units are read 4 apart."""
    case, clean, model = tiny_case(with_big)
    knobs(ZFEC_HIP_GRID_CAP=cap)
    planes, name, after, _ = rp.call(case, heal, "dev")
    assert name == kernel(heal)
    rp.judge(model, planes, after, ("grid-stride", cap, with_big), heal)
    if heal:
        healed_is_clean(model, clean, after)


@pytest.mark.parametrize("with_big", [False, True])
@pytest.mark.parametrize("cap", [1, 3])
def test_list_longer_than_the_grid(knobs, cap, with_big):
    check_grid_stride(False, knobs, cap, with_big)


# ---- runs: wide codes ---------------------------------------------------------------------------------------

def runs_case(layout):
    """K=10/M=16 with 14 slots (c = 4): runs [0, 1], [2, 3, 4] (block layout;
    the packed layout's gaps cut it further), [5], [7].  Pairs in stripe 3, the
    second stripe of the second run, and in stripe 7, the last run: with a
    run's own stripe count as the plane stride, stripe 3's second word would
    land in plane 0 of stripe 6 and stripe 7's in plane 1 of stripe 0."""
    sizes = [1024, 1024, 17, 17, 17, 4097, 0, 1]
    cor = rp.place_pair(3, 2, 11, 17, "overlapped chunk", 0) + rp.place_pair(7, 0, 13, 1, "same byte", 1)
    cor += [(1, 12, 1023, 7), (5, 3, 4096, 1)]  # single slots
    case = sc.ScrubCase(10, 16, list(range(14)), sizes, cor, layout=layout, seed=49)
    model = rp.Model(case)
    assert model.planes.T.tolist() == [[rp.CLEAN, rp.NONE], [12, rp.NONE], [rp.CLEAN, rp.NONE], [2, 11],
                                       [rp.CLEAN, rp.NONE], [3, rp.NONE], [rp.CLEAN, rp.NONE], [0, 13]]
    return case, model


def check_runs(heal, layout, desc, res):
    case, model = runs_case(layout)
    planes, name, after, arena = rp.call(case, heal, desc, res)
    assert name == run_kernel(heal)
    rp.judge(model, planes, after, ("runs", layout, desc, res), heal)
    if heal:
        rp.no_bit_left(model, arena)


@pytest.mark.parametrize("res", ["dev", "host"])
@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("layout", ["block", "packed"])
def test_wide_code_runs(layout, desc, res):
    check_runs(False, layout, desc, res)


def check_runs_unfit(heal):
    case, _ = runs_case("block")
    soff = list(case.soff)
    soff[3] = case.src_bytes  # the pair stripe of the second run
    model = rp.Model(case, unfit=(3,))
    for res in ("dev", "host"):
        planes, name, after, _ = rp.call(case, heal, "dev", res, soff=soff)
        rp.judge(model, planes, after, ("runs, unfit", res), heal)


def test_wide_code_unfit_device_side_descriptor():
    check_runs_unfit(False)


# ---- equal sizes: the uniform call on the same buffer ---------------------------------------------------------

def equal_case():
    ns, sz = 12, 1040
    cor = []
    for n, s in enumerate(range(1, ns, 2)):
        a, b = [(0, 1), (2, 6), (3, 4), (0, 5), (1, 6), (4, 5)][n]
        cor += rp.place_pair(s, a, b, sz, rp.PLACEMENTS[n % 5], n)
    cor.append((4, 3, 1039, 0x21))
    return sc.ScrubCase(3, 10, sc.NUMS, [sz] * ns, cor, layout="block", seed=50)


def check_equal_sizes(heal):
    """Block layout, equal sizes: offsets advance by sz, so the uniform call
    describes the same buffer.  Both planes, and the arena afterwards, are
    exactly the uniform call's."""
    case = equal_case()
    ns, sz = case.ns, case.sizes[0]
    assert case.soff == [s * sz for s in range(ns)]
    planes, name, after, _ = rp.call(case, heal, "dev")
    assert name == kernel(heal)
    arena = torch.from_numpy(np.concatenate([case.src[:sc.IN_OFF + case.src_bytes],
                                             np.full(sc.TAIL, sc.BACKGROUND, dtype=np.uint8)])).cuda()
    out = torch.full((2, ns), 0x55, dtype=torch.int32, device="cuda")
    code = capi.Code(3, 10)
    fn = code.correct2_batch if heal else code.locate2_batch
    fn(arena.data_ptr() + sc.IN_OFF, case.sbs, sz, case.nums, sz, ns, out.data_ptr(),
       stream=torch.cuda.current_stream().cuda_stream)
    assert capi.last_kernel_name() == run_kernel(heal)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == planes).all()
    assert (arena.cpu().numpy() == after).all()
    model = rp.Model(case)
    assert sum(model.pair_of(s) is not None for s in range(ns)) == 6
    rp.judge(model, planes, after, "equal sizes", heal)


def test_equal_sizes_match_the_uniform_call():
    check_equal_sizes(False)


# ---- the Python method ------------------------------------------------------------------------------------

def test_python_method():
    dec = zfec_amd.Decoder(3, 10)
    case, clean, model, _, _ = rp.main_case("permuted")
    n = sc.IN_OFF + case.src_bytes
    want = torch.from_numpy(model.planes.view(np.int32).copy())
    for dev in (False, True):
        full = torch.from_numpy(case.src.copy()).cuda()
        szs = torch.tensor(case.sizes, device="cuda") if dev else case.sizes
        offs = torch.tensor(case.soff, device="cuda") if dev else case.soff
        got = dec.locate2_ragged(full[sc.IN_OFF:n], szs, case.nums, offsets=offs)
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, case.ns) and got.is_cuda
        assert torch.equal(got.cpu(), want)
        assert (full.cpu().numpy() == case.src).all()
    # default offsets: the packed layout without gaps
    packed = torch.from_numpy(np.concatenate([case.stripe_blocks(s).reshape(-1) for s in range(case.ns)])).cuda()
    assert torch.equal(dec.locate2_ragged(packed, case.sizes, case.nums).cpu(), want)
    assert tuple(dec.locate2_ragged(packed, [], case.nums).shape) == (2, 0)
    first = next(s for s, sz in enumerate(case.sizes) if sz)
    with pytest.raises(zfec_amd.Error, match="fec_locate2_batch_ragged: stripe %d does not fit src" % first):
        bad = list(case.soff)
        bad[first] = case.src_bytes
        dec.locate2_ragged(torch.from_numpy(case.src.copy()).cuda()[sc.IN_OFF:n], case.sizes, case.nums, offsets=bad)
