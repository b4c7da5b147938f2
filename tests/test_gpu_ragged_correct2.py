"""The ragged pair correction on the GPU (fec_correct2_batch_ragged;
zfec_amd/csrc/kernels.hip matcorrect_ragged<K> for the single slots, then
pairs_locate_ragged, pairs_finish and pairs_correct_ragged over the dirty list,
for k <= 4 and 4 to 8 checks; fec_correct_batch_ragged's path below 4 checks;
one fec_correct2_batch per run for other shapes).  The cases are
test_gpu_ragged_locate2.py's.  Both verdict planes are compared with the CPU
model's (tests/ragged_pairs_case.py), and the WHOLE arena after the call with
the expected one: healed stripes equal to the never-corrupted arena, every
other byte as on entry, the gaps, the 64-byte tail past the declared extent and
the IN_OFF lead included.  fec_verify_batch_ragged then sets no bit for any
stripe with a slot or pair verdict."""
import numpy as np
import pytest

import zfec_amd

import ragged_pairs_case as rp
import ragged_scrub_case as sc
import test_gpu_ragged_locate2 as loc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("layout", ["packed", "shuffled", "block"])
@pytest.mark.parametrize("order", sorted(rp.ORDERS))
def test_every_pair_every_placement_is_healed(order, layout, desc):
    loc.check_main(True, order, layout, desc)


@pytest.mark.parametrize("res", ["dev", "pinned", "host"])
@pytest.mark.parametrize("desc", ["host", "dev"])
def test_verdict_words_in_device_pinned_and_host_memory(desc, res):
    loc.check_result_memory(True, desc, res)


def test_page_locked_host_arena():
    loc.check_pinned_arena(True)


def test_clean_arena_is_left_alone():
    loc.check_clean(True)


@pytest.mark.parametrize("cap", [None, 1])
def test_unfit_device_side_descriptors(knobs, cap):
    loc.check_unfit(True, knobs, cap)


@pytest.mark.parametrize("desc", ["host", "dev"])
def test_three_corrupt_slots_are_refused_and_nothing_is_written(desc):
    loc.check_triples(True, desc)


@pytest.mark.parametrize("c", [2, 3])
def test_fewer_than_four_checks(c):
    loc.check_few_checks(True, c)


@pytest.mark.parametrize("with_big", [False, True])
@pytest.mark.parametrize("cap", [1, 3])
def test_list_longer_than_the_grid(knobs, cap, with_big):
    loc.check_grid_stride(True, knobs, cap, with_big)


@pytest.mark.parametrize("res", ["dev", "host"])
@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("layout", ["block", "packed"])
def test_wide_code_runs(layout, desc, res):
    loc.check_runs(True, layout, desc, res)


def test_wide_code_unfit_device_side_descriptor():
    loc.check_runs_unfit(True)


def test_equal_sizes_match_the_uniform_call():
    loc.check_equal_sizes(True)


@pytest.mark.parametrize("cap", [None, 1])
def test_tiny_pair_stripes_do_not_reach_the_next_slot(knobs, cap):
    """Sizes 1, 3 and 15 in the packed layout: slot h + 1 begins where slot h
    ends, and after the last slot come 13 to 15 bytes of background and the
    next stripe.  The byte-wise stores of both rewritten slots must end with
    the slot; the last slot is among them."""
    sizes = [1, 3, 15, 1, 3, 15, 1, 3, 15]
    ab = [(0, 1), (2, 6), (5, 6)]
    cor = []
    for s, sz in enumerate(sizes):
        a, b = ab[s // 3]
        cor += [(s, a, sz - 1, 0x11 + s), (s, b, 0, 0x31 + s)]
    case = sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, seed=43)
    clean = sc.ScrubCase(3, 10, sc.NUMS, sizes, (), seed=43)
    model = rp.Model(case)
    assert [model.pair_of(s) for s in range(9)] == [ab[s // 3] for s in range(9)]
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    planes, name, after, _ = rp.call(case, True)
    assert name == "pairs_correct_ragged"
    rp.judge(model, planes, after, ("tiny", cap), True)
    loc.healed_is_clean(model, clean, after)
    for s, sz in enumerate(sizes):  # said once more: the byte after the last slot
        assert after[sc.IN_OFF + case.soff[s] + 7 * sz] == sc.BACKGROUND, s


def test_python_method():
    dec = zfec_amd.Decoder(3, 10)
    case, clean, model, _, _ = rp.main_case("permuted")
    n = sc.IN_OFF + case.src_bytes
    want = torch.from_numpy(model.planes.view(np.int32).copy())
    for dev in (False, True):
        full = torch.from_numpy(case.src.copy()).cuda()
        arena = full[sc.IN_OFF:n]
        szs = torch.tensor(case.sizes, device="cuda") if dev else case.sizes
        offs = torch.tensor(case.soff, device="cuda") if dev else case.soff
        got = dec.correct2_ragged(arena, szs, case.nums, offsets=offs)
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, case.ns) and got.is_cuda
        assert torch.equal(got.cpu(), want)
        assert (full.cpu().numpy() == clean.src).all()
        assert not dec.verify_ragged(arena, szs, case.nums, offsets=offs).any()
    # default offsets: the packed layout without gaps
    packed = torch.from_numpy(np.concatenate([case.stripe_blocks(s).reshape(-1) for s in range(case.ns)])).cuda()
    healed = np.concatenate([clean.stripe_blocks(s).reshape(-1) for s in range(case.ns)])
    assert torch.equal(dec.correct2_ragged(packed, case.sizes, case.nums).cpu(), want)
    assert (packed.cpu().numpy() == healed).all()
    assert tuple(dec.correct2_ragged(packed, [], case.nums).shape) == (2, 0)
    first = next(s for s, sz in enumerate(case.sizes) if sz)
    with pytest.raises(zfec_amd.Error, match="fec_correct2_batch_ragged: stripe %d does not fit blocks" % first):
        bad = list(case.soff)
        bad[first] = case.src_bytes
        dec.correct2_ragged(torch.from_numpy(case.src.copy()).cuda()[sc.IN_OFF:n], case.sizes, case.nums,
                            offsets=bad)
