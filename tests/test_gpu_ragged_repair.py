"""The ragged repair on the GPU (fec_repair_batch_ragged; zfec_amd/csrc/kernels.hip
matrepair_ragged<K,R> for k <= 4, runs of shared-matrix launches for wider
codes): every stripe its own size and its own pattern.  The whole output arena,
pre-filled with the guard byte, is compared with what the CPU oracle expects
(tests/ragged_repair_case.py): decode from the stripe's present blocks, then
encode the target.  So the rows of FEC_REPAIR_NONE targets, the gaps, the
stripes that are to be skipped and the tail must all keep their fill, and the
source must come back unchanged."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import ragged_repair_case as rr

rc = rr.rc
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NONE = rr.NONE


def words(vals, where):
    """nstripes 8-byte words in host (numpy) or device (torch) memory: (keep-alive, address)."""
    a = np.array([int(v) % 2**64 for v in vals], dtype=np.uint64)
    if where == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t, t.data_ptr()


def id_words(ids, where):
    """nstripes uint32 ids in host or device memory, or none ("null")."""
    if where == "null":
        return None, 0
    a = np.array([int(v) % 2**32 for v in ids], dtype=np.uint32)
    if where == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int32)).cuda()
    return t, t.data_ptr()


def launch(case, desc="host", idw="host", pinned=False, soff=None, doff=None, sizes=None, ids=None, tail=0,
           present=None, targets=None):
    """One call over fresh copies of the case's arenas, which end `tail` bytes
    past what the case holds; returns (the whole output tensor, the last
    kernel's name).  The source must come back unchanged."""
    src_h = np.concatenate([case.src, np.full(tail, rr.BACKGROUND, dtype=np.uint8)])
    dst_h = np.full(case.want.size + tail, rr.GUARD, dtype=np.uint8)
    if pinned:
        src, dst = torch.from_numpy(src_h.copy()).pin_memory(), torch.from_numpy(dst_h).pin_memory()
    else:
        src, dst = torch.from_numpy(src_h).cuda(), torch.from_numpy(dst_h).cuda()
    keep = [words(case.sizes if sizes is None else sizes, desc), words(case.soff if soff is None else soff, desc),
            words(case.doff if doff is None else doff, desc), id_words(case.ids if ids is None else ids, idw)]
    capi.Code(case.k, case.m).repair_batch_ragged(
        src.data_ptr() + rr.IN_OFF, case.src_bytes, case.sbs, keep[1][1], dst.data_ptr() + rr.OUT_OFF,
        case.dst_bytes, case.dbs, keep[2][1], keep[0][1], case.present if present is None else present,
        case.targets if targets is None else targets, keep[3][1], case.ns,
        stream=torch.cuda.current_stream().cuda_stream)
    name = capi.last_kernel_name()
    torch.cuda.synchronize()
    assert (src.cpu().numpy() == src_h).all(), "the source was written"
    got = dst.cpu().numpy()
    assert (got[case.want.size:] == rr.GUARD).all(), "bytes written past the arena"
    return got[:case.want.size], name


def check(case, got, what):
    assert (got == case.want).all(), (what, case.explain(got))


# ---- the edge sizes of K=3/M=10, six patterns --------------------------------------------------

PERM = [int(x) for x in np.random.default_rng(11).permutation(len(rc.EDGE_SIZES))]
ORDERS = {"listed": rc.EDGE_SIZES, "reversed": rc.EDGE_SIZES[::-1], "permuted": [rc.EDGE_SIZES[i] for i in PERM],
          "boundary": rc.BOUNDARY_SIZES}
_cases = {}


def base_case(order, layout="packed"):
    """Each case (and the oracle's arena) is computed once and shared, unchanged, by the tests that run it."""
    key = (order, layout)
    if key not in _cases:
        sizes = ORDERS[order]
        place = [int(x) for x in np.random.default_rng(5).permutation(len(sizes))]
        _cases[key] = rr.RepairCase(3, 10, sizes, rr.PRESENT, rr.TARGETS, rr.cycled_ids(len(sizes), len(rr.PRESENT)),
                                    layout=layout, place=place, seed=sorted(ORDERS).index(order))
    return _cases[key]


def test_the_patterns_are_the_ones_meant():
    masks = [sum(1 for t in row if t != NONE) for row in rr.TARGETS]
    assert sorted(set(masks)) == [0, 1, 2, 3]
    assert any(all(b >= 3 for b in p) for p in rr.PRESENT), "no parity-only pattern"
    assert any((set(t) - {NONE}) & set(p) for p, t in zip(rr.PRESENT, rr.TARGETS)), "no copy row"
    assert len({tuple(sorted(p)) for p in rr.PRESENT}) == len(rr.PRESENT)
    assert any(p != sorted(p) for p in rr.PRESENT), "every pattern in ascending slot order"
    ids = rr.cycled_ids(len(rc.EDGE_SIZES), len(rr.PRESENT))
    assert all(a != b for a, b in zip(ids, ids[1:]))


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_edge_and_boundary_sizes(knobs, order, cap):
    """With ZFEC_HIP_GRID_CAP=1 the launch is one workgroup whose four waves
    each cross many stripes and patterns: a carried id, mask or table shows."""
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = base_case(order)
    got, name = launch(case)
    assert name == "matrepair_ragged<3,3>"
    check(case, got, (order, cap))


def test_boundary_ranges_begin_where_meant():
    ub = capi.ragged_units(rc.BOUNDARY_SIZES)
    assert ub[-1] == 108 and rc.wave_ranges(108, 4) == [(0, 27), (27, 54), (54, 81), (81, 108)]
    s27, s54, s81 = (rc.stripe_of(ub, u) for u in (27, 54, 81))
    assert (ub[s27], rc.BOUNDARY_SIZES[s27 - 1]) == (27, 0) and (ub[s54], rc.BOUNDARY_SIZES[s54 - 1]) == (54, 0)
    assert ub[s81] < 81 < ub[s81 + 1]


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("layout", ["packed", "shuffled", "block"])
def test_layouts(knobs, layout, cap):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = base_case("permuted", layout)
    assert case.sbs == (sum(case.sizes) + 7 if layout == "block" else 0)
    got, name = launch(case)
    assert name == "matrepair_ragged<3,3>"
    check(case, got, (layout, cap))


SMALL = [0, 1, 17, 1025, 2049, 900, 0, 3000]


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("idw", ["host", "dev"])
@pytest.mark.parametrize("desc", ["host", "dev"])
def test_descriptors_and_ids_in_host_and_device_memory(knobs, desc, idw, cap):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = rr.RepairCase(3, 10, SMALL, rr.PRESENT, rr.TARGETS, [5, 0, 1, 2, 4, 3, 0, 1], seed=7)
    got, name = launch(case, desc, idw)
    assert name == "matrepair_ragged<3,3>"
    check(case, got, (desc, idw, cap))


def test_page_locked_host_blocks():
    case = rr.RepairCase(3, 10, SMALL, rr.PRESENT, rr.TARGETS, [5, 0, 1, 2, 4, 3, 0, 1], seed=8)
    got, name = launch(case, pinned=True)
    assert name == "matrepair_ragged<3,3>"
    check(case, got, "page-locked")


def test_one_pattern_without_ids():
    case = rr.RepairCase(3, 10, SMALL, [rr.PRESENT[2]], [rr.TARGETS[2]], [0] * len(SMALL), seed=9)
    for desc in ("host", "dev"):
        got, name = launch(case, desc, "null")
        assert name == "matrepair_ragged<3,3>"
        check(case, got, ("pattern_of NULL", desc))


def test_nothing_to_store_launches_nothing():
    """All targets FEC_REPAIR_NONE, or all sizes zero: no kernel runs (the
    last kernel's name stays what an earlier call left) and nothing is written."""
    marker = rr.RepairCase(3, 10, [64], [rr.PRESENT[0]], [[2]], [0], seed=1)
    for case in (rr.RepairCase(3, 10, SMALL, [rr.PRESENT[3]], [rr.TARGETS[3]], [0] * len(SMALL), seed=10),
                 rr.RepairCase(3, 10, [0, 0, 0], rr.PRESENT, rr.TARGETS, [0, 1, 2], seed=10)):
        _, before = launch(marker)
        assert before == "matrepair_ragged<3,1>"
        got, name = launch(case)
        assert name == before
        check(case, got, "nothing to store")


# ---- row groups --------------------------------------------------------------------------------

def test_row_groups_of_eight_and_three(knobs):
    """ntargets = 11: rows 0-7 and 8-10 over one staging."""
    present = [[0, 1, 5], [9, 4, 6], [7, 2, 0]]
    targets = [[2, 3, 4, 6, 7, 8, 9, 0, 1, NONE, 5], [0, 1, 2, 3, NONE, 5, NONE, 7, 8, 9, 4],
               [NONE] * 8 + [1, NONE, 3]]
    sizes = [1025, 0, 17, 2049, 1, 3000, 1024]
    for cap in (None, 1):
        if cap is not None:
            knobs(ZFEC_HIP_GRID_CAP=cap)
        case = rr.RepairCase(3, 10, sizes, present, targets, rr.cycled_ids(len(sizes), 3), seed=11)
        got, name = launch(case)
        assert name == "matrepair_ragged<3,3>"
        check(case, got, ("8 + 3", cap))


def test_a_row_group_no_pattern_uses_is_skipped():
    present = [[0, 1, 5], [9, 4, 6]]
    targets = [[2, 3, 4, 6, NONE, 8, 9, 0] + [NONE] * 3, [0, 1, NONE, 3, 7, 5, 2, 8] + [NONE] * 3]
    sizes = [1025, 0, 17, 2049]
    case = rr.RepairCase(3, 10, sizes, present, targets, rr.cycled_ids(len(sizes), 2), seed=12)
    got, name = launch(case)
    assert name == "matrepair_ragged<3,8>", "the second group's launch ran"
    check(case, got, "second group unused")


# ---- device-side descriptors that are not to be followed ---------------------------------------

@pytest.mark.parametrize("cap", [None, 1])
def test_bad_device_side_descriptors_leave_their_stripe_untouched(knobs, cap):
    """Stripes with an id >= npatterns, an offset past the source arena, an
    offset past the output arena, a size of 2^63 and a wrapping offset: each
    is neither read nor written, its neighbours are right, status FEC_OK.  Both
    tensors end 8 KiB past the extents the call declares, and the offsets that
    lie past an extent still point into that tail."""
    sizes = [900, 33, 2048, 300, 1025, 17, 4000, 250, 1, 1500, 200, 64, 700]
    bad = {1: "id", 3: "src", 5: "size", 7: "dst", 10: "wrap"}
    ids = [(s + 1) % 6 if (s + 1) % 6 != 3 else 4 for s in range(len(sizes))]  # no all-NONE pattern here
    case = rr.RepairCase(3, 10, sizes, rr.PRESENT, rr.TARGETS, ids, seed=13, skip=set(bad))
    soff, doff, szs, dids = list(case.soff), list(case.doff), list(sizes), list(ids)
    dids[1] = len(rr.PRESENT)
    soff[3] = case.src_bytes + 100
    szs[5] = 2**63
    doff[7] = case.dst_bytes - 3 * sizes[7] + 1  # its last row ends one byte past the extent
    soff[10] = 2**64 - 8
    assert soff[3] + 3 * sizes[3] <= case.src_bytes + 8192
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    got, name = launch(case, "dev", "dev", soff=soff, doff=doff, sizes=szs, ids=dids, tail=8192)
    assert name == "matrepair_ragged<3,3>"
    check(case, got, ("bad descriptors", cap))
    for s in bad:  # and said once more, stripe by stripe
        for a, b in case.row_spans(s):
            assert (got[a:b] == rr.GUARD).all(), (s, bad[s])


def test_mixed_descriptor_kinds_are_refused():
    case = base_case("listed")
    src = torch.from_numpy(case.src.copy()).cuda()
    dst = torch.zeros(case.want.size, dtype=torch.uint8, device="cuda")
    hs, ho, do = words(case.sizes, "host"), words(case.soff, "host"), words(case.doff, "dev")
    ids = id_words(case.ids, "host")
    with pytest.raises(capi.FecError, match="fec_repair_batch_ragged: sizes, src_offsets and dst_offsets are of mixed"):
        capi.Code(3, 10).repair_batch_ragged(src.data_ptr() + rr.IN_OFF, case.src_bytes, 0, ho[1],
                                             dst.data_ptr() + rr.OUT_OFF, case.dst_bytes, 0, do[1], hs[1],
                                             case.present, case.targets, ids[1], case.ns)


def test_pageable_host_blocks_are_refused():
    case = base_case("listed")
    src = case.src.copy()
    dst = torch.zeros(case.want.size, dtype=torch.uint8, device="cuda")
    hs, ho, do = words(case.sizes, "host"), words(case.soff, "host"), words(case.doff, "host")
    ids = id_words(case.ids, "host")
    with pytest.raises(capi.FecError, match="fec_repair_batch_ragged takes device or page-locked host memory"):
        capi.Code(3, 10).repair_batch_ragged(src.ctypes.data + rr.IN_OFF, case.src_bytes, 0, ho[1],
                                             dst.data_ptr() + rr.OUT_OFF, case.dst_bytes, 0, do[1], hs[1],
                                             case.present, case.targets, ids[1], case.ns)


# ---- every shape -------------------------------------------------------------------------------

@pytest.mark.parametrize("r", range(1, 9))
@pytest.mark.parametrize("k", range(1, 5))
def test_every_shape(knobs, k, r):
    """<K,R> for K = 1..4, R = 1..8: two patterns whose masks differ, every
    row live in one of them, under one workgroup so that waves cross stripes."""
    m = 12
    rng = np.random.default_rng(100 * k + r)
    present = [sorted(int(x) for x in rng.choice(m, size=k, replace=False))[::-1],
               [int(x) for x in rng.choice(m, size=k, replace=False)]]
    targets = [[int(x) for x in rng.integers(0, m, size=r)], [int(x) for x in rng.integers(0, m, size=r)]]
    for i in range(r):  # each row is NONE in at most one of the two
        if i % 3 == 1:
            targets[i % 2][i] = NONE
    sizes = [0, 1, 17, 1025, 2049]
    case = rr.RepairCase(k, m, sizes, present, targets, [0, 1, 0, 1, 0], seed=100 * k + r)
    knobs(ZFEC_HIP_GRID_CAP=1)
    got, name = launch(case)
    assert name == "matrepair_ragged<%d,%d>" % (k, r)
    check(case, got, (k, r))


# ---- equivalence -------------------------------------------------------------------------------

def test_equals_repair_batch_per_stripe():
    case = rr.RepairCase(3, 10, SMALL, rr.PRESENT, rr.TARGETS, [5, 0, 1, 2, 4, 3, 0, 1], seed=14)
    got, _ = launch(case)
    check(case, got, "ragged")
    code = capi.Code(3, 10)
    src = torch.from_numpy(case.src.copy()).cuda()
    dst = torch.from_numpy(np.full(case.want.size, rr.GUARD, dtype=np.uint8)).cuda()
    for s, sz in enumerate(case.sizes):
        if sz:
            ids = np.array([case.ids[s]], dtype=np.uint32)
            code.repair_batch(src.data_ptr() + rr.IN_OFF + case.soff[s], sz, 0,
                              dst.data_ptr() + rr.OUT_OFF + case.doff[s], sz, 0, case.present, case.targets,
                              ids.ctypes.data, sz, 1, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == got).all()


def test_targets_of_all_primaries_equal_the_ragged_decode():
    nums = [0, 7, 2]
    case = rr.RepairCase(3, 10, rc.EDGE_SIZES, [nums], [[0, 1, 2]], [0] * len(rc.EDGE_SIZES), seed=15)
    got, name = launch(case, idw="null")
    assert name == "matrepair_ragged<3,3>"
    check(case, got, "decode as repair")
    src = torch.from_numpy(case.src.copy()).cuda()
    dst = torch.from_numpy(np.full(case.want.size, rr.GUARD, dtype=np.uint8)).cuda()
    keep = [words(case.sizes, "host"), words(case.soff, "host"), words(case.doff, "host")]
    capi.Code(3, 10).decode_batch_ragged(src.data_ptr() + rr.IN_OFF, case.src_bytes, 0, keep[1][1],
                                         dst.data_ptr() + rr.OUT_OFF, case.dst_bytes, 0, keep[2][1], keep[0][1], nums,
                                         case.ns, stream=torch.cuda.current_stream().cuda_stream,
                                         flags=capi.FEC_FLAG_ASYNC | capi.FEC_FLAG_ALL_PRIMARIES)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == got).all()


# ---- wider codes: runs ---------------------------------------------------------------------------

@pytest.mark.parametrize("idw", ["host", "dev"])
@pytest.mark.parametrize("desc", ["host", "dev"])
def test_wide_code_runs(desc, idw):
    """K=10/M=16: stripes 0 and 1 are equal, adjacent and share an id, so a run
    of two forms; the rest are runs of one.  A device-side bad id is skipped."""
    k, m = 10, 16
    present = [[0, 1, 2, 13, 4, 5, 15, 7, 8, 9], [12, 11, 10, 15, 14, 13, 0, 1, 2, 3]]
    targets = [[3, 6, NONE, 10], [NONE, 4, 5, 12]]
    sizes = [4096, 4096, 2048, 0, 5000, 1, 2048]
    ids = [0, 0, 1, 1, 0, 1, 1]
    bad = desc == "dev" and idw == "dev"
    case = rr.RepairCase(k, m, sizes, present, targets, ids, seed=16, skip={6} if bad else ())
    dids = list(ids)
    if bad:
        dids[6] = 2
    got, name = launch(case, desc, idw, ids=dids)
    assert name and "_ragged" not in name, name
    check(case, got, ("runs", desc, idw))


# ---- the Python method ---------------------------------------------------------------------------

def test_python_method():
    k, m = 3, 10
    dec = zfec_amd.Decoder(k, m)
    sizes = [int(x) for x in np.random.default_rng(3).integers(0, 2500, size=24)]
    ids = rr.cycled_ids(24, 6)
    case = rr.RepairCase(k, m, sizes, rr.PRESENT, rr.TARGETS, ids, seed=17)
    arena = torch.from_numpy(case.src.copy()).cuda()[rr.IN_OFF:rr.IN_OFF + case.src_bytes]
    want = case.want[rr.OUT_OFF:rr.OUT_OFF + case.dst_bytes]
    # the pattern form, explicit offsets and out: -1 rows keep their contents
    out = torch.full((case.dst_bytes,), rr.GUARD, dtype=torch.uint8, device="cuda")
    res = dec.repair_ragged(arena, sizes, (rr.PRESENT, ids), rr.TARGETS, offsets=case.soff, out=out,
                            out_offsets=case.doff)
    assert res is out and (out.cpu().numpy() == want).all()
    # the per-stripe form on the device, device descriptors
    bn = torch.tensor([rr.PRESENT[i] for i in ids], device="cuda")
    tg = torch.tensor([rr.TARGETS[i] for i in ids], device="cuda")
    out2 = torch.full((case.dst_bytes,), rr.GUARD, dtype=torch.uint8, device="cuda")
    dec.repair_ragged(arena, torch.tensor(sizes, device="cuda"), bn, tg, offsets=torch.tensor(case.soff, device="cuda"),
                      out=out2, out_offsets=torch.tensor(case.doff, device="cuda"))
    assert (out2.cpu().numpy() == want).all()
    # default offsets: the packed layout without gaps, a new output arena
    packed = torch.from_numpy(np.concatenate(
        [case.src[rr.IN_OFF + case.soff[s]:][:k * sz] for s, sz in enumerate(sizes)])).cuda()
    res = dec.repair_ragged(packed, sizes, (rr.PRESENT, ids), rr.TARGETS).cpu().numpy()
    assert res.size == 3 * sum(sizes)
    o = 0
    for s, sz in enumerate(sizes):
        for i, (a, b) in enumerate(case.row_spans(s)):
            if rr.TARGETS[ids[s]][i] != NONE:
                assert (res[o + i * sz:o + (i + 1) * sz] == case.want[a:b]).all(), (s, i)
        o += 3 * sz
    with pytest.raises(zfec_amd.Error, match="stripe 2 does not fit src"):
        bad = list(case.soff)
        bad[2] = case.src_bytes
        assert sizes[2] > 0
        dec.repair_ragged(arena, sizes, (rr.PRESENT, ids), rr.TARGETS, offsets=bad, out=out, out_offsets=case.doff)
    assert dec.repair_ragged(arena, [], (rr.PRESENT, []), rr.TARGETS).numel() == 0
