"""Ragged batches on the GPU (fec_encode_batch_ragged / fec_decode_batch_ragged;
zfec_amd/csrc/kernels.hip matapply_ragged<K,R> and ragged_scan for k <= 4, runs
of shared-matrix launches for wider codes): every stripe its own size, checked
bit for bit against the CPU oracle, with every byte before, between and after
the output rows held at its fill (tests/ragged_case.py)."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import far_arena
import ragged_case as rc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def words(vals, desc):
    """nstripes 8-byte words in host (numpy) or device (torch) memory: (keep-alive, address)."""
    a = np.array([int(v) % 2**64 for v in vals], dtype=np.uint64)
    if desc == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t, t.data_ptr()


def launch(case, desc="host", doff=None, out_lead=rc.OUT_OFF, tail=rc.TAIL, src_bytes=None, dst_bytes=None):
    """One call over fresh arenas; returns (the whole output tensor on the
    host, the last kernel's name).  The arenas end `tail` bytes past the
    case's own extents, which are what the call declares unless told."""
    src = torch.from_numpy(np.concatenate([case.src[:rc.IN_OFF + case.src_bytes],
                                           np.full(tail, rc.BACKGROUND, dtype=np.uint8)])).cuda()
    dst = torch.full((out_lead + case.dst_bytes + tail,), rc.GUARD, dtype=torch.uint8, device="cuda")
    keep = [words(case.sizes, desc), words(case.soff, desc), words(case.doff if doff is None else doff, desc)]
    code = capi.Code(case.k, case.m)
    flags = capi.FEC_FLAG_ASYNC | (capi.FEC_FLAG_ALL_PRIMARIES if case.all_primaries else 0)
    fn = code.encode_batch_ragged if case.op == "enc" else code.decode_batch_ragged
    fn(src.data_ptr() + rc.IN_OFF, case.src_bytes if src_bytes is None else src_bytes, case.sbs, keep[1][1],
       dst.data_ptr() + out_lead, case.dst_bytes if dst_bytes is None else dst_bytes, case.dbs, keep[2][1],
       keep[0][1], case.nums, case.ns, stream=torch.cuda.current_stream().cuda_stream, flags=flags)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), capi.last_kernel_name()


def check(case, got, what):
    assert got.shape == case.want.shape, (what, got.shape, case.want.shape)
    assert (got == case.want).all(), (what,) + case.explain(got)


# ---- the edge sizes of K=3/M=10 -------------------------------------------------------------------

PERM = [int(x) for x in np.random.default_rng(11).permutation(len(rc.EDGE_SIZES))]
ORDERS = {"listed": rc.EDGE_SIZES, "reversed": rc.EDGE_SIZES[::-1], "permuted": [rc.EDGE_SIZES[i] for i in PERM]}
OPS = {"enc": dict(op="enc"), "dec": dict(op="dec", nums=[0, 5, 9]),
       "dec_all": dict(op="dec", nums=[0, 5, 9], all_primaries=True)}
_cases = {}


def edge_case(sizes_key, sizes, op):
    """Each case (and its oracle rows) is computed once and shared, unchanged, by the grids that run it."""
    key = (sizes_key, op)
    if key not in _cases:
        seed = 3 * sorted(list(ORDERS) + ["boundary"]).index(sizes_key) + sorted(OPS).index(op)
        _cases[key] = rc.Case(3, 10, sizes=sizes, seed=seed, **OPS[op])
    return _cases[key]


def test_edge_ranges_begin_where_the_test_means_them_to():
    """Under ZFEC_HIP_GRID_CAP=1 the launch has 4 waves of 27 units: in the
    listed order the 69-unit stripe occupies units 38-106, so three of the four
    ranges work inside it -- one runs into it, two begin in its middle; in the
    boundary list two ranges begin on a stripe right after zero-size stripes
    and one mid-stripe."""
    us = capi.ragged_units(rc.EDGE_SIZES)
    assert us == rc.units(rc.EDGE_SIZES) and us[-1] == 108
    big = rc.EDGE_SIZES.index(70001)
    assert (us[big], us[big + 1] - 1) == (38, 106)
    ranges = rc.wave_ranges(108, 4)
    assert [a for a, _ in ranges] == [0, 27, 54, 81] and all(b - a == 27 for a, b in ranges)
    assert [rc.stripe_of(us, a) for a, _ in ranges] == [1, 16, big, big]  # the first range skips stripe 0, which is empty
    assert [a < us[big + 1] and b > us[big] for a, b in ranges] == [False, True, True, True]
    assert all(us[big] < a < us[big + 1] for a, _ in ranges[2:])
    ub = capi.ragged_units(rc.BOUNDARY_SIZES)
    assert ub == rc.units(rc.BOUNDARY_SIZES) and ub[-1] == 108
    s27, s54, s81 = (rc.stripe_of(ub, u) for u in (27, 54, 81))
    assert (s27, ub[s27], rc.BOUNDARY_SIZES[s27 - 1]) == (29, 27, 0)
    assert (s54, ub[s54], rc.BOUNDARY_SIZES[s54 - 1]) == (57, 54, 0)
    assert ub[s81] < 81 < ub[s81 + 1]


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_edge_sizes_k3(knobs, order, op, cap):
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    case = edge_case(order, ORDERS[order], op)
    got, name = launch(case)
    assert name == "matapply_ragged<3,%d>" % case.r
    check(case, got, (order, op, cap))


@pytest.mark.parametrize("op", sorted(OPS))
def test_edge_boundaries_k3(knobs, op):
    knobs(ZFEC_HIP_GRID_CAP=1)
    case = edge_case("boundary", rc.BOUNDARY_SIZES, op)
    got, _ = launch(case)
    check(case, got, ("boundary", op))


# ---- every k, row groups, a primary copy ----------------------------------------------------------

SIZES40 = [int(x) for x in np.random.default_rng(40).integers(0, 3001, size=40)]


@pytest.mark.parametrize("k,m,nums,last", [
    (1, 2, None, "matapply_ragged<1,1>"),
    (2, 4, None, "matapply_ragged<2,2>"),
    (3, 10, None, "matapply_ragged<3,7>"),
    (4, 12, None, "matapply_ragged<4,8>"),
    (3, 12, None, "matapply_ragged<3,1>"),  # 9 rows: groups of 8 and 1
    (3, 10, [3, 1, 9], "matapply_ragged<3,3>"),  # block 1 is a copy of that primary
])
def test_every_k_and_row_groups(k, m, nums, last):
    case = rc.Case(k, m, "enc", SIZES40, nums=nums, seed=100 + k * 16 + m)
    got, name = launch(case)
    assert name == last
    check(case, got, (k, m, nums))


# ---- layouts ---------------------------------------------------------------------------------------

def stripe_rows(case, got):
    return [[got[a:b] for a, b in case.row_spans(s)] for s in range(case.ns)]


def test_layouts():
    place = [int(x) for x in np.random.default_rng(5).permutation(len(SIZES40))]
    cases = [rc.Case(3, 10, "enc", SIZES40, seed=77, layout=lay, place=place)
             for lay in ("packed", "block", "shuffled")]
    rows = []
    for case in cases:
        got, _ = launch(case)
        check(case, got, case.layout)
        rows.append(stripe_rows(case, got))
    for other in rows[1:]:
        for s in range(len(SIZES40)):
            for a, b in zip(rows[0][s], other[s]):
                assert (a == b).all(), ("stripe", s)


# ---- descriptor arrays on the host and on the device ------------------------------------------------

@pytest.mark.parametrize("op", ["enc", "dec"])
def test_host_and_device_descriptors_agree(op):
    case = rc.Case(3, 10, sizes=ORDERS["permuted"] + SIZES40, seed=9, **OPS[op])
    host, name_h = launch(case, "host")
    dev, name_d = launch(case, "dev")
    assert name_h == name_d == "matapply_ragged<3,%d>" % case.r
    check(case, host, "host arrays")
    check(case, dev, "device arrays")
    assert (host == dev).all()


@pytest.fixture(scope="module")
def many_small():
    return rc.Case(3, 10, "enc", [s % 41 for s in range(70001)], seed=41)


@pytest.mark.parametrize("cap", [None, 3])
def test_scan_many_small(knobs, many_small, cap):
    """70 001 stripes of 0 to 40 bytes, past any one tile of ragged_scan."""
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    got, name = launch(many_small, "dev")
    assert name == "matapply_ragged<3,7>"
    check(many_small, got, ("many small", cap))


# ---- device-side descriptors that do not fit ---------------------------------------------------------

def test_unfit_stripes_are_skipped():
    """The arenas are declared 4 KiB short of their true end, and three
    device-side descriptors point into that allocated tail (or wrap): their
    stripes stay untouched, the other nine are exact, the status is FEC_OK.
    Nothing points outside the tensors, so a missing test in the kernel
    shows as a failed comparison."""
    sizes = [900, 33, 2048, 300, 1025, 17, 4000, 250, 1, 1500, 200, 64]
    case = rc.Case(3, 10, "enc", sizes, seed=12)
    lead, tail, r = 67, 4096 + rc.TAIL, case.r
    doff = list(case.doff)
    doff[3] = case.dst_bytes + 100                   # begins past the extent
    doff[7] = case.dst_bytes - r * sizes[7] + 1      # its last row ends one byte past it
    doff[10] = 2**64 - 8                             # offset + rows wraps: 8 bytes before the base
    assert doff[3] + r * sizes[3] <= case.dst_bytes + 4096 and 8 < lead
    got, name = launch(case, "dev", doff=doff, out_lead=lead, tail=tail)  # raises unless FEC_OK
    assert name == "matapply_ragged<3,7>"
    want = np.full(got.shape, rc.GUARD, dtype=np.uint8)
    want[lead:lead + case.dst_bytes] = case.want[rc.OUT_OFF:rc.OUT_OFF + case.dst_bytes]
    for s in (3, 7, 10):
        for a, b in case.row_spans(s):
            want[a - rc.OUT_OFF + lead:b - rc.OUT_OFF + lead] = rc.GUARD
    bad = np.flatnonzero(got != want)
    assert not bad.size, ("first wrong bytes (offsets from the base)", (bad[:8] - lead).tolist())


# ---- offsets past 2 GiB and 4 GiB ---------------------------------------------------------------------

@pytest.mark.parametrize("desc", ["host", "dev"])
def test_far_offsets(desc):
    """Five stripes placed so that, from the base, one straddles 2^31, one
    2^32 and one begins past 2^32, on both sides; judged by far_arena's rule
    (the gathered rows are exact, and the arena holds no other byte than its
    fill), so that a truncated offset lands on background inside the arena."""
    k, m, r = 3, 10, 7
    sizes = [3001, 1, 4097, 0, 2500]
    offs = [2**31 - 1000, 2**31 + 2**20 + 7, 2**32 - 2000, 12345, 2**32 + 2**28 + 3]
    for o, edge in ((offs[0], 2**31), (offs[2], 2**32)):
        assert o < edge < o + min(sizes[0], sizes[2])  # block 0 / row 0 straddles it
    case = rc.Case(k, m, "enc", sizes, seed=31)
    code = capi.Code(k, m)
    src = far_arena.Arena(torch, far_arena.BACKGROUND, far_arena.SRC_ODD)
    dst = far_arena.Arena(torch, far_arena.GUARD, far_arena.DST_ODD)
    lays = []
    for s, sz in enumerate(sizes):
        if not sz:
            continue
        a = rc.IN_OFF + case.soff[s]
        blocks = case.src[a:a + k * sz].reshape(1, k, sz)
        src.place(far_arena.Layout("far_pair", k, sz, 1, offs[s], (sz, 0)), blocks)
        b = rc.OUT_OFF + case.doff[s]
        lays.append((far_arena.Layout("far_pair", r, sz, 1, offs[s], (sz, 0)),
                     case.want[b:b + r * sz].reshape(1, r, sz)))
    keep = [words(sizes, desc), words(offs, desc)]
    code.encode_batch_ragged(src.base, far_arena.SPAN, 0, keep[1][1], dst.base, far_arena.SPAN, 0, keep[1][1],
                             keep[0][1], case.nums, len(sizes), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = np.concatenate([dst.gather(lay).reshape(-1) for lay, _ in lays]).reshape(1, 1, -1)
    want = np.concatenate([w.reshape(-1) for _, w in lays]).reshape(1, 1, -1)
    far_arena.judge(got, want, dst.count_not(far_arena.GUARD), far_arena.GUARD, ("far offsets", desc))


# ---- wider codes: runs of shared-matrix launches -------------------------------------------------------

@pytest.mark.parametrize("desc", ["host", "dev"])
@pytest.mark.parametrize("op", ["enc", "dec"])
def test_wide_code_runs(op, desc):
    sizes = [4096] * 5 + [2048] * 3 + [0] + [5000]
    kw = dict(op="enc") if op == "enc" else dict(op="dec", nums=[0, 11, 2, 3, 15, 5, 6, 7, 12, 9])
    case = rc.Case(10, 16, sizes=sizes, seed=16, **kw)
    got, name = launch(case, desc)
    assert name and not name.startswith("matapply_ragged"), name
    check(case, got, (op, desc))


# ---- the Python surface ------------------------------------------------------------------------------------

def test_python_surface():
    k, m = 3, 10
    enc, dec = zfec_amd.Encoder(k, m), zfec_amd.Decoder(k, m)
    sizes = [int(x) for x in np.random.default_rng(3).integers(0, 2500, size=24)]
    start = np.cumsum([0] + sizes)
    total = int(start[-1])
    host = np.random.default_rng(4).integers(0, 256, size=k * total, dtype=np.uint8)
    data = torch.from_numpy(host).cuda()
    out, ooff = enc.encode_ragged(data, sizes)                       # sizes as a CPU list
    assert out.numel() == (m - k) * total and ooff.tolist() == [(m - k) * int(x) for x in start[:-1]]
    dsizes = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    given = torch.full(((m - k) * total,), rc.GUARD, dtype=torch.uint8, device="cuda")
    out2, ooff2 = enc.encode_ragged(data, dsizes, out=given)         # sizes as a device tensor, out given
    assert out2 is given and ooff2.is_cuda and ooff2.tolist() == ooff.tolist()
    assert torch.equal(out, out2)
    # slots [0, 5, 9]: primary 0, then blocks 5 and 9 of every stripe
    par = out.cpu().numpy()
    recv = np.empty(k * total, dtype=np.uint8)
    for s, sz in enumerate(sizes):
        a, p = k * int(start[s]), (m - k) * int(start[s])
        recv[a:a + sz] = host[a:a + sz]
        recv[a + sz:a + 2 * sz] = par[p + (5 - k) * sz:p + (5 - k + 1) * sz]
        recv[a + 2 * sz:a + 3 * sz] = par[p + (9 - k) * sz:p + (9 - k + 1) * sz]
    back, boff = dec.decode_ragged(torch.from_numpy(recv).cuda(), dsizes, [0, 5, 9])
    back = back.cpu().numpy()
    assert boff.tolist() == [2 * int(x) for x in start[:-1]]
    for s, sz in enumerate(sizes):
        a, b = k * int(start[s]), 2 * int(start[s])
        assert (back[b:b + 2 * sz] == host[a + sz:a + 3 * sz]).all(), ("stripe", s)
