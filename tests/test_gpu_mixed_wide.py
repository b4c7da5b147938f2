"""GPU parity of the pattern-per-stripe calls on wide codes (4 < k <= 32):
fec_decode_batch_mixed and fec_repair_batch as ONE launch of the mix form of
the run-time-data bit-sliced kernels (zfec_amd/csrc/kernels.hip
matapply_bsr<RT,mix>, matapply_bsr<RT,lds,mix>).  Expected bytes come from the
CPU oracle alone: all m blocks of random data are encoded, a decode must return
the data and a repair block targets[i].  Buffers, guards (0xA5; inputs at offset
3, outputs at offset 5) and pattern builders are test_gpu_mixed's and
test_gpu_repair's."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import far_arena
import test_gpu_mixed as mixed
import test_gpu_repair as repair
from test_gpu_mixed import WIDE_IDS, random_patterns, received, stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NONE = capi.FEC_REPAIR_NONE
SZS = (2048, 2049, 4096 + 17)  # one unit, a shifted overlapping last unit, three units
SZMAX = 3 * 2048 + 5


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def mix_name(r):
    """The kernel a pattern-per-stripe call of r rows takes: one wave for r <=
    10, two for r <= 20, four for r <= 32, tiles of ceil(r / waves) rows."""
    nw = 1 if r <= 10 else 2 if r <= 20 else 4
    return "matapply_bsr<%d%s,mix>" % (-(-r // nw), "" if nw == 1 else ",lds")


def assert_mix(name, r, what=""):
    assert name.startswith("matapply_bsr<") and name.endswith(",mix>"), (name, what)
    assert name == mix_name(r), (name, what)


def code_for(k):
    return k, min(256, k + max(k, 4))


def decode(code, k, m, ns, sz, pats, ids, kind="padded", where="host", r=None, **kw):
    """test_gpu_mixed.check (the data back, the guards intact) on the fused kernel."""
    host = mixed.check(code, k, m, ns, sz, pats, ids, kind, where, name=False, szmax=SZMAX, **kw)
    assert_mix(capi.last_kernel_name(), k if r is None else r, (k, m, ns, sz, kind, where))
    return host


# ---- decode forms -------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 7, 10, 11, 16, 20, 21, 25, 32])
def test_decode_forms(k):
    """Solo RT 5, 7, 10; two waves with RT 6, 8, 10 (k = 11, 16, 20); four with
    RT 6, 7, 8 (k = 21, 25, 32); k odd and no multiple of the phase (2 or 4
    inputs).  Runs of ids and 12 distinct ones, every layout, ids on either
    side with the same bytes."""
    k, m = code_for(k)
    ns = 12
    code = capi.Code(k, m)
    rng = np.random.default_rng(k)
    pats3, pats12 = random_patterns(rng, k, m, 3), random_patterns(rng, k, m, ns)
    assert m - k >= k and all(b >= k for b in pats3[1])  # an all-parity pattern
    for sz in SZS:
        for kind in ("packed", "padded", "bm"):
            for pats, ids in ((pats3, WIDE_IDS), (pats12, np.arange(ns))):
                a = decode(code, k, m, ns, sz, pats, ids, kind, "host")
                b = decode(code, k, m, ns, sz, pats, ids, kind, "device")
                assert (a == b).all(), (k, sz, kind)


# ---- repair forms -------------------------------------------------------------------------

def repair_patterns(rng, k, m, t):
    """test_gpu_repair.sweep_patterns' nine (parity, primaries, a present
    target, a duplicate, NONE first / middle / last, all NONE, a random draw),
    then one pattern per row position with NONE there."""
    pres, tgts = repair.sweep_patterns(rng, k, m, t, 9)
    for i in range(t):
        pr = rng.permutation(m)[:k].tolist()
        tg = [int(b) for b in rng.integers(0, m, size=t)]
        tg[i] = NONE
        pres.append(pr)
        tgts.append(tg)
    assert [NONE] * t in tgts
    assert all(any(tg[i] == NONE for tg in tgts) for i in range(t))
    return pres, tgts


def repair_forms(k, m, t, ns):
    code = capi.Code(k, m)
    pres, tgts = repair_patterns(np.random.default_rng(100 * k + t), k, m, t)
    assert len(pres) <= ns
    ids = np.arange(ns) % len(pres)
    for sz, kind, where in ((2049, "padded", "host"), (4096 + 17, "bm", "device"), (2048, "packed", "device")):
        repair.check(code, k, m, ns, sz, pres, tgts, ids, kind, where, name=mix_name(t), szmax=SZMAX)


@pytest.mark.parametrize("t", range(1, 11))
def test_repair_solo_forms(t):
    """(5, 40), 1..10 targets: every one-wave RT."""
    repair_forms(5, 40, t, 22)


@pytest.mark.parametrize("t", [11, 12, 16, 17, 20, 21, 24, 25, 32])
def test_repair_lds_forms(t):
    """(20, 60): RT 6-10 on two waves (t = 11..20) and RT 6-8 on four."""
    repair_forms(20, 60, t, 44)


def test_repair_all_none_launches_nothing():
    """Every target of every pattern FEC_REPAIR_NONE: no launch, nothing written."""
    k, m, ns, sz, t = 5, 9, 12, 2049, 3
    code = capi.Code(k, m)
    pres = random_patterns(np.random.default_rng(1), k, m, 3)
    mixed.check(code, k, m, ns, 64, pres, WIDE_IDS, name=False, szmax=SZMAX)  # another kernel's name
    before = capi.last_kernel_name()
    repair.check(code, k, m, ns, sz, pres, [[NONE] * t] * 3, WIDE_IDS, szmax=SZMAX)
    assert capi.last_kernel_name() == before


# ---- the grid-stride walk -----------------------------------------------------------------

@pytest.mark.parametrize("k", [6, 12])
@pytest.mark.parametrize("cap", [3, 7])
def test_grid_stride_carry(knobs, cap, k):
    """3 or 7 workgroups walk 23 stripes of 4 units: the step is 0 stripes and 3
    units, or 1 stripe and 3 units, so the carry runs; with 23 distinct
    patterns a wrong stripe after it decodes with the wrong matrix."""
    knobs(ZFEC_HIP_GRID_CAP=cap)
    k, m = code_for(k)
    ns, sz = 23, 3 * 2048 + 5
    pats = random_patterns(np.random.default_rng(cap * k), k, m, ns)
    for where in ("host", "device"):
        decode(capi.Code(k, m), k, m, ns, sz, pats, np.arange(ns), "padded", where)


# ---- ids that name no pattern -------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 12])
def test_device_id_out_of_range_leaves_the_stripe(k):
    k, m = code_for(k)
    sz = 2049
    code = capi.Code(k, m)
    pats = random_patterns(np.random.default_rng(k), k, m, 2)
    data, allb = stripes(k, m, 3, SZMAX)
    case = mixed.Case(received(allb, pats, [0, 1, 1], sz))
    assert_mix(case.launch(code, pats, np.array([0, 9, 1], dtype=np.uint32), "device"), k)
    got, _ = case.result()
    assert (got[0] == data[0, :, :sz]).all() and (got[2] == data[2, :, :sz]).all()
    assert (got[1] == mixed.GUARD).all()


# ---- against the run path -----------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 20])
def test_same_bytes_as_the_run_path(knobs, k):
    """ZFEC_HIP_MIXED_FUSED=0 selects the runs of shared-pattern launches: the
    same bytes, another kernel."""
    k, m = code_for(k)
    ns, sz = 12, 4096 + 17
    code = capi.Code(k, m)
    rng = np.random.default_rng(k)
    pats = random_patterns(rng, k, m, 3)
    pres, tgts = repair_patterns(rng, k, m, 4)
    rids = np.arange(ns) % len(pres)
    fused_d = decode(code, k, m, ns, sz, pats, WIDE_IDS, "padded", "device")
    fused_r = repair.check(code, k, m, ns, sz, pres, tgts, rids, "bm", "host", name=mix_name(4), szmax=SZMAX)
    knobs(ZFEC_HIP_MIXED_FUSED=0)
    runs_d = mixed.check(code, k, m, ns, sz, pats, WIDE_IDS, "padded", "device", name=False, szmax=SZMAX)
    assert not capi.last_kernel_name().endswith(",mix>")
    runs_r = repair.check(code, k, m, ns, sz, pres, tgts, rids, "bm", "host", szmax=SZMAX)
    assert not capi.last_kernel_name().endswith(",mix>")
    assert (fused_d == runs_d).all() and (fused_r == runs_r).all()


# ---- shapes that keep the run path --------------------------------------------------------

def test_short_blocks_take_the_run_path():
    k, m, ns = 5, 9, 12
    pats = random_patterns(np.random.default_rng(2), k, m, 3)
    mixed.check(capi.Code(k, m), k, m, ns, 2047, pats, WIDE_IDS, name=False, szmax=SZMAX)
    assert not capi.last_kernel_name().endswith(",mix>")


def test_codes_past_32_take_the_run_path():
    k, m, ns = 40, 60, 12
    pats = [np.random.default_rng(i).permutation(m)[:k].tolist() for i in range(3)]
    for where in ("host", "device"):
        mixed.check(capi.Code(k, m), k, m, ns, 2049, pats, WIDE_IDS, "padded", where, name=False, szmax=2049)
        assert not capi.last_kernel_name().endswith(",mix>")


def test_page_locked_host_blocks_take_the_run_path():
    k, m, ns, sz = 5, 9, 12, 2049
    data, allb = stripes(k, m, ns, SZMAX)
    pats = random_patterns(np.random.default_rng(3), k, m, 3)
    case = mixed.Case(received(allb, pats, WIDE_IDS, sz), device_mem=False)
    assert not case.launch(capi.Code(k, m), pats, WIDE_IDS, flags=0).endswith(",mix>")
    assert (case.result()[0] == data[:, :, :sz]).all()
    pres, tgts = repair_patterns(np.random.default_rng(4), k, m, 2)
    ids = np.arange(ns) % len(pres)
    rcase = repair.Case(received(allb, pres, ids, sz), 2, device_mem=False)
    assert not rcase.launch(capi.Code(k, m), pres, tgts, ids, flags=0).endswith(",mix>")
    assert (rcase.result()[0] == repair.expected(allb, tgts, ids, sz)).all()


# ---- host-visible behaviour ---------------------------------------------------------------

def test_two_streams():
    """Asynchronous calls back to back on two streams of one thread, each with
    its own records in the shared staging ring, more calls than it has slots."""
    k, m, ns, sz = 12, 24, 12, 2049
    code = capi.Code(k, m)
    data, allb = stripes(k, m, ns, SZMAX)
    rng = np.random.default_rng(5)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cases = []
    for i in range(6):
        pats = random_patterns(rng, k, m, 5 + i)
        ids = rng.integers(0, len(pats), size=ns)
        cases.append((mixed.Case(received(allb, pats, ids, sz)), pats, ids))
    pres, tgts = repair_patterns(rng, k, m, 3)
    rids = rng.integers(0, len(pres), size=ns)
    rcase = repair.Case(received(allb, pres, rids, sz), 3)
    torch.cuda.synchronize()
    for i, (case, pats, ids) in enumerate(cases):
        assert_mix(case.launch(code, pats, ids, "host" if i % 3 else "device", stream=streams[i % 2].cuda_stream), k)
    assert_mix(rcase.launch(code, pres, tgts, rids, stream=streams[0].cuda_stream), 3)
    for i, (case, _, _) in enumerate(cases):
        assert (case.result(i)[0] == data[:, :, :sz]).all(), i
    assert (rcase.result()[0] == repair.expected(allb, tgts, rids, sz)).all()


def test_unplanned_calls_decline_under_graph_capture():
    k, m, ns, sz = 12, 24, 12, 2049
    code = capi.Code(k, m)
    data, allb = stripes(k, m, ns, SZMAX)
    pats = random_patterns(np.random.default_rng(6), k, m, 3)
    case = mixed.Case(received(allb, pats, WIDE_IDS, sz))
    rcase = repair.Case(received(allb, pats, WIDE_IDS, sz), 2)
    tgts = [[0, NONE], [1, 2], [3, 0]]
    assert_mix(case.launch(code, pats, WIDE_IDS, "device"), k)  # outside the capture: works (and the probe has run)
    assert (case.result()[0] == data[:, :, :sz]).all()
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                case.launch(code, pats, WIDE_IDS)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                rcase.launch(code, pats, tgts, WIDE_IDS)
    torch.cuda.synchronize()


# ---- far offsets --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def arenas():
    src = far_arena.Arena(torch, far_arena.BACKGROUND, far_arena.SRC_ODD)
    dst = far_arena.Arena(torch, far_arena.GUARD, far_arena.DST_ODD)
    torch.cuda.synchronize()
    yield src, dst
    del src.t, dst.t
    del src, dst
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [5, 12])
def test_far_offsets(arenas, k):
    """70 stripes just under 64 MiB apart (far_arena.far_stripes): stripes 33..
    begin past 2^31 bytes from the base, 65.. past 2^32, each with its own
    pattern.  The rows must lie where 64-bit offsets put them and nowhere else
    (far_arena.judge), and the source arena must come back unchanged."""
    src, dst = arenas
    k, m = code_for(k)
    sz, ns = 8192 + 67, far_arena.NS
    lay = far_arena.Layout("far_stripes", k, sz)
    data, allb = stripes(k, m, ns, sz, seed=far_arena.SEED)
    pats = random_patterns(np.random.default_rng(far_arena.SEED + k), k, m, ns)
    ids = np.arange(ns, dtype=np.uint32)
    keep = torch.from_numpy(ids.view(np.int32)).cuda()
    src.place(lay, received(allb, pats, ids, sz))
    before = src.total()
    try:
        capi.Code(k, m).decode_batch_mixed(src.base, lay.bs, lay.ss, dst.base, lay.bs, lay.ss, pats, keep.data_ptr(),
                                           sz, ns, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = capi.last_kernel_name()
        dst.check(lay, np.asarray(data), (k, name))
        far_arena.judge_source(before, src.total(), k)
    finally:
        src.clear(lay)
    assert_mix(name, k)
