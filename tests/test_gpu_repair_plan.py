"""GPU parity of the pattern plans (fec_repair_plan_new, fec_repair_batch_planned,
Decoder.repair_plan / decode_plan): a planned call gives the bytes of the
unplanned one and of the CPU oracle, one plan serves many calls, and with ids
in device memory the call can be captured into a graph.  Buffers, guards and
pattern builders are test_gpu_mixed's and test_gpu_repair's."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

import test_gpu_repair as repair
from test_gpu_mixed import GUARD, IN_OFF, OUT_OFF, received, stripes
from test_gpu_mixed_wide import mix_name

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NONE = capi.FEC_REPAIR_NONE
SZ = 2049  # a shifted, overlapping last unit on the wide kernels


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def kernel_of(k, t):
    return "matrepair_mixed<%d,%d>" % (k, (t - 1) % 8 + 1) if k <= 4 else mix_name(t)


def patterns_for(k, m, t, what):
    """(present, targets) of 12 patterns.  A decode plan's targets are 0..k-1
    for every pattern; a repair's (t may exceed m - k) are, in order: the
    absent blocks, then present ones; random primaries; NONE first; NONE last;
    all NONE; then random draws from all m numbers with NONE mixed in."""
    rng = np.random.default_rng(1000 * k + t)
    pres = repair.random_present(rng, k, m, 12)
    if what == "decode":
        return pres, [list(range(k))] * len(pres)
    tgts = []
    for p, pr in enumerate(pres):
        tg = [NONE if rng.random() < 0.2 else int(b) for b in rng.integers(0, m, size=t)]
        if p == 0:
            tg = [int(b) for b in (repair.absent(pr, m) + pr * t)[:t]]
        elif p == 1:
            tg = rng.integers(0, k, size=t).tolist()
        elif p == 2:
            tg[0] = NONE
        elif p == 3:
            tg[t - 1] = NONE
        elif p == 4:
            tg = [NONE] * t
        tgts.append(tg)
    return pres, tgts


def device_ids(ids):
    return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda()


def planned(plan, case, ids, where="host", stream=None, flags=capi.FEC_FLAG_ASYNC):
    """test_gpu_repair.Case.launch through the plan; ids: an array, or with
    where == "device" also a tensor already on the device."""
    if where == "device":
        case.keep = ids if hasattr(ids, "data_ptr") else device_ids(ids)
        ptr = case.keep.data_ptr()
    else:
        case.keep = ids = np.ascontiguousarray(ids, dtype=np.uint32)
        ptr = ids.ctypes.data
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    plan.repair_batch(case.src.data_ptr() + IN_OFF, case.lin.bs, case.lin.ss, case.dst.data_ptr() + OUT_OFF,
                      case.lout.bs, case.lout.ss, ptr, case.sz, case.ns, stream=st, flags=flags)
    return capi.last_kernel_name()


SHAPES = [(3, 10, "decode", 3), (3, 10, "repair", 3), (3, 10, "repair", 11), (4, 12, "decode", 4),
          (4, 12, "repair", 3), (4, 12, "repair", 11), (5, 9, "decode", 5), (5, 9, "repair", 3),
          (20, 60, "decode", 20), (20, 60, "repair", 3), (20, 60, "repair", 11)]


@pytest.mark.parametrize("k,m,what,t", SHAPES, ids=["%d_%d-%s-%d" % s for s in SHAPES])
def test_planned_equals_unplanned(k, m, what, t):
    """Byte for byte the unplanned call's output and the oracle's, ids on either
    side; (3, 10) and (4, 12) with 11 targets run as launches of 8 and 3 rows."""
    ns, sz = 37, SZ
    code = capi.Code(k, m)
    pres, tgts = patterns_for(k, m, t, what)
    ids = np.arange(ns) % len(pres)
    data, allb = stripes(k, m, ns, SZ)
    want = repair.expected(allb, tgts, ids, sz)
    plan = code.repair_plan(pres, tgts)
    try:
        for where in ("host", "device"):
            for kind in ("padded", "bm"):
                unplanned = repair.check(code, k, m, ns, sz, pres, tgts, ids, kind, where, name=kernel_of(k, t),
                                         szmax=SZ)
                case = repair.Case(received(allb, pres, ids, sz), t, kind)
                assert planned(plan, case, ids, where) == kernel_of(k, t)
                got, host = case.result((k, m, what, t, kind, where))
                assert (got == want).all()
                assert (host == unplanned).all()
    finally:
        plan.close()


def test_kernel_names():
    plan = capi.Code(3, 10).repair_plan([[7, 8, 9]], [[0, 1, 2]])
    data, allb = stripes(3, 10, 4, 64)
    case = repair.Case(received(allb, [[7, 8, 9]], [0] * 4, 64), 3)
    assert planned(plan, case, [0] * 4) == "matrepair_mixed<3,3>"
    assert (case.result()[0] == data).all()
    plan.close()
    for k, m in ((5, 9), (20, 60)):
        assert kernel_of(k, k).endswith(",mix>") and kernel_of(k, 3) == "matapply_bsr<3,mix>"


@pytest.mark.parametrize("k,m", [(3, 10), (20, 60)])
def test_one_plan_many_calls(k, m):
    """One plan, three calls over different buffers and sizes."""
    code = capi.Code(k, m)
    pres, tgts = patterns_for(k, m, 3, "repair")
    plan = code.repair_plan(pres, tgts)
    rng = np.random.default_rng(k)
    try:
        for sz, ns in ((2048, 300), (5000, 12), (1 << 16, 1)):
            data, allb = stripes(k, m, ns, sz, seed=3)
            ids = rng.integers(0, len(pres), size=ns)
            case = repair.Case(received(allb, pres, ids, sz), 3, "packed")
            assert planned(plan, case, ids, "device") == kernel_of(k, 3)
            assert (case.result((k, sz, ns))[0] == repair.expected(allb, tgts, ids, sz)).all()
    finally:
        plan.close()


# ---- graph capture ------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (20, 60)])
def test_graph_capture_with_device_ids(k, m):
    """The planned call with ids in device memory stages nothing: captured on a
    side stream, replayed twice with the input rewritten in between."""
    ns, sz, t = 16, 4096, 3
    code = capi.Code(k, m)
    pres, tgts = patterns_for(k, m, t, "repair")
    ids = np.arange(ns) % len(pres)
    plan = code.repair_plan(pres, tgts)  # the routine-table probe runs here
    data_a, allb_a = stripes(k, m, ns, sz, seed=5)
    data_b, allb_b = stripes(k, m, ns, sz, seed=6)
    case = repair.Case(received(allb_a, pres, ids, sz), t)
    other = repair.Case(received(allb_b, pres, ids, sz), t)
    on_device = device_ids(ids)  # made before the capture: nothing but the kernel is recorded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            name = planned(plan, case, on_device, "device", stream=s.cuda_stream)
    assert name == kernel_of(k, t)
    torch.cuda.synchronize()
    assert (case.result("captured, not run")[0] == GUARD).all()
    g.replay()
    assert (case.result("first replay")[0] == repair.expected(allb_a, tgts, ids, sz)).all()
    case.src.copy_(other.src)
    case.dst.fill_(GUARD)
    g.replay()
    assert (case.result("second replay")[0] == repair.expected(allb_b, tgts, ids, sz)).all()
    del g
    plan.close()


def test_host_ids_decline_under_capture():
    k, m, ns, sz, t = 20, 60, 16, 4096, 3
    code = capi.Code(k, m)
    pres, tgts = patterns_for(k, m, t, "repair")
    ids = np.arange(ns) % len(pres)
    plan = code.repair_plan(pres, tgts)
    data, allb = stripes(k, m, ns, sz, seed=5)
    case = repair.Case(received(allb, pres, ids, sz), t)
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                planned(plan, case, ids, "host", stream=s.cuda_stream)
    torch.cuda.synchronize()
    plan.close()


def test_wrong_device():
    if zfec_amd.device_count() < 2:
        pytest.skip("needs a second device")
    k, m, ns, sz = 3, 10, 4, 64
    plan = capi.Code(k, m).repair_plan([[7, 8, 9]], [[0]], device=1)
    src = torch.zeros(ns * k * sz, dtype=torch.uint8, device="cuda:0")
    dst = torch.zeros(ns * sz, dtype=torch.uint8, device="cuda:0")
    ids = np.zeros(ns, dtype=np.uint32)
    with pytest.raises(capi.FecError, match="status %d: .*the plan lives on device 1" % capi.FEC_EINVAL):
        plan.repair_batch(src.data_ptr(), sz, k * sz, dst.data_ptr(), sz, sz, ids.ctypes.data, sz, ns)
    plan.close()


# ---- the Python surface -------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (12, 24)])
def test_python_surface(k, m):
    ns, sz = 37, SZ
    dec = zfec_amd.Decoder(k, m)
    data, allb = stripes(k, m, ns, SZ)
    rng = np.random.default_rng(k)
    pats = repair.random_present(rng, k, m, 7)
    ids = rng.integers(0, 7, size=ns)
    blocks = torch.from_numpy(received(allb, pats, ids, sz)).cuda()
    plan = dec.decode_plan(pats)
    assert plan.npatterns == 7 and plan.patterns.tolist() == pats
    assert plan.targets.tolist() == [list(range(k))] * 7
    forms = {"list": ids.tolist(), "numpy": ids, "numpy uint32": ids.astype(np.uint32),
             "host tensor": torch.from_numpy(ids), "device tensor": torch.from_numpy(ids).cuda(),
             "device int32": torch.from_numpy(ids).cuda().to(torch.int32)}
    for what, form in forms.items():
        out = plan.decode_batch(blocks, form)
        assert capi.last_kernel_name() == kernel_of(k, k), what
        assert tuple(out.shape) == (ns, k, sz) and out.is_contiguous(), what
        assert (out.cpu().numpy() == data[:, :, :sz]).all(), what
    # the same bytes as the unplanned call
    assert (dec.decode_batch_mixed(blocks, (pats, ids.tolist())).cpu().numpy() == data[:, :, :sz]).all()
    # block-major in, block-major out
    bm = blocks.transpose(0, 1).contiguous().transpose(0, 1)
    out = plan.decode_batch(bm, ids)
    assert out.stride(0) < out.stride(1) and (out.cpu().numpy() == data[:, :, :sz]).all()
    plan.close()
    plan.close()
    with pytest.raises(zfec_amd.Error, match="the repair plan is closed"):
        plan.decode_batch(blocks, ids)
    # a repair plan: out= keeps the rows of -1 targets
    tgts = [[int(b) for b in rng.permutation(m)[:2]] for _ in pats]
    tgts[1][0] = -1
    tgts[2] = [-1, -1]
    rplan = dec.repair_plan(np.asarray(pats), torch.tensor(tgts))
    out = torch.full((ns, 2, sz), GUARD, dtype=torch.uint8, device="cuda")
    assert rplan.repair_batch(blocks, torch.from_numpy(ids).cuda(), out=out) is out
    want = repair.expected(allb, [[NONE if b < 0 else b for b in tg] for tg in tgts], ids, sz)
    assert (out.cpu().numpy() == want).all()
    fresh = rplan.repair_batch(blocks, ids)
    live = want != GUARD
    assert tuple(fresh.shape) == (ns, 2, sz) and (fresh.cpu().numpy()[live] == want[live]).all()
    rplan.close()


def test_python_call_preconditions():
    """The checks of RepairPlan.repair_batch that precede any launch (a plan itself needs a GPU)."""
    dec = zfec_amd.Decoder(3, 10)
    plan = dec.repair_plan([[7, 8, 9], [0, 5, 2]], [[0, 1], [9, -1]])
    assert plan.npatterns == 2 and plan.patterns.tolist() == [[7, 8, 9], [0, 5, 2]]
    assert plan.targets.tolist() == [[0, 1], [9, -1]]
    ns, sz = 4, 16
    host = torch.zeros((ns, 3, sz), dtype=torch.uint8)
    with pytest.raises(zfec_amd.Error, match="device tensor .*not a host tensor"):
        plan.repair_batch(host, [0, 1, 1, 0])
    with pytest.raises(zfec_amd.Error, match="host \\(numpy\\) blocks are not staged"):
        plan.repair_batch(host.numpy(), [0, 1, 1, 0])
    with pytest.raises(zfec_amd.Error, match="required to hold 3 blocks per stripe, not 4"):
        plan.repair_batch(torch.zeros((ns, 4, sz), dtype=torch.uint8), [0, 1, 1, 0])
    with pytest.raises(zfec_amd.Error, match="pattern_of is required to hold nstripes = 4 ids, not 3"):
        plan.repair_batch(host, [0, 1, 1])
    with pytest.raises(zfec_amd.Error, match="pattern_of is required to be a 1-D integer array"):
        plan.repair_batch(host, [[0, 1, 1, 0]])
    with pytest.raises(zfec_amd.Error, match="pattern_of ids are required to be in \\[0, 1\\]"):
        plan.repair_batch(host, torch.tensor([0, 1, 2, 0]))
    with pytest.raises(zfec_amd.Error, match="out is required to be a uint8 tensor \\[nstripes, t, sz\\] = \\[4, 2, 16\\]"):
        plan.repair_batch(host, [0, 1, 1, 0], out=torch.zeros((ns, 3, sz), dtype=torch.uint8))
    with pytest.raises(zfec_amd.Error, match="decode_batch takes a plan made by Decoder.decode_plan"):
        plan.decode_batch(host, [0, 1, 1, 0])
    plan.close()
    plan.close()
    with pytest.raises(zfec_amd.Error, match="the repair plan is closed"):
        plan.repair_batch(host, [0, 1, 1, 0])


def test_decode_plan_past_32_raises():
    with pytest.raises(zfec_amd.Error, match="decode_plan takes codes of k <= 32"):
        zfec_amd.Decoder(40, 60).decode_plan([list(range(40))])
