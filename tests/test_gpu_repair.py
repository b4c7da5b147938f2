"""GPU parity of the batched repair (fec_repair_batch; zfec_amd/csrc/kernels.hip
matrepair_mixed<K, R> for k <= 4, runs of the shared-matrix path past that and
for pattern_of = NULL).  Shares come from the CPU oracle's encode
(zfec/fec.c:487-505), so the expected output needs no matrix algebra: row i of
stripe s is block targets[..][i] of that stripe.  Outputs are pre-filled with
0xA5; the rows of FEC_REPAIR_NONE targets and the bytes before, between and
after the rows must come back unchanged.  Inputs start at offset 3, outputs at
offset 5.  The buffer helpers are test_gpu_mixed's."""
import itertools

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi

from test_gpu_mixed import GUARD, IN_OFF, OUT_OFF, SIZES, TAIL, Layout, received, stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NONE = capi.FEC_REPAIR_NONE


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def expected(allb, tgts, ids, sz):
    """(ns, t, sz): row i of stripe s is block tgts[ids[s]][i] of it; the rows of
    NONE targets, and every row of a stripe whose id names no pattern, hold the guard."""
    ns, t = allb.shape[0], len(tgts[0])
    want = np.full((ns, t, sz), GUARD, dtype=np.uint8)
    for s in range(ns):
        if ids[s] < len(tgts):
            for i, b in enumerate(tgts[ids[s]]):
                if b != NONE:
                    want[s, i] = allb[s, b, :sz]
    return want


class Case(object):
    def __init__(self, recv, t, kind="padded", device_mem=True):
        self.ns, self.k, self.sz = recv.shape
        self.t = t
        self.lin = Layout(kind, self.ns, self.k, self.sz)
        self.lout = Layout(kind, self.ns, t, self.sz)
        src = np.zeros(IN_OFF + self.lin.nbytes + TAIL, dtype=np.uint8)
        self.lin.view(src[IN_OFF:IN_OFF + self.lin.nbytes])[:, :, :self.sz] = recv
        dst = np.full(OUT_OFF + self.lout.nbytes + TAIL, GUARD, dtype=np.uint8)
        if device_mem:
            self.src, self.dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        else:
            self.src, self.dst = torch.from_numpy(src).pin_memory(), torch.from_numpy(dst).pin_memory()
        self.keep = None

    def launch(self, code, pres, tgts, ids, where="host", stream=None, flags=capi.FEC_FLAG_ASYNC):
        """ids: uint32 numpy array; where: "host", "device" or "null" (pattern_of = NULL)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        if where == "device":
            self.keep = torch.from_numpy(ids.view(np.int32)).cuda()
            ptr = self.keep.data_ptr()
        elif where == "null":
            ptr = 0
        else:
            self.keep = ids
            ptr = ids.ctypes.data
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        code.repair_batch(self.src.data_ptr() + IN_OFF, self.lin.bs, self.lin.ss, self.dst.data_ptr() + OUT_OFF,
                          self.lout.bs, self.lout.ss, pres, tgts, ptr, self.sz, self.ns, stream=st, flags=flags)
        return capi.last_kernel_name()

    def result(self, what=""):
        """The output rows (ns, t, sz), the guards checked; and the whole buffer."""
        torch.cuda.synchronize()
        host = self.dst.cpu().numpy()
        n = self.lout.nbytes
        assert (host[:OUT_OFF] == GUARD).all(), ("write before the output", what)
        assert (host[OUT_OFF + n:] == GUARD).all(), ("write after the output", what)
        body = self.lout.view(host[OUT_OFF:OUT_OFF + n])
        assert (body[:, :, self.sz:] == GUARD).all(), ("write past a row", what)
        return body[:, :, :self.sz], host


def check(code, k, m, ns, sz, pres, tgts, ids, kind="padded", where="host", name=None, szmax=None, seed=0,
          recv_ids=None):
    """Launch and compare.  name: the kernel name expected (None: not asserted).
    recv_ids: the ids the received blocks are laid out by, where `ids` itself
    holds ids that name no pattern."""
    data, allb = stripes(k, m, ns, szmax or sz, seed)
    t = len(tgts[0])
    case = Case(received(allb, pres, ids if recv_ids is None else recv_ids, sz), t, kind)
    got_name = case.launch(code, pres, tgts, ids, where)
    what = (k, m, ns, sz, t, kind, where, got_name)
    got, host = case.result(what)
    if name is not None:
        assert got_name == name, what
    want = expected(allb, tgts, ids, sz)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (what, "first wrong (stripe, row):", bad[:4].tolist())
    return host


def random_present(rng, k, m, n):
    """n present sets, each a random k-subset in a random slot order; the first
    is the all-primaries shuffle, the second (where the code has k parity
    blocks) all parity."""
    pres = [rng.permutation(k).tolist()]
    if m - k >= k:
        pres.append((k + rng.permutation(m - k)[:k]).tolist())
    while len(pres) < n:
        pres.append(rng.permutation(m)[:k].tolist())
    return pres


def absent(pres, m):
    return [b for b in range(m) if b not in pres]


def sweep_patterns(rng, k, m, t, n):
    """n (present, targets) patterns with t targets each.  In order: all targets
    parity; all targets primaries; a target that is present; a duplicate target;
    NONE in the first, a middle and the last row; all NONE; then random draws
    from all m numbers with NONE mixed in."""
    pres = random_present(rng, k, m, n)
    tgts = []
    for p, pr in enumerate(pres):
        miss = rng.permutation(absent(pr, m))
        tg = [int(miss[i % len(miss)]) for i in range(t)]
        if p == 0:
            tg = (k + rng.permutation(m - k)[:t]).tolist()
        elif p == 1:
            tg = rng.integers(0, k, size=t).tolist()
        elif p == 2:
            tg[0] = pr[0]
        elif p == 3:
            tg[t - 1] = tg[0]
        elif p == 4:
            tg[0] = NONE
        elif p == 5:
            tg[t // 2] = NONE
        elif p == 6:
            tg[t - 1] = NONE
        elif p == 7:
            tg = [NONE] * t
        else:
            tg = [NONE if rng.random() < 0.2 else int(b) for b in rng.integers(0, m, size=t)]
        tgts.append(tg)
    return pres, tgts


@pytest.mark.parametrize("R", range(1, 9))
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sweep(K, R):
    """37 stripes, each with its own pattern, at the byte tail (1, 15, 17),
    exact chunks (16, 1024: exactly 64), a partly masked wave (1023, 1040: 65
    chunks, a second wave with one live lane) and four waves per stripe, in
    every layout."""
    m, ns = K + 8, 37
    assert m - K >= R  # all-parity targets exist
    code = capi.Code(K, m)
    pres, tgts = sweep_patterns(np.random.default_rng(10 * K + R), K, m, R, ns)
    assert [NONE] * R in tgts
    for kind in ("packed", "padded", "bm"):
        for sz in SIZES:
            check(code, K, m, ns, sz, pres, tgts, np.arange(ns), kind, name="matrepair_mixed<%d,%d>" % (K, R),
                  szmax=max(SIZES))


def test_all_120_subsets():
    """K=3/M=10: every present subset, once sorted and once shuffled, each with
    its 7 absent blocks as targets in random order."""
    k, m, sz = 3, 10, 1040
    rng = np.random.default_rng(120)
    subs = [list(c) for c in itertools.combinations(range(m), k)]
    assert len(subs) == 120
    pres = subs + [rng.permutation(c).tolist() for c in subs]
    tgts = [rng.permutation(absent(p, m)).tolist() for p in pres]
    check(capi.Code(k, m), k, m, 240, sz, pres, tgts, rng.permutation(240), name="matrepair_mixed<3,7>")


@pytest.mark.parametrize("sz", [1040, 4096])
def test_grid_stride(knobs, sz):
    """Two workgroups (8 waves) walk 37 stripes of 2 or 4 waves each.  A step
    of 8 waves is exactly 4 or 2 stripes here (gs_w = 0), so the carry of the
    walk never runs: test_gpu_wave_walk.py has the geometries with gs_w != 0."""
    knobs(ZFEC_HIP_GRID_CAP=2)
    k, m, ns = 3, 10, 37
    pres, tgts = sweep_patterns(np.random.default_rng(sz), k, m, 3, ns)
    check(capi.Code(k, m), k, m, ns, sz, pres, tgts, np.arange(ns), name="matrepair_mixed<3,3>", szmax=4096)


@pytest.mark.parametrize("sz,ns", [(4096, 37), (20000, 5)])
def test_split_launches(knobs, sz, ns):
    """ZFEC_HIP_LAUNCH_UNITS=1024: 4 KiB stripes go in groups of 4 (the id
    pointer advanced per group), 20000-byte blocks in byte ranges of 16 KiB."""
    knobs(ZFEC_HIP_LAUNCH_UNITS=1024)
    k, m = 3, 10
    pres, tgts = sweep_patterns(np.random.default_rng(sz), k, m, 4, max(ns, 9))
    ids = (np.arange(ns) * 5) % len(pres)
    check(capi.Code(k, m), k, m, ns, sz, pres, tgts, ids, name="matrepair_mixed<3,4>", seed=1)


def test_host_and_device_ids_identical():
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    rng = np.random.default_rng(7)
    pres, tgts = sweep_patterns(rng, k, m, 2, 9)
    ids = rng.integers(0, 9, size=ns)
    a = check(code, k, m, ns, sz, pres, tgts, ids, where="host", name="matrepair_mixed<3,2>", szmax=4096)
    b = check(code, k, m, ns, sz, pres, tgts, ids, where="device", name="matrepair_mixed<3,2>", szmax=4096)
    assert (a == b).all()


def test_device_id_out_of_range_leaves_the_stripe():
    """A device-side id >= npatterns reads no table: its stripe keeps the
    guard, its neighbours are repaired."""
    k, m, ns, sz = 3, 10, 37, 1040
    rng = np.random.default_rng(8)
    pres, tgts = sweep_patterns(rng, k, m, 3, 4)  # no NONE among these four
    good = rng.integers(0, 4, size=ns)
    ids = good.copy()
    ids[[0, 11, 12, 36]] = [4, 5, 0xFFFFFFFF, 1 << 20]
    check(capi.Code(k, m), k, m, ns, sz, pres, tgts, ids.astype(np.uint32), where="device",
          name="matrepair_mixed<3,3>", szmax=4096, recv_ids=good)


def test_more_than_eight_targets():
    """(3, 14) with t = 11 runs as launches of 8 and 3 rows over one upload.
    One pattern's last three targets are all NONE; when every pattern's are,
    the second launch is skipped."""
    k, m, ns, sz, t = 3, 14, 37, 1040, 11
    code = capi.Code(k, m)
    rng = np.random.default_rng(11)
    pres = random_present(rng, k, m, 9)
    tgts = [rng.permutation(absent(p, m)).tolist() for p in pres]
    assert all(len(tg) == t for tg in tgts)
    tgts[3][8:] = [NONE] * 3
    tgts[5][2] = NONE
    tgts[6][9] = NONE
    ids = rng.integers(0, 9, size=ns)
    ids[:9] = np.arange(9)
    check(code, k, m, ns, sz, pres, tgts, ids, name="matrepair_mixed<3,3>")
    check(code, k, m, ns, sz, pres, tgts, ids, "bm", "device", name="matrepair_mixed<3,3>")
    short = [tg[:8] + [NONE] * 3 for tg in tgts]
    check(code, k, m, ns, sz, pres, short, ids, name="matrepair_mixed<3,8>")


@pytest.mark.parametrize("kind", ["padded", "bm"])
@pytest.mark.parametrize("k,m,tg", [(3, 10, [8, 1]), (10, 16, [15, NONE, 4])])
def test_pattern_of_null(k, m, tg, kind):
    """pattern_of = NULL: one pattern for every stripe, through the
    shared-matrix path; the same bytes as the per-stripe call with all ids 0."""
    ns, sz = 37, 1040
    code = capi.Code(k, m)
    pres = [np.random.default_rng(k).permutation(m)[:k].tolist()]
    ids = np.zeros(ns, dtype=np.uint32)
    a = check(code, k, m, ns, sz, pres, [tg], ids, kind, "null")
    assert not capi.last_kernel_name().startswith("matrepair_mixed")
    b = check(code, k, m, ns, sz, pres, [tg], ids, kind, "host",
              name="matrepair_mixed<3,2>" if k <= 4 else None)
    assert (a == b).all()


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_pattern_of_null_dense_block_major(k, m):
    """Stripes packed back to back inside each block array (both stripe strides
    == sz): the shared-matrix path runs them as one long stripe.  The NONE
    row's whole array keeps the guard."""
    ns, sz = 37, 1040
    data, allb = stripes(k, m, ns, 4096)
    pres = np.random.default_rng(m).permutation(m)[:k].tolist()
    tg = [absent(pres, m)[0], NONE, pres[1], 0]
    src = torch.from_numpy(np.ascontiguousarray(allb[:, pres, :sz].transpose(1, 0, 2))).cuda()  # (k, ns, sz)
    dst = torch.full((len(tg), ns, sz), GUARD, dtype=torch.uint8, device="cuda")
    capi.Code(k, m).repair_batch(src.data_ptr(), ns * sz, sz, dst.data_ptr(), ns * sz, sz, [pres], [tg], 0, sz, ns,
                                 stream=torch.cuda.current_stream().cuda_stream)
    assert not capi.last_kernel_name().startswith("matrepair_mixed")
    torch.cuda.synchronize()
    got = dst.cpu().numpy().transpose(1, 0, 2)
    assert (got == expected(allb, [tg], np.zeros(ns, dtype=np.int64), sz)).all()


WIDE_IDS = [0, 0, 0, 1, 1, 2, 0, 0, 2, 2, 2, 1]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k,m", [(5, 9), (20, 60)])
def test_fallback_past_the_register_shapes(k, m, where):
    """k > 4: runs of consecutive stripes with one id, each one shared-matrix
    launch of that pattern's live rows."""
    ns, sz = 12, 2049
    rng = np.random.default_rng(k)
    pres = random_present(rng, k, m, 3)
    tgts = [rng.permutation(absent(p, m))[:4].tolist() for p in pres]
    tgts[0][1] = NONE
    tgts[1][0] = pres[1][2]
    tgts[2][3] = NONE
    tgts[2][2] = tgts[2][0]
    check(capi.Code(k, m), k, m, ns, sz, pres, tgts, WIDE_IDS, "padded", where)
    assert not capi.last_kernel_name().startswith("matrepair_mixed")
    pres.append(pres[0])
    tgts.append([NONE] * 4)  # an all-NONE pattern: its run launches nothing
    check(capi.Code(k, m), k, m, ns, sz, pres, tgts, [3 if i == 1 else i for i in WIDE_IDS], "bm", where)


def test_agrees_with_decode_then_encode():
    """The long way on one batch: fec_decode_batch_mixed, then fec_encode_batch
    of the 7 parity rows, gives the bytes fec_repair_batch gives for targets 0..9."""
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    rng = np.random.default_rng(12)
    pres = random_present(rng, k, m, 9)
    ids = rng.integers(0, 9, size=ns).astype(np.uint32)
    data, allb = stripes(k, m, ns, 4096)
    tgts = [list(range(m))] * 9
    case = Case(received(allb, pres, ids, sz), m, "packed")
    assert case.launch(code, pres, tgts, ids) == "matrepair_mixed<3,2>"
    got, _ = case.result()
    st = torch.cuda.current_stream().cuda_stream
    prim = torch.empty((ns, k, sz), dtype=torch.uint8, device="cuda")
    par = torch.empty((ns, m - k, sz), dtype=torch.uint8, device="cuda")
    code.decode_batch_mixed(case.src.data_ptr() + IN_OFF, case.lin.bs, case.lin.ss, prim.data_ptr(), sz, k * sz, pres,
                            ids.ctypes.data, sz, ns, stream=st)
    code.encode_batch(prim.data_ptr(), sz, k * sz, par.data_ptr(), sz, (m - k) * sz, list(range(k, m)), sz, ns,
                      stream=st)
    torch.cuda.synchronize()
    long_way = torch.cat([prim, par], dim=1).cpu().numpy()
    assert (got == long_way).all() and (got == allb[:, :, :sz]).all()


def test_two_streams():
    """Asynchronous calls back to back on two streams, each with its own
    pattern table, more of them than the staging ring has slots."""
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    data, allb = stripes(k, m, ns, 4096)
    rng = np.random.default_rng(2)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cases = []
    for i in range(6):
        pres, tgts = sweep_patterns(rng, k, m, 3, 5 + i)
        ids = rng.integers(0, len(pres), size=ns)
        cases.append((Case(received(allb, pres, ids, sz), 3), pres, tgts, ids))
    torch.cuda.synchronize()
    for i, (case, pres, tgts, ids) in enumerate(cases):
        s = streams[i % 2]
        assert case.launch(code, pres, tgts, ids, "host" if i % 3 else "device", stream=s.cuda_stream) == \
            "matrepair_mixed<3,3>"
    for i, (case, pres, tgts, ids) in enumerate(cases):
        got, _ = case.result(i)
        assert (got == expected(allb, tgts, ids, sz)).all(), i


def test_page_locked_host_memory():
    """src and dst in page-locked host memory are read and written in place."""
    k, m, ns, sz = 3, 10, 37, 1040
    data, allb = stripes(k, m, ns, 4096)
    rng = np.random.default_rng(3)
    pres, tgts = sweep_patterns(rng, k, m, 2, 9)
    ids = rng.integers(0, 9, size=ns)
    case = Case(received(allb, pres, ids, sz), 2, device_mem=False)
    assert case.launch(capi.Code(k, m), pres, tgts, ids, flags=0) == "matrepair_mixed<3,2>"
    got, _ = case.result()
    assert (got == expected(allb, tgts, ids, sz)).all()


@pytest.mark.parametrize("which", ["src", "dst"])
def test_pageable_host_memory_is_refused(which):
    """The call does not stage: a pageable src or dst is FEC_EINVAL, the other
    side in device memory, and nothing is written."""
    k, m, ns, sz = 3, 10, 4, 64
    dev_src = torch.zeros(ns * k * sz, dtype=torch.uint8, device="cuda")
    dev_dst = torch.full((ns * 2 * sz,), GUARD, dtype=torch.uint8, device="cuda")
    host = np.full(ns * k * sz, GUARD, dtype=np.uint8)
    ids = np.zeros(ns, dtype=np.uint32)
    src = host.ctypes.data if which == "src" else dev_src.data_ptr()
    dst = host.ctypes.data if which == "dst" else dev_dst.data_ptr()
    with pytest.raises(capi.FecError, match="status %d: .*%s is pageable host memory" % (capi.FEC_EINVAL, which)):
        capi.Code(k, m).repair_batch(src, sz, k * sz, dst, sz, 2 * sz, [[7, 8, 9]], [[0, 1]], ids.ctypes.data, sz, ns,
                                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (host == GUARD).all() and (dev_dst.cpu().numpy() == GUARD).all()


def test_declines_under_graph_capture():
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    data, allb = stripes(k, m, ns, 4096)
    pres, tgts, ids = [[7, 8, 9], [2, 0, 5]], [[0, NONE], [9, 1]], np.arange(ns) % 2
    case = Case(received(allb, pres, ids, sz), 2)
    case.launch(code, pres, tgts, ids)  # outside the capture: works
    assert (case.result()[0] == expected(allb, tgts, ids, sz)).all()
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                case.launch(code, pres, tgts, ids)
    torch.cuda.synchronize()


def test_python_api():
    k, m, ns, sz, t = 3, 10, 37, 1040, 3
    dec = zfec_amd.Decoder(k, m)
    data, allb = stripes(k, m, ns, 4096)
    rng = np.random.default_rng(4)
    pres, tgts = sweep_patterns(rng, k, m, t, 11)
    ids = rng.integers(0, 11, size=ns)
    ids[:11] = np.arange(11)
    nums = np.asarray(pres)[ids]  # (ns, k)
    tg = np.asarray(tgts, dtype=np.int64)
    tg[tg == NONE] = -1
    per_stripe = tg[ids]  # (ns, t)
    blocks = torch.from_numpy(received(allb, pres, ids, sz)).cuda()
    want = expected(allb, tgts, ids, sz)
    live = (per_stripe >= 0)
    assert not live.all() and live.any()
    forms = {
        "lists": (nums.tolist(), per_stripe.tolist()),
        "numpy": (nums, per_stripe),
        "host tensor": (torch.from_numpy(nums), torch.from_numpy(per_stripe)),
        "device tensor": (torch.from_numpy(nums).cuda(), torch.from_numpy(per_stripe).cuda()),
        "device nums, host targets": (torch.from_numpy(nums).cuda(), per_stripe),
        "pair": ((pres, ids.tolist()), tg.tolist()),
        "pair, device ids": ((np.asarray(pres), torch.from_numpy(ids).cuda()), torch.from_numpy(tg)),
    }
    for what, (bn, targets) in forms.items():
        out = dec.repair_batch(blocks, bn, targets)
        assert capi.last_kernel_name() == "matrepair_mixed<3,3>", what
        assert tuple(out.shape) == (ns, t, sz) and out.is_contiguous(), what
        assert (out.cpu().numpy()[live] == want[live]).all(), what
        # out=: the rows of -1 targets keep their contents
        mine = torch.full((ns, t, sz), GUARD, dtype=torch.uint8, device="cuda")
        assert dec.repair_batch(blocks, bn, targets, out=mine) is mine
        assert (mine.cpu().numpy() == want).all(), what
    # block-major input gives block-major output
    bm = blocks.transpose(0, 1).contiguous().transpose(0, 1)
    out = dec.repair_batch(bm, nums, per_stripe)
    assert out.stride(0) < out.stride(1) and (out.cpu().numpy()[live] == want[live]).all()
    # a strided out
    wide = torch.full((ns, t, sz + 24), GUARD, dtype=torch.uint8, device="cuda")
    dec.repair_batch(blocks, nums, per_stripe, out=wide[:, :, :sz])
    host = wide.cpu().numpy()
    assert (host[:, :, :sz] == want).all() and (host[:, :, sz:] == GUARD).all()
