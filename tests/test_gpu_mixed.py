"""GPU parity of the batched decode with a pattern per stripe
(fec_decode_batch_mixed; zfec_amd/csrc/kernels.hip matapply_mixed<K> for k <= 4,
runs of the shared-pattern path past that).  Shares come from the CPU oracle's
encode (zfec/fec.c:487-505) and the expected output is the original data.
Outputs are pre-filled with 0xA5; the bytes before, between and after the rows
must come back unchanged.  Inputs start at offset 3, outputs at offset 5."""
import functools
import itertools

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
TAIL = 64
IN_OFF, OUT_OFF = 3, 5


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


@functools.lru_cache(maxsize=None)
def stripes(k, m, ns, sz, seed=0):
    """data (ns, k, sz) and all m blocks of every stripe (ns, m, sz), read-only.
    Output byte x depends only on byte x of the inputs, so the oracle encodes
    the batch as one long stripe, and a shorter block is a prefix of these."""
    rng = np.random.default_rng(1000 * k + 10 * m + seed)
    data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
    flat = np.ascontiguousarray(data.transpose(1, 0, 2)).reshape(k, ns * sz)
    par = oracle.encode(k, m, flat).reshape(m - k, ns, sz).transpose(1, 0, 2)
    allb = np.concatenate([data, par], axis=1)
    data.setflags(write=False)
    allb.setflags(write=False)
    return data, allb


def received(allb, pats, ids, sz):
    """(ns, k, sz): slot j of stripe s holds block pats[ids[s]][j]."""
    ns = allb.shape[0]
    nums = np.asarray(pats, dtype=np.int64)[np.asarray(ids, dtype=np.int64)]
    return np.ascontiguousarray(allb[np.arange(ns)[:, None], nums, :sz])


def random_patterns(rng, k, m, n):
    """n patterns, each a random k-subset in a random slot order; the first two
    are the all-primaries shuffle and (where the code has k parity blocks) an
    all-parity one."""
    pats = [rng.permutation(k).tolist()]
    if m - k >= k:
        pats.append((k + rng.permutation(m - k)[:k]).tolist())
    while len(pats) < n:
        pats.append(rng.permutation(m)[:k].tolist())
    return pats


class Layout(object):
    """Where block j of stripe s starts, for `rows` rows of sz bytes per stripe:
    packed [s][j][sz], padded (rows sz + 24 apart) or block-major [j][s][sz + 8]."""

    def __init__(self, kind, ns, rows, sz):
        self.kind, self.ns, self.rows, self.sz = kind, ns, rows, sz
        if kind == "bm":
            self.ld = sz + 8
            self.bs, self.ss = ns * self.ld, self.ld
        else:
            self.ld = sz if kind == "packed" else sz + 24
            self.bs, self.ss = self.ld, rows * self.ld
        self.nbytes = ns * rows * self.ld

    def view(self, flat):
        """(ns, rows, ld) view of the flat byte array of nbytes."""
        if self.kind == "bm":
            return flat.reshape(self.rows, self.ns, self.ld).transpose(1, 0, 2)
        return flat.reshape(self.ns, self.rows, self.ld)


class Case(object):
    def __init__(self, recv, kind="padded", device_mem=True):
        self.ns, self.k, self.sz = recv.shape
        self.lin = Layout(kind, self.ns, self.k, self.sz)
        self.lout = Layout(kind, self.ns, self.k, self.sz)
        src = np.zeros(IN_OFF + self.lin.nbytes + TAIL, dtype=np.uint8)
        self.lin.view(src[IN_OFF:IN_OFF + self.lin.nbytes])[:, :, :self.sz] = recv
        dst = np.full(OUT_OFF + self.lout.nbytes + TAIL, GUARD, dtype=np.uint8)
        if device_mem:
            self.src, self.dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        else:
            self.src, self.dst = torch.from_numpy(src).pin_memory(), torch.from_numpy(dst).pin_memory()
        self.keep = None

    def launch(self, code, pats, ids, where="host", stream=None, flags=capi.FEC_FLAG_ASYNC):
        """ids: uint32 numpy array; where: "host" or "device"."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        if where == "device":
            self.keep = torch.from_numpy(ids.view(np.int32)).cuda()
            ptr = self.keep.data_ptr()
        else:
            self.keep = ids
            ptr = ids.ctypes.data
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        code.decode_batch_mixed(self.src.data_ptr() + IN_OFF, self.lin.bs, self.lin.ss,
                                self.dst.data_ptr() + OUT_OFF, self.lout.bs, self.lout.ss, pats, ptr, self.sz, self.ns,
                                stream=st, flags=flags)
        return capi.last_kernel_name()

    def result(self, what=""):
        """The output rows (ns, k, sz), the guards checked; and the whole buffer."""
        torch.cuda.synchronize()
        host = self.dst.cpu().numpy()
        n = self.lout.nbytes
        assert (host[:OUT_OFF] == GUARD).all(), ("write before the output", what)
        assert (host[OUT_OFF + n:] == GUARD).all(), ("write after the output", what)
        body = self.lout.view(host[OUT_OFF:OUT_OFF + n])
        assert (body[:, :, self.sz:] == GUARD).all(), ("write past a row", what)
        return body[:, :, :self.sz], host


def check(code, k, m, ns, sz, pats, ids, kind="padded", where="host", name=True, szmax=None, seed=0):
    data, allb = stripes(k, m, ns, szmax or sz, seed)
    case = Case(received(allb, pats, ids, sz), kind)
    got_name = case.launch(code, pats, ids, where)
    what = (k, m, ns, sz, kind, where, got_name)
    got, host = case.result(what)
    if name:
        assert got_name == "matapply_mixed<%d>" % k, what
    assert (got == data[:, :, :sz]).all(), what
    return host


SIZES = (1, 15, 16, 17, 1023, 1024, 1040, 4096)


@pytest.mark.parametrize("kind", ["packed", "padded", "bm"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sweep(K, kind):
    """37 stripes, each with its own pattern, at the byte tail (1, 15, 17),
    exact chunks (16, 1024: exactly 64), a partly masked wave (1023, 1040: 65
    chunks, a second wave with one live lane) and four waves per stripe."""
    m, ns = K + 4, 37
    code = capi.Code(K, m)
    rng = np.random.default_rng(K)
    pats = random_patterns(rng, K, m, ns)
    for sz in SIZES:
        check(code, K, m, ns, sz, pats, np.arange(ns), kind, szmax=max(SIZES))


def test_all_120_subsets():
    k, m, sz = 3, 10, 1040
    rng = np.random.default_rng(120)
    subs = [list(c) for c in itertools.combinations(range(m), k)]
    pats = subs + [rng.permutation(c).tolist() for c in subs]
    assert len(subs) == 120
    check(capi.Code(k, m), k, m, 240, sz, pats, rng.permutation(240))


@pytest.mark.parametrize("sz", [1040, 4096])
def test_grid_stride(knobs, sz):
    """Two workgroups (8 waves) walk 37 stripes of 2 or 4 waves each.  A step
    of 8 waves is exactly 4 or 2 stripes here (gs_w = 0), so the carry of the
    walk never runs: test_gpu_wave_walk.py has the geometries with gs_w != 0."""
    knobs(ZFEC_HIP_GRID_CAP=2)
    k, m, ns = 3, 10, 37
    pats = random_patterns(np.random.default_rng(sz), k, m, ns)
    check(capi.Code(k, m), k, m, ns, sz, pats, np.arange(ns), szmax=4096)


@pytest.mark.parametrize("sz,ns", [(4096, 37), (20000, 5)])
def test_split_launches(knobs, sz, ns):
    """ZFEC_HIP_LAUNCH_UNITS=1024: 4 KiB stripes go in groups of 4 (the id
    pointer advanced per group), 20000-byte blocks in byte ranges of 16 KiB."""
    knobs(ZFEC_HIP_LAUNCH_UNITS=1024)
    k, m = 3, 10
    pats = random_patterns(np.random.default_rng(sz), k, m, ns)
    check(capi.Code(k, m), k, m, ns, sz, pats, np.arange(ns), seed=1)


@pytest.mark.parametrize("where", ["host", "device"])
def test_id_width(where):
    """66,000 stripes of one chunk: more stripes (and waves) than 16 bits count."""
    k, m, ns, sz = 3, 10, 66000, 16
    pats = [list(c) for c in itertools.combinations(range(m), k)]
    check(capi.Code(k, m), k, m, ns, sz, pats, np.arange(ns) % 120, "packed", where)


def test_host_and_device_ids_identical():
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    rng = np.random.default_rng(7)
    pats = random_patterns(rng, k, m, 9)
    ids = rng.integers(0, 9, size=ns)
    a = check(code, k, m, ns, sz, pats, ids, where="host", szmax=4096)
    b = check(code, k, m, ns, sz, pats, ids, where="device", szmax=4096)
    assert (a == b).all()


@pytest.mark.parametrize("kind", ["padded", "bm"])
def test_agrees_with_shared_pattern_call(kind):
    """One pattern that obeys fec_decode's slot rule: the same bytes as
    fec_decode_batch with FEC_FLAG_ALL_PRIMARIES."""
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    pat = [0, 7, 5]
    ids = np.zeros(ns, dtype=np.uint32)
    mixed = check(code, k, m, ns, sz, [pat], ids, kind, szmax=4096)
    data, allb = stripes(k, m, ns, 4096)
    case = Case(received(allb, [pat], ids, sz), kind)
    code.decode_batch(case.src.data_ptr() + IN_OFF, case.lin.bs, case.lin.ss, case.dst.data_ptr() + OUT_OFF,
                      case.lout.bs, case.lout.ss, pat, sz, ns, stream=torch.cuda.current_stream().cuda_stream,
                      flags=capi.FEC_FLAG_ASYNC | capi.FEC_FLAG_ALL_PRIMARIES)
    assert not capi.last_kernel_name().startswith("matapply_mixed")
    got, host = case.result(kind)
    assert (got == data[:, :, :sz]).all()
    assert (host == mixed).all()


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
        pats = random_patterns(rng, k, m, 5 + i)
        ids = rng.integers(0, len(pats), size=ns)
        cases.append((Case(received(allb, pats, ids, sz)), pats, ids))
    torch.cuda.synchronize()
    for i, (case, pats, ids) in enumerate(cases):
        s = streams[i % 2]
        assert case.launch(code, pats, ids, "host" if i % 3 else "device", stream=s.cuda_stream) == "matapply_mixed<3>"
    for i, (case, _, _) in enumerate(cases):
        got, _ = case.result(i)
        assert (got == data[:, :, :sz]).all(), i


def test_page_locked_host_memory():
    """src and dst in page-locked host memory are read and written in place."""
    k, m, ns, sz = 3, 10, 37, 1040
    data, allb = stripes(k, m, ns, 4096)
    rng = np.random.default_rng(3)
    pats = random_patterns(rng, k, m, 7)
    ids = rng.integers(0, 7, size=ns)
    case = Case(received(allb, pats, ids, sz), device_mem=False)
    assert case.launch(capi.Code(k, m), pats, ids, flags=0) == "matapply_mixed<3>"
    got, _ = case.result()
    assert (got == data[:, :, :sz]).all()


def test_declines_under_graph_capture():
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    data, allb = stripes(k, m, ns, 4096)
    pats, ids = [[7, 8, 9], [2, 0, 5]], np.arange(ns) % 2
    case = Case(received(allb, pats, ids, sz))
    case.launch(code, pats, ids)  # outside the capture: works
    assert (case.result()[0] == data[:, :, :sz]).all()
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                case.launch(code, pats, ids)
    torch.cuda.synchronize()


WIDE_IDS = [0, 0, 0, 1, 1, 2, 0, 0, 2, 2, 2, 1]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k,m", [(5, 9), (20, 60)])
def test_fallback_past_the_register_shapes(k, m, where):
    """k > 4: runs of consecutive stripes with one id through the shared-pattern path."""
    ns, sz = 12, 2049
    rng = np.random.default_rng(k)
    pats = random_patterns(rng, k, m, 3)
    host = check(capi.Code(k, m), k, m, ns, sz, pats, WIDE_IDS, "padded", where, name=False)
    assert host is not None and not capi.last_kernel_name().startswith("matapply_mixed")


def test_python_api():
    k, m, ns, sz = 3, 10, 37, 1040
    dec = zfec_amd.Decoder(k, m)
    data, allb = stripes(k, m, ns, 4096)
    rng = np.random.default_rng(4)
    pats = random_patterns(rng, k, m, 11)
    ids = rng.integers(0, 11, size=ns)
    nums = np.asarray(pats)[ids]  # (ns, k)
    blocks = torch.from_numpy(received(allb, pats, ids, sz)).cuda()
    want = data[:, :, :sz]
    forms = {
        "lists": nums.tolist(),
        "numpy": nums,
        "host tensor": torch.from_numpy(nums),
        "device tensor": torch.from_numpy(nums).cuda(),
        "pair": (pats, ids.tolist()),
        "pair, device ids": (np.asarray(pats), torch.from_numpy(ids).cuda()),
    }
    for what, form in forms.items():
        out = dec.decode_batch_mixed(blocks, form)
        assert capi.last_kernel_name() == "matapply_mixed<3>", what
        assert tuple(out.shape) == (ns, k, sz) and out.is_contiguous(), what
        assert (out.cpu().numpy() == want).all(), what
    # block-major input gives block-major output
    bm = blocks.transpose(0, 1).contiguous().transpose(0, 1)
    out = dec.decode_batch_mixed(bm, nums)
    assert out.stride(0) < out.stride(1) and (out.cpu().numpy() == want).all()
    # stripe by stripe: Decoder.decode on the same blocks
    for s in range(ns):
        one = dec.decode([blocks[s, j] for j in range(k)], [int(x) for x in nums[s]])
        assert (torch.stack(one).cpu().numpy() == want[s]).all(), s
