"""GPU checks of the batched error location (fec_locate_batch;
zfec_amd/csrc/kernels.hip matlocate_reg<K,R> for k <= 4 with 2 <= c <= 8, the
verify kernels for c == 1, the expected rows through the encode kernels plus
rows_locate past that, then locate_finish).  Shares come from the CPU oracle's
encode; the expected verdicts come from the numpy model of the definition
(tests/locate_ref.py), never from the library.  Inputs start at byte offset 3.
The verdict words are pre-filled with 0xA5A5A5A5 and sit between guard words:
after every call the guards are unchanged, the verdicts exact, src is
byte-identical to what was uploaded, and the kernel name is the expected one."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from locate_ref import CLEAN, MANY, UNKNOWN, oracle_PQ, verdicts
from test_gpu_verify import IN_OFF, TAIL, Layout, bases, stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5A5A5A5
GW = 4  # guard words before and after the verdicts

SIZES = (1, 15, 16, 17, 1023, 1024, 1025, 4097)
NS = (1, 3, 70)
NSMAX, SZMAX = 70, 4097


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def kernel_name(k, c):
    if c == 1:
        return "matverify_reg<%d,1>" % k if k <= 4 else "rows_differ"
    return "matlocate_reg<%d,%d>" % (k, c) if k <= 4 and c <= 8 else "rows_locate"


def some_slots(n, rng, most=5):
    """Up to `most` of n slots: the first, the last, both sides of a 32-slot
    word boundary and random ones."""
    if n <= most:
        return list(range(n))
    pick = {0, n - 1}
    if n > 32:
        pick |= {31, 32}
    while len(pick) < most:
        pick.add(int(rng.integers(0, n)))
    return sorted(pick)


def patterns(k, c, ns, sz, seed):
    """name -> corruption list [(stripe, slot, byte positions, xor values)]."""
    rng = np.random.default_rng(seed)
    nb = k + c
    nz = lambda n=None: rng.integers(1, 256, size=n, dtype=np.uint8)  # noqa: E731

    def one(s, j, x):
        return (s, j, np.array([x]), np.array([nz()], dtype=np.uint8))

    mid = sz // 2
    tail = sz - sz % 16 if sz % 16 and sz > 16 else max(0, sz - 16)
    positions = sorted({0, sz - 1, tail, mid})
    out = {"clean": []}
    # one byte of one block per stripe, the stripes next to each other: every
    # basis slot at the first, the last, a tail and a middle byte, then checks
    items = [(j, x) for x in positions for j in some_slots(k, rng)]
    items += [(k + i, x) for x in (0, sz - 1) for i in some_slots(c, rng, 3)]
    if ns == 1:
        items = [items[i] for i in rng.permutation(len(items))[:6]]
    for r0 in range(0, len(items), ns):
        out["single bytes %d" % r0] = [one(s, j, x) for s, (j, x) in enumerate(items[r0:r0 + ns])]
    s = ns // 2
    j = int(rng.integers(0, nb))
    out["whole block"] = [(s, j, np.arange(sz), nz(sz))]
    xs = np.unique(np.array([(int(rng.integers(0, 1024)) + 1024 * h) % sz for h in range(5)]))
    out["several bytes of a basis block"] = [(s, int(rng.integers(0, k)), xs, nz(len(xs)))]
    out["several bytes of a check"] = [(s, k + int(rng.integers(0, c)), xs, nz(len(xs)))]
    if nb >= 3 or c >= 2:
        a, b = (int(v) for v in rng.permutation(nb)[:2])
        out["two blocks, one byte"] = [one(s, a, mid), one(s, b, mid)]
        a, b = (int(v) for v in rng.permutation(k + 1)[:2])  # at least one basis slot
        if sz >= 2:
            # far apart: different waves each see a single-slot error, only the
            # OR across waves gives MANY
            out["two blocks, far apart"] = [one(s, a, 0), one(s, b, sz - 1)]
        if k >= 2 and sz >= 2:
            out["two basis blocks, far apart"] = [one(s, 0, sz - 1), one(s, k - 1, 0)]
    if ns >= 3:
        # different culprits in neighbouring stripes, clean stripes between them
        cor = []
        for t in range(0, ns, 3):
            cor.append(one(t, int(rng.integers(0, nb)), int(rng.integers(0, sz))))
            if t + 1 < ns:
                cor.append(one(t + 1, int(rng.integers(0, nb)), int(rng.integers(0, sz))))
        out["neighbours"] = cor
    return out


class Case(object):
    """ns stripes of the blocks `nums` (first k the basis) in one layout."""

    def __init__(self, k, m, nums, ns, sz, kind="padded", src_mem="device", szmax=SZMAX):
        self.k, self.m, self.nums, self.ns, self.sz = k, m, list(nums), ns, sz
        self.nb = len(self.nums)
        self.c = self.nb - k
        self.src_mem = src_mem
        self.clean = np.ascontiguousarray(stripes(k, m, NSMAX, szmax)[:ns][:, self.nums, :sz])
        self.lay = Layout(kind, ns, self.nb, sz)
        self.P, self.Q = oracle_PQ(k, m, tuple(self.nums))

    def upload(self, corruptions):
        blocks = self.clean.copy()
        for s, j, xs, vs in corruptions:
            blocks[s, j, xs] ^= vs
        host = np.zeros(IN_OFF + self.lay.nbytes + TAIL, dtype=np.uint8)
        self.lay.view(host[IN_OFF:IN_OFF + self.lay.nbytes])[:, :, :self.sz] = blocks
        t = torch.from_numpy(host)
        self.src = t.cuda() if self.src_mem == "device" else t.pin_memory()
        return blocks

    def run(self, code, corruptions, what, out_mem="device", stream=None, flags=capi.FEC_FLAG_ASYNC):
        """Corrupt, locate, check everything; returns the verdicts (ns,)."""
        blocks = self.upload(corruptions)
        want = verdicts(self.P, self.Q, blocks)
        uploaded = self.src.clone()
        n = self.ns
        words = np.full(GW + n + GW, FILL, dtype=np.uint32)
        if out_mem == "device":
            out = torch.from_numpy(words.view(np.int32)).cuda()
            ptr = out.data_ptr() + 4 * GW
        elif out_mem == "pinned":
            out = torch.from_numpy(words.view(np.int32)).pin_memory()
            ptr = out.data_ptr() + 4 * GW
        else:
            out = words
            ptr = words.ctypes.data + 4 * GW
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if flags & capi.FEC_FLAG_LIBRARY_STREAM:
            torch.cuda.synchronize()  # the library's stream does not wait for the upload's
        code.locate_batch(self.src.data_ptr() + IN_OFF, self.lay.bs, self.lay.ss, self.nums, self.sz, self.ns, ptr,
                          stream=st, flags=flags)
        got_name = capi.last_kernel_name()
        torch.cuda.synchronize()
        got = out if out_mem == "numpy" else out.cpu().numpy().view(np.uint32)
        assert (got[:GW] == FILL).all() and (got[GW + n:] == FILL).all(), ("guard words", what)
        got = got[GW:GW + n].copy()
        assert (got == want).all(), (what, got_name, [(int(i), hex(got[i]), hex(want[i]))
                                                      for i in np.nonzero(got != want)[0][:4]])
        assert torch.equal(self.src, uploaded), ("src was written", what)
        assert got_name == kernel_name(self.k, self.c), (what, got_name)
        return got


def sweep(k, m, c, kind, sizes, nss, seed, which=None):
    code = capi.Code(k, m)
    seen = set()
    for bname, nums in bases(k, m, seed):
        if which is not None and bname not in which:
            continue
        for ns in nss:
            for sz in sizes:
                case = Case(k, m, nums[:k + c], ns, sz, kind)
                for pname, cor in patterns(k, c, ns, sz, seed + sz + ns).items():
                    seen |= set(case.run(code, cor, (k, m, c, kind, bname, ns, sz, pname)).tolist())
    return seen


# ---- the fused kernel, and c == 1 through verify -----------------------------------------

FUSED = [(1, 3, 2), (2, 4, 2), (4, 12, 8)] + [(3, 10, c) for c in range(1, 8)]


@pytest.mark.parametrize("k,m,c", FUSED)
def test_fused_all_sizes_and_batches(k, m, c):
    """Padded layout, every size with every batch: the byte tail (1, 15), exact
    chunks (16, 1024: exactly one wave), the overlapped last chunk (17, 1023),
    one wave plus one unit (1025) and four waves plus one unit (4097) per
    stripe.  c == 1 answers CLEAN or UNKNOWN only."""
    seen = sweep(k, m, c, "padded", SIZES, NS, seed=100 * k + m + c)
    assert CLEAN in seen
    if c == 1:
        assert seen == {CLEAN, UNKNOWN}
    else:
        assert MANY in seen and UNKNOWN not in seen
        assert {0, k - 1, k, k + c - 1} <= seen  # basis and check slots were named


@pytest.mark.parametrize("kind", ["packed", "bm"])
@pytest.mark.parametrize("k,m,c", FUSED)
def test_fused_layouts(k, m, c, kind):
    sweep(k, m, c, kind, SIZES, (3,), seed=200 * k + m + c)
    sweep(k, m, c, kind, (1025,), (70,), seed=300 * k + m + c, which=("mixed",))


def test_grid_stride(knobs):
    """Three workgroups (12 waves) walk 37 stripes of 3 waves each.  A step of
    12 waves is exactly 4 stripes here (gs_w = 0), so the carry of the walk
    never runs: test_gpu_wave_walk.py has the geometries with gs_w != 0."""
    k, m, c = 3, 10, 7
    code = capi.Code(k, m)
    knobs(ZFEC_HIP_GRID_CAP=3)
    case = Case(k, m, range(m), 37, 2049)
    for pname, cor in patterns(k, c, 37, 2049, 5).items():
        case.run(code, cor, ("capped", pname))


def test_split_launches(knobs):
    """Launches of at most 1024 units: 4 KiB stripes in groups of 4 (the word
    pointer advanced per group), 20000-byte blocks in byte ranges of 16 KiB
    (the bits of one stripe come from two launches)."""
    k, m, c = 3, 10, 7
    code = capi.Code(k, m)
    knobs(ZFEC_HIP_LAUNCH_UNITS=1024)
    for ns, sz in ((37, 4096), (5, 20000)):
        case = Case(k, m, range(m), ns, sz, szmax=max(SZMAX, sz))
        for pname, cor in patterns(k, c, ns, sz, sz).items():
            case.run(code, cor, (ns, sz, pname))
        one = lambda s, j, x: (s, j, np.array([x]), np.array([0x21], dtype=np.uint8))  # noqa: E731
        far = 16384 if sz > 16384 else 5
        assert case.run(code, [one(ns - 1, 1, sz - 1), one(ns - 1, 1, 3)], "one slot, two ranges")[ns - 1] == 1
        assert case.run(code, [one(ns - 1, 1, far), one(ns - 1, 2, 3)], "two slots, two ranges")[ns - 1] == MANY


# ---- rows_locate ----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,c", [(4, 13, 9), (5, 8, 3), (10, 16, 6), (33, 36, 3), (4, 60, 56)])
def test_scratch_path(k, m, c):
    """k <= 4 with more than 8 checks, the smallest k > 4, a wide code, more
    than 32 basis slots (two excluded words), and more than kMaxOut checks (row
    0's pair is read again by the second group of rows)."""
    seen = sweep(k, m, c, "padded", SIZES, (1, 3), seed=400 * k + m, which=("primaries", "mixed"))
    seen |= sweep(k, m, c, "bm", (17, 1025), (3,), seed=500 * k + m, which=("parity", "mixed"))
    seen |= sweep(k, m, c, "packed", (1025,), (70,), seed=600 * k + m, which=("mixed",))
    assert {CLEAN, MANY, 0, k - 1, k, k + c - 1} <= seen and UNKNOWN not in seen


def test_scratch_path_wide():
    seen = sweep(20, 60, 40, "padded", (1025,), (3,), seed=2060, which=("mixed",))
    assert {CLEAN, MANY} <= seen


@pytest.mark.parametrize("k,m", [(5, 6), (10, 11)])
def test_one_check_past_the_register_path(k, m):
    assert sweep(k, m, 1, "padded", (17, 1025), (3,), seed=k, which=("mixed",)) == {CLEAN, UNKNOWN}


def test_scratch_cap_cuts_are_invisible(knobs):
    """A test-only scratch cap of 64 KiB.  K=10/M=16: 4097-byte blocks go in
    runs of 2 stripes; 10923-byte blocks stripe by stripe in byte ranges of
    10880 and 43 bytes, one slot corrupted on both sides of the cut."""
    knobs(ZFEC_HIP_VERIFY_SCRATCH=65536)
    k, m, c = 10, 16, 6
    code = capi.Code(k, m)
    case = Case(k, m, range(m), 5, 4097)
    for pname, cor in patterns(k, c, 5, 4097, 1).items():
        case.run(code, cor, ("runs", pname))
    sz = 10923
    case = Case(k, m, range(m), 3, sz, szmax=sz)
    for pname, cor in patterns(k, c, 3, sz, 2).items():
        case.run(code, cor, ("ranges", pname))
    one = lambda s, j, x: (s, j, np.array([x]), np.array([0x33], dtype=np.uint8))  # noqa: E731
    assert case.run(code, [one(2, 7, 10900), one(2, 7, 5)], "one slot, both ranges")[2] == 7
    assert case.run(code, [one(1, 7, 10900), one(1, 3, 5)], "two slots, one per range")[1] == MANY


# ---- memory kinds, streams, refusals ---------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
@pytest.mark.parametrize("out_mem", ["numpy", "pinned"])
def test_culprit_in_host_memory(k, m, out_mem):
    """The verdicts are gathered in device memory the library owns and copied
    back; the call is synchronous whatever the flags."""
    ns, sz = 37, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    for flags in (capi.FEC_FLAG_ASYNC, 0, capi.FEC_FLAG_LIBRARY_STREAM):
        for pname, cor in patterns(k, m - k, ns, sz, 3).items():
            case.run(code, cor, (out_mem, flags, pname), out_mem=out_mem, flags=flags)


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_src_in_page_locked_host_memory(k, m):
    ns, sz = 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz, src_mem="pinned")
    for out_mem in ("device", "numpy"):
        for pname, cor in patterns(k, m - k, ns, sz, 4).items():
            case.run(code, cor, (out_mem, pname), out_mem=out_mem, flags=0)


def test_deterministic():
    k, m, ns, sz = 3, 10, 70, 4097
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    cor = patterns(k, m - k, ns, sz, 9)["neighbours"]
    assert (case.run(code, cor, "first") == case.run(code, cor, "second")).all()


def test_empty_calls():
    """nstripes == 0 touches nothing; sz == 0 answers CLEAN for every stripe."""
    k, m = 3, 10
    code = capi.Code(k, m)
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.full((8,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code.locate_batch(src.data_ptr(), 0, 0, list(range(m)), 16, 0, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == FILL).all()
    code.locate_batch(src.data_ptr(), 0, 0, list(range(m)), 0, 3, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == [FILL] * 2 + [CLEAN] * 3 + [FILL] * 3
    host = np.full(8, FILL, dtype=np.uint32)
    code.locate_batch(src.data_ptr(), 0, 0, list(range(m)), 0, 3, host.ctypes.data + 8, stream=st)
    assert host.tolist() == [FILL] * 2 + [CLEAN] * 3 + [FILL] * 3


def test_pageable_src_is_refused():
    k, m = 3, 10
    src = np.zeros(4 * m * 64, dtype=np.uint8)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.FecError, match="pageable host memory, which this call does not stage"):
        capi.Code(k, m).locate_batch(src.ctypes.data, 64, m * 64, list(range(m)), 64, 4, out.data_ptr())


def test_culprit_on_another_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    k, m, ns, sz = 3, 10, 3, 64
    case = Case(k, m, range(m), ns, sz)
    case.upload([])
    other = torch.zeros(16, dtype=torch.int32, device="cuda:1")
    with pytest.raises(capi.FecError, match="culprit lives on device 1, the blocks on device 0"):
        capi.Code(k, m).locate_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns,
                                     other.data_ptr())


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_two_streams(k, m):
    """Asynchronous calls back to back on two streams: each waits on the GPU
    for the call that used the thread's working words (and scratch) before it."""
    ns, sz = 5, 4097
    code = capi.Code(k, m)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for i in range(6):
        case = Case(k, m, range(m), ns, sz)
        cor = [(i % ns, (2 * i) % m, np.array([(i * 700) % sz]), np.array([1 + i], dtype=np.uint8))]
        if i % 3 == 2:
            cor.append(((i + 1) % ns, 1, np.array([5, 3000]), np.array([7, 9], dtype=np.uint8)))
        want = verdicts(case.P, case.Q, case.upload(cor))
        out = torch.full((ns,), -1, dtype=torch.int32, device="cuda")
        runs.append((case, want, out))
    torch.cuda.synchronize()
    for i, (case, want, out) in enumerate(runs):
        code.locate_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns, out.data_ptr(),
                          stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, (case, want, out) in enumerate(runs):
        assert (out.cpu().numpy().view(np.uint32) == want).all(), i
        assert want[i % ns] == (2 * i) % m


def test_declines_under_graph_capture():
    k, m, ns, sz = 3, 10, 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    case.run(code, [(1, 4, np.array([5]), np.array([1], dtype=np.uint8))], "outside the capture")
    out = torch.zeros(ns, dtype=torch.int32, device="cuda")
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                code.locate_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns,
                                  out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()


# ---- Python API --------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (3, 4), (10, 16)])
def test_python_api(k, m):
    ns, sz = 37, 1025
    dec = zfec_amd.Decoder(k, m)
    rng = np.random.default_rng(m)
    nums = rng.permutation(m).tolist()
    c = m - k
    P, Q = oracle_PQ(k, m, tuple(nums))
    clean_host = np.ascontiguousarray(stripes(k, m, NSMAX, SZMAX)[:ns][:, nums, :sz])
    host = clean_host.copy()
    for s, j, x, v in [(3, m - 1, sz - 1, 1), (4, k, 0, 2), (9, 0, 500, 3), (36, k - 1, 17, 4), (20, 0, 1, 5),
                       (20, m - 1, 1024, 6)]:
        host[s, j, x] ^= v
    want = verdicts(P, Q, host).view(np.int32)
    if c >= 2:
        assert want[[3, 4, 9, 36, 20]].tolist() == [m - 1, k, 0, k - 1, zfec_amd.LOCATE_MANY]
    else:
        assert set(want[[3, 4, 9, 36, 20]].tolist()) == {zfec_amd.LOCATE_UNKNOWN}
    assert (want == zfec_amd.LOCATE_CLEAN).sum() == ns - 5
    blocks = torch.from_numpy(host).cuda()
    out = dec.locate_batch(blocks, nums)
    assert out.dtype == torch.int32 and tuple(out.shape) == (ns,) and out.device == blocks.device
    assert (out.cpu().numpy() == want).all()
    # block-major input
    bm = blocks.transpose(0, 1).contiguous().transpose(0, 1)
    assert (dec.locate_batch(bm, nums).cpu().numpy() == want).all()
    # on a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dec.locate_batch(blocks, nums)
    s.synchronize()
    assert (out.cpu().numpy() == want).all()
    # a clean batch, and empty ones
    clean = torch.from_numpy(clean_host).cuda()
    assert (dec.locate_batch(clean, nums) == zfec_amd.LOCATE_CLEAN).all()
    assert tuple(dec.locate_batch(clean[:0], nums).shape) == (0,)
    empty = dec.locate_batch(clean[:, :, :0], nums)
    assert empty.dtype == torch.int32 and empty.tolist() == [zfec_amd.LOCATE_CLEAN] * ns
    assert torch.equal(blocks.cpu(), torch.from_numpy(host))


def test_scrub_locate_repair_end_to_end():
    """K=3/M=10, 70 stripes of 4097 bytes, one random block overwritten in a
    third of the stripes: verify_batch flags them, locate_batch names the slot,
    repair_batch rebuilds it from the first k other slots -- three calls, the
    patterns built on the device from the verdicts -- and every block then
    equals the oracle's."""
    k, m, ns, sz = 3, 10, 70, 4097
    dec = zfec_amd.Decoder(k, m)
    rng = np.random.default_rng(77)
    nums = rng.permutation(m).tolist()
    clean = np.ascontiguousarray(stripes(k, m, NSMAX, SZMAX)[:ns][:, nums, :sz])
    host = clean.copy()
    bad = np.sort(rng.permutation(ns)[:ns // 3])
    slot = rng.integers(0, m, size=len(bad))
    for s, j in zip(bad, slot):
        host[s, j] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
    blocks = torch.from_numpy(host).cuda()
    flagged = dec.verify_batch(blocks, nums).any(dim=1)
    verdict = dec.locate_batch(blocks, nums)
    want = np.full(ns, zfec_amd.LOCATE_CLEAN, dtype=np.int32)
    want[bad] = slot
    assert (verdict.cpu().numpy() == want).all()
    assert torch.equal(flagged, verdict != zfec_amd.LOCATE_CLEAN)
    # per stripe: the first k slots that are not the culprit, and the culprit's block number as the target
    dev = blocks.device
    nums_t = torch.tensor(nums, dtype=torch.int64, device=dev)
    v = verdict.to(torch.int64)
    idx = torch.arange(k, device=dev).unsqueeze(0).expand(ns, k)
    idx = idx + (idx >= v.unsqueeze(1)).to(torch.int64) * (v.unsqueeze(1) >= 0)
    present = torch.gather(blocks, 1, idx.unsqueeze(-1).expand(ns, k, sz)).contiguous()
    targets = torch.where(v >= 0, nums_t[v.clamp(min=0)], torch.full_like(v, -1)).unsqueeze(1)
    rebuilt = dec.repair_batch(present, nums_t[idx], targets)
    hit = torch.nonzero(v >= 0).squeeze(1)
    blocks[hit, v[hit]] = rebuilt[hit, 0]
    assert (blocks.cpu().numpy() == clean).all()
    assert (dec.locate_batch(blocks, nums) == zfec_amd.LOCATE_CLEAN).all()
