"""GPU checks of the batched in-place correction (fec_correct_batch: the
location path of fec_locate_batch, then zfec_amd/csrc/kernels.hip
matcorrect_reg<K> for k <= 4 or rows_correct past that).  Shares come from the
CPU oracle's encode; the expected verdicts and the expected blocks come from
the numpy model of the definition (tests/correct_ref.py), never from the
library.  Inputs start at byte offset 3.  The block buffer is pre-filled with
random bytes, so row slack and the bytes around the blocks act as guards, and
the verdict words sit between 0xA5A5A5A5 guard words.  After every call the
verdicts are exact, the ENTIRE block buffer is byte-identical to the model's
blocks_after laid into the same pre-filled buffer (corrected rows, untouched
stripes, slack and guards in one comparison), and the kernel name is the
expected one."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from correct_ref import corrected
from locate_ref import CLEAN, MANY, UNKNOWN, oracle_PQ
from test_gpu_locate import patterns
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


def kernel_name(k):
    return "matcorrect_reg<%d>" % k if k <= 4 else "rows_correct"


def one(s, j, x, v=0x21):
    return (s, j, np.array([x]), np.array([v], dtype=np.uint8))


class Case(object):
    """ns stripes of the blocks `nums` (first k the basis) in one layout."""

    def __init__(self, k, m, nums, ns, sz, kind="padded", mem="device", szmax=SZMAX):
        self.k, self.m, self.nums, self.ns, self.sz = k, m, list(nums), ns, sz
        self.nb = len(self.nums)
        self.c = self.nb - k
        self.mem = mem
        self.clean = np.ascontiguousarray(stripes(k, m, NSMAX, szmax)[:ns][:, self.nums, :sz])
        self.lay = Layout(kind, ns, self.nb, sz)
        self.P, self.Q = oracle_PQ(k, m, tuple(self.nums))
        self.prefill = np.random.default_rng(ns * 131 + sz).integers(
            0, 256, size=IN_OFF + self.lay.nbytes + TAIL, dtype=np.uint8)

    def lay_in(self, blocks):
        """The pre-filled host buffer with `blocks` (ns, nb, sz) laid into it."""
        host = self.prefill.copy()
        self.lay.view(host[IN_OFF:IN_OFF + self.lay.nbytes])[:, :, :self.sz] = blocks
        return host

    def corrupt(self, corruptions):
        blocks = self.clean.copy()
        for s, j, xs, vs in corruptions:
            blocks[s, j, xs] ^= vs
        return blocks

    def upload(self, blocks):
        t = torch.from_numpy(self.lay_in(blocks))
        self.buf = t.cuda() if self.mem == "device" else t.pin_memory()
        return self.buf

    def call(self, code, ptr, stream=None, flags=capi.FEC_FLAG_ASYNC):
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        code.correct_batch(self.buf.data_ptr() + IN_OFF, self.lay.bs, self.lay.ss, self.nums, self.sz, self.ns, ptr,
                           stream=st, flags=flags)

    def run(self, code, corruptions, what, out_mem="device", stream=None, flags=capi.FEC_FLAG_ASYNC, blocks=None):
        """Corrupt (or take `blocks`), correct, check everything; returns
        (verdicts (ns,), the model's blocks_after)."""
        if blocks is None:
            blocks = self.corrupt(corruptions)
        want, after = corrected(self.P, self.Q, blocks)
        self.upload(blocks)
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
        if flags & capi.FEC_FLAG_LIBRARY_STREAM:
            torch.cuda.synchronize()  # the library's stream does not wait for the upload's
        self.call(code, ptr, stream, flags)
        got_name = capi.last_kernel_name()
        torch.cuda.synchronize()
        got = out if out_mem == "numpy" else out.cpu().numpy().view(np.uint32)
        assert (got[:GW] == FILL).all() and (got[GW + n:] == FILL).all(), ("guard words", what)
        got = got[GW:GW + n].copy()
        assert (got == want).all(), (what, got_name, [(int(i), hex(got[i]), hex(want[i]))
                                                      for i in np.nonzero(got != want)[0][:4]])
        have = self.buf.cpu().numpy()
        expect = self.lay_in(after)
        if not (have == expect).all():
            bad = np.nonzero(have != expect)[0]
            where = [(int(o), divmod(int(o) - IN_OFF, self.lay.ss if self.lay.kind != "bm" else self.lay.bs))
                     for o in bad[:4]]
            raise AssertionError(("block buffer", what, got_name, len(bad), where))
        assert got_name == kernel_name(self.k), (what, got_name)
        return got, after


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
                    seen |= set(case.run(code, cor, (k, m, c, kind, bname, ns, sz, pname))[0].tolist())
    return seen


def saw_everything(seen, k, c):
    """CLEAN, MANY and a corrected slot 0, k-1, k and k+c-1."""
    assert {CLEAN, MANY, 0, k - 1, k, k + c - 1} <= seen and UNKNOWN not in seen, sorted(seen)


# ---- the register kernel ---------------------------------------------------------------------

REG = [(1, 3, 2), (2, 4, 2), (3, 10, 2), (3, 10, 7), (4, 12, 8)]


@pytest.mark.parametrize("k,m,c", REG)
def test_reg_all_sizes_and_batches(k, m, c):
    """Padded layout, every size with every batch: the byte tail (1, 15), exact
    chunks (16, 1024: exactly one wave), the overlapped last chunk (17, 1023),
    one wave plus one unit (1025) and four waves plus one unit (4097)."""
    saw_everything(sweep(k, m, c, "padded", SIZES, NS, seed=100 * k + m + c), k, c)


@pytest.mark.parametrize("kind", ["packed", "bm"])
@pytest.mark.parametrize("k,m,c", REG)
def test_reg_layouts(k, m, c, kind):
    seen = sweep(k, m, c, kind, SIZES, (3,), seed=200 * k + m + c)
    seen |= sweep(k, m, c, kind, (1025,), (70,), seed=300 * k + m + c, which=("mixed",))
    saw_everything(seen, k, c)


def test_one_check_rewrites_nothing():
    """c == 1: CLEAN or UNKNOWN only, and the buffer stays as uploaded."""
    assert sweep(3, 10, 1, "padded", SIZES, NS, seed=311) == {CLEAN, UNKNOWN}


def test_dispatch_by_k_alone():
    """Nine checks locate on rows_locate, k = 4 corrects on matcorrect_reg<4>
    (Case.run checks the name)."""
    k, m, c = 4, 13, 9
    seen = sweep(k, m, c, "padded", (17, 1025), (1, 3), seed=413, which=("primaries", "mixed"))
    saw_everything(seen, k, c)


# ---- rows_correct --------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,c", [(5, 8, 3), (10, 16, 6), (33, 36, 3)])
def test_rows_correct(k, m, c):
    """The smallest k > 4, a wide code, and culprit slots on both sides of the
    32-slot word boundary (test_gpu_locate.some_slots picks 31 and 32)."""
    seen = sweep(k, m, c, "padded", SIZES, (1, 3), seed=400 * k + m, which=("primaries", "mixed"))
    seen |= sweep(k, m, c, "bm", (17, 1025), (3,), seed=500 * k + m, which=("parity", "mixed"))
    seen |= sweep(k, m, c, "packed", (1025,), (70,), seed=600 * k + m, which=("mixed",))
    saw_everything(seen, k, c)
    if k > 32:
        assert {31, 32} <= seen


def test_rows_correct_wide():
    seen = sweep(20, 60, 40, "padded", (1025,), (3,), seed=2060, which=("mixed",))
    assert {CLEAN, MANY} <= seen and any(v < 60 for v in seen)


# ---- walks ----------------------------------------------------------------------------------------

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
    """Launches of at most 1024 units: 4 KiB stripes in groups of 4 (the verdict
    pointer advanced per group), 20000-byte blocks in byte ranges of 16 KiB.  A
    culprit corrupted in two byte ranges of one stripe is fully restored; two
    different slots in two ranges give MANY and no write."""
    k, m, c = 3, 10, 7
    code = capi.Code(k, m)
    knobs(ZFEC_HIP_LAUNCH_UNITS=1024)
    for ns, sz in ((37, 4096), (5, 20000)):
        case = Case(k, m, range(m), ns, sz, szmax=max(SZMAX, sz))
        for pname, cor in patterns(k, c, ns, sz, sz).items():
            case.run(code, cor, (ns, sz, pname))
        far = 16384 if sz > 16384 else 5
        got, after = case.run(code, [one(ns - 1, 1, sz - 1), one(ns - 1, 1, 3)], "one slot, two ranges")
        assert got[ns - 1] == 1 and (after == case.clean).all()
        cor = [one(ns - 1, 1, far), one(ns - 1, 2, 3)]
        got, after = case.run(code, cor, "two slots, two ranges")
        assert got[ns - 1] == MANY and (after == case.corrupt(cor)).all()


def test_scratch_cap_cuts_are_invisible(knobs):
    """A test-only scratch cap of 64 KiB on the location path.  K=10/M=16:
    4097-byte blocks go in runs of 2 stripes; 10923-byte blocks stripe by stripe
    in byte ranges of 10880 and 43 bytes, one slot corrupted on both sides of
    the cut and restored on both."""
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
    got, after = case.run(code, [one(2, 7, 10900, 0x33), one(2, 7, 5, 0x33)], "one slot, both ranges")
    assert got[2] == 7 and (after == case.clean).all()
    assert case.run(code, [one(1, 7, 10900), one(1, 3, 5)], "two slots, one per range")[0][1] == MANY


# ---- memory kinds, streams, refusals ---------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
@pytest.mark.parametrize("out_mem", ["numpy", "pinned"])
def test_culprit_in_host_memory(k, m, out_mem):
    """The verdicts are gathered in device words the library owns, which the
    correction reads, and copied back; the call is synchronous whatever the
    flags."""
    ns, sz = 37, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    for flags in (capi.FEC_FLAG_ASYNC, 0, capi.FEC_FLAG_LIBRARY_STREAM):
        for pname, cor in patterns(k, m - k, ns, sz, 3).items():
            case.run(code, cor, (out_mem, flags, pname), out_mem=out_mem, flags=flags)


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_blocks_in_page_locked_host_memory(k, m):
    """Read and corrected in place, by plain stores."""
    ns, sz = 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz, mem="pinned")
    seen = set()
    for out_mem in ("device", "numpy"):
        for pname, cor in patterns(k, m - k, ns, sz, 4).items():
            seen |= set(case.run(code, cor, (out_mem, pname), out_mem=out_mem, flags=0)[0].tolist())
    assert any(v < m for v in seen)


def test_pageable_blocks_are_refused():
    k, m = 3, 10
    blocks = np.zeros(4 * m * 64, dtype=np.uint8)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.FecError, match="fec_correct_batch takes device or page-locked host memory: blocks is "
                                            "pageable host memory, which this call does not stage"):
        capi.Code(k, m).correct_batch(blocks.ctypes.data, 64, m * 64, list(range(m)), 64, 4, out.data_ptr())
    assert not blocks.any()


def test_culprit_on_another_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    k, m, ns, sz = 3, 10, 3, 64
    case = Case(k, m, range(m), ns, sz)
    case.upload(case.clean)
    other = torch.zeros(16, dtype=torch.int32, device="cuda:1")
    with pytest.raises(capi.FecError, match="culprit lives on device 1, the blocks on device 0"):
        case.call(capi.Code(k, m), other.data_ptr())


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_two_streams(k, m):
    """Asynchronous calls back to back on two streams: each waits on the GPU
    for the call that used the thread's working words (and scratch) before it,
    and each correction reads its own verdicts."""
    ns, sz = 5, 4097
    code = capi.Code(k, m)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for i in range(6):
        case = Case(k, m, range(m), ns, sz)
        cor = [(i % ns, (2 * i) % m, np.array([(i * 700) % sz]), np.array([1 + i], dtype=np.uint8))]
        if i % 3 == 2:
            cor.append(((i + 1) % ns, 1, np.array([5, 3000]), np.array([7, 9], dtype=np.uint8)))
        want, after = corrected(case.P, case.Q, case.corrupt(cor))
        case.upload(case.corrupt(cor))
        out = torch.full((ns,), -1, dtype=torch.int32, device="cuda")
        runs.append((case, want, after, out))
    torch.cuda.synchronize()
    for i, (case, want, after, out) in enumerate(runs):
        case.call(code, out.data_ptr(), stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, (case, want, after, out) in enumerate(runs):
        assert (out.cpu().numpy().view(np.uint32) == want).all(), i
        assert want[i % ns] == (2 * i) % m
        assert (case.buf.cpu().numpy() == case.lay_in(after)).all(), i
        assert (after == case.clean).all()


def test_declines_under_graph_capture():
    k, m, ns, sz = 3, 10, 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    case.run(code, [one(1, 4, 5, 1)], "outside the capture")
    blocks = case.corrupt([one(1, 4, 5, 1)])
    case.upload(blocks)
    out = torch.zeros(ns, dtype=torch.int32, device="cuda")
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="fec_correct_batch: the stream is being captured into a graph"):
                case.call(code, out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (case.buf.cpu().numpy() == case.lay_in(blocks)).all()


def test_empty_calls():
    """nstripes == 0 touches nothing; sz == 0 answers CLEAN for every stripe
    and writes no block byte."""
    k, m = 3, 10
    code = capi.Code(k, m)
    buf = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((8,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code.correct_batch(buf.data_ptr(), 0, 0, list(range(m)), 16, 0, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == FILL).all()
    code.correct_batch(buf.data_ptr(), 0, 0, list(range(m)), 0, 3, out.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == [FILL] * 2 + [CLEAN] * 3 + [FILL] * 3
    host = np.full(8, FILL, dtype=np.uint32)
    code.correct_batch(buf.data_ptr(), 0, 0, list(range(m)), 0, 3, host.ctypes.data + 8, stream=st)
    assert host.tolist() == [FILL] * 2 + [CLEAN] * 3 + [FILL] * 3
    assert (buf == 0x5A).all()


# ---- deterministic, idempotent -------------------------------------------------------------------

def test_deterministic():
    k, m, ns, sz = 3, 10, 70, 4097
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    cor = patterns(k, m - k, ns, sz, 9)["neighbours"]
    first = case.run(code, cor, "first")[0]
    buf = case.buf.clone()
    assert (case.run(code, cor, "second")[0] == first).all()
    assert torch.equal(case.buf, buf)


@pytest.mark.parametrize("k,m,c", [(3, 10, 7), (3, 10, 2), (3, 10, 1), (10, 16, 6)])
def test_idempotent(k, m, c):
    """A second call on the healed buffer answers CLEAN for every stripe that
    was corrected and the same MANY / UNKNOWN as before elsewhere, and writes
    nothing."""
    ns, sz = 37, 1025
    code = capi.Code(k, m)
    case = Case(k, m, list(range(m))[:k + c], ns, sz)
    cor = []
    for pname, items in patterns(k, c, ns, sz, 21 + c).items():
        if pname != "whole block":
            cor += items
    seen = {}
    for s, j, xs, vs in cor:  # one corruption list per stripe, the first one named
        seen.setdefault(s, []).append((s, j, xs, vs))
    cor = [it for s in sorted(seen) for it in seen[s][:2]]
    first, after = case.run(code, cor, "first")
    again, after2 = case.run(code, None, "second", blocks=after)
    fixed = first < k + c
    assert (again[fixed] == CLEAN).all() and (again[~fixed] == first[~fixed]).all()
    assert (after2 == after).all()
    if c >= 2:
        assert fixed.any() and (first == MANY).any()
    else:
        assert set(first.tolist()) == {CLEAN, UNKNOWN}


# ---- Python API --------------------------------------------------------------------------

def spoiled(k, m, ns, sz, seed):
    """One random block overwritten in a third of ns stripes of a shuffled
    (k, m) layout: (nums, clean, host, bad stripes, their slots)."""
    rng = np.random.default_rng(seed)
    nums = rng.permutation(m).tolist()
    clean = np.ascontiguousarray(stripes(k, m, NSMAX, SZMAX)[:ns][:, nums, :sz])
    host = clean.copy()
    bad = np.sort(rng.permutation(ns)[:ns // 3])
    slot = rng.integers(0, m, size=len(bad))
    for s, j in zip(bad, slot):
        host[s, j] ^= rng.integers(1, 256, size=sz, dtype=np.uint8)
    return nums, clean, host, bad, slot


def test_python_api():
    k, m, ns, sz = 3, 10, 70, 4097
    dec = zfec_amd.Decoder(k, m)
    nums, clean, host, bad, slot = spoiled(k, m, ns, sz, 77)
    want = np.full(ns, zfec_amd.LOCATE_CLEAN, dtype=np.int32)
    want[bad] = slot
    blocks = torch.from_numpy(host).cuda()
    out = dec.correct_batch(blocks, nums)
    assert out.dtype == torch.int32 and tuple(out.shape) == (ns,) and out.device == blocks.device
    assert (out.cpu().numpy() == want).all()
    assert (blocks.cpu().numpy() == clean).all()
    assert not dec.verify_batch(blocks, nums).any()
    assert (dec.correct_batch(blocks, nums) == zfec_amd.LOCATE_CLEAN).all()
    # block-major storage, on a non-default stream
    bm = torch.from_numpy(host).cuda().transpose(0, 1).contiguous().transpose(0, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dec.correct_batch(bm, nums)
    s.synchronize()
    assert (out.cpu().numpy() == want).all() and (bm.cpu().numpy() == clean).all()
    # empty batches
    assert tuple(dec.correct_batch(blocks[:0], nums).shape) == (0,)
    empty = dec.correct_batch(blocks[:, :, :0], nums)
    assert empty.dtype == torch.int32 and empty.tolist() == [zfec_amd.LOCATE_CLEAN] * ns


@pytest.mark.parametrize("k,m,c", [(3, 10, 7), (10, 16, 6)])
def test_equals_the_three_call_recipe(k, m, c):
    """locate_batch -> patterns built with tensor operations -> repair_batch ->
    copy back yields the same bytes as correct_batch, on single errors, on
    several errors (MANY: neither writes) and on clean stripes."""
    ns, sz = 70, 1025
    dec = zfec_amd.Decoder(k, m)
    nums, clean, host, bad, slot = spoiled(k, m, ns, sz, 5 * k + m)
    host[1, 0, 7] ^= 1  # two blocks far apart, and two at one byte
    host[1, m - 1, 900] ^= 2
    host[2, 1, 33] ^= 3
    host[2, k, 33] ^= 4
    dev = torch.device("cuda")
    recipe = torch.from_numpy(host).to(dev)
    verdict = dec.locate_batch(recipe, nums)
    nums_t = torch.tensor(nums, dtype=torch.int64, device=dev)
    v = verdict.to(torch.int64)
    idx = torch.arange(k, device=dev).unsqueeze(0).expand(ns, k)
    idx = idx + (idx >= v.unsqueeze(1)).to(torch.int64) * (v.unsqueeze(1) >= 0)
    present = torch.gather(recipe, 1, idx.unsqueeze(-1).expand(ns, k, sz)).contiguous()
    targets = torch.where(v >= 0, nums_t[v.clamp(min=0)], torch.full_like(v, -1)).unsqueeze(1)
    rebuilt = dec.repair_batch(present, nums_t[idx], targets)
    hit = torch.nonzero(v >= 0).squeeze(1)
    recipe[hit, v[hit]] = rebuilt[hit, 0]
    healed = torch.from_numpy(host).to(dev)
    out = dec.correct_batch(healed, nums)
    assert torch.equal(out, verdict)
    assert torch.equal(healed, recipe)
    alone = ~np.isin(bad, (1, 2))  # stripes 1 and 2 may hold a further error
    assert alone.sum() >= ns // 3 - 2 and (out.cpu().numpy()[bad[alone]] == slot[alone]).all()
    assert out[1].item() == zfec_amd.LOCATE_MANY
