"""GPU checks of the batched parity verification (fec_verify_batch;
zfec_amd/csrc/kernels.hip matverify_reg<K,R> for k <= 4, the expected rows
through the encode kernels plus rows_differ past that).  Shares come from the
CPU oracle's encode; the expected masks are computed in numpy from the matrix
P the oracle builds (tests/verify_ref.py), never from the library.  Inputs
start at byte offset 3.  The mismatch words are pre-filled with 0xA5A5A5A5 and
sit between guard words: after every call the guards are unchanged, the words
are exact (no stray bits), src is byte-identical to what was uploaded, and the
kernel name is the expected one."""
import functools

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle
from verify_ref import gf_matmul, mul_table, oracle_P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5A5A5A5
GW = 4  # guard words before and after the mismatch words
TAIL = 64
IN_OFF = 3

SIZES = (1, 15, 16, 17, 1023, 1024, 1025, 4097)
NS = (1, 3, 70)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


@functools.lru_cache(maxsize=None)
def stripes(k, m, ns, sz):
    """All m blocks of ns stripes (ns, m, sz), read-only.  Output byte x depends
    only on byte x of the inputs, so the oracle encodes the batch as one long
    stripe, and a shorter block or a smaller batch is a prefix of these."""
    rng = np.random.default_rng(1000 * k + 10 * m)
    data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
    flat = np.ascontiguousarray(data.transpose(1, 0, 2)).reshape(k, ns * sz)
    par = oracle.encode(k, m, flat).reshape(m - k, ns, sz).transpose(1, 0, 2)
    allb = np.concatenate([data, par], axis=1)
    allb.setflags(write=False)
    return allb


def bases(k, m, seed):
    """Block numbers of all m slots, the first k the basis: the primaries in
    order, a shuffled all-parity basis (where the code has k parity blocks) and
    a mixed one."""
    rng = np.random.default_rng(seed)
    out = [("primaries", list(range(m)))]
    if m - k >= k:
        par = (k + rng.permutation(m - k)).tolist()
        out.append(("parity", par[:k] + rng.permutation(par[k:] + list(range(k))).tolist()))
    while True:
        mixed = rng.permutation(m).tolist()
        primary = [b < k for b in mixed[:k]]
        if k == 1 or (any(primary) and not all(primary)):
            break
    out.append(("mixed", mixed))
    return out


@functools.lru_cache(maxsize=None)
def check_rows(k, m, nums):
    """The oracle-built P of `nums`, anchored once: it has no zero entry and
    maps the clean basis shares onto the clean check shares."""
    P = oracle_P(k, m, nums)
    assert P.all()
    allb = stripes(k, m, 1, 64)[0]
    assert (gf_matmul(P, allb[list(nums[:k])]) == allb[list(nums[k:])]).all()
    return P


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
        if self.kind == "bm":
            return flat.reshape(self.rows, self.ns, self.ld).transpose(1, 0, 2)
        return flat.reshape(self.ns, self.rows, self.ld)

    def offset(self, s, j, x):
        return IN_OFF + s * self.ss + j * self.bs + x


def expected_bits(P, k, ns, corruptions):
    """(ns, c) bool from the oracle's P: `corruptions` is a list of
    (stripe, slot, byte, xor value).  At every touched byte, check i differs
    iff sum_j P[i][j] * delta(basis j) ^ delta(check i) is nonzero."""
    c = P.shape[0]
    bits = np.zeros((ns, c), dtype=bool)
    if not corruptions:
        return bits
    mul = mul_table()
    pos = sorted({x for _, _, x, _ in corruptions})
    col = {x: t for t, x in enumerate(pos)}
    delta = np.zeros((ns, k + c, len(pos)), dtype=np.uint8)
    for s, j, x, v in corruptions:
        delta[s, j, col[x]] ^= v
    for i in range(c):
        err = delta[:, k + i, :].copy()
        for j in range(k):
            if delta[:, j, :].any():
                err ^= mul[P[i, j]][delta[:, j, :]]
        bits[:, i] = err.any(axis=1)
    return bits


def pack(bits):
    ns, c = bits.shape
    W = (c + 31) // 32
    words = np.zeros((ns, W), dtype=np.uint32)
    for i in range(c):
        words[:, i // 32] |= bits[:, i].astype(np.uint32) << np.uint32(i % 32)
    return words


def patterns(k, c, ns, sz, seed):
    """name -> corruption list: the patterns every shape is checked with."""
    rng = np.random.default_rng(seed)
    s = ns // 2
    slot = lambda: k + int(rng.integers(0, c))  # noqa: E731
    out = {
        "clean": [],
        "check, first byte": [(s, slot(), 0, 0x01)],
        "check, last byte": [(s, slot(), sz - 1, 0x80)],
        "check, byte sz-16": [(s, slot(), max(0, sz - 16), 0x5A)],
        "basis": [(s, int(rng.integers(0, k)), int(rng.integers(0, sz)), 0xFF)],
        "every check": [(t, k + i, int((7 * t + 13 * i) % sz), 1 + (i % 255)) for t in range(ns) for i in range(c)],
    }
    if ns >= 2 and c >= 2:
        a = int(rng.integers(0, ns - 1))
        i0 = int(rng.integers(0, c))
        i1 = (i0 + 1 + int(rng.integers(0, c - 1))) % c
        out["neighbours"] = [(a, k + i0, sz - 1, 0x10), (a + 1, k + i1, 0, 0x20)]
    return out


class Case(object):
    """ns stripes of the blocks `nums` (first k the basis) in one layout, in
    device memory (or page-locked host memory), plus guarded mismatch words."""

    def __init__(self, k, m, nums, ns, sz, kind="padded", src_mem="device", szmax=None, nsmax=None):
        self.k, self.m, self.nums, self.ns, self.sz = k, m, list(nums), ns, sz
        self.nb = len(self.nums)
        self.c = self.nb - k
        self.W = (self.c + 31) // 32
        allb = stripes(k, m, nsmax or ns, szmax or sz)
        self.lay = Layout(kind, ns, self.nb, sz)
        host = np.zeros(IN_OFF + self.lay.nbytes + TAIL, dtype=np.uint8)
        self.lay.view(host[IN_OFF:IN_OFF + self.lay.nbytes])[:, :, :sz] = allb[:ns][:, self.nums, :sz]
        t = torch.from_numpy(host)
        self.src = t.cuda() if src_mem == "device" else t.pin_memory()
        self.orig = self.src.clone()
        self.P = check_rows(k, m, tuple(self.nums))

    def corrupt(self, corruptions):
        self.src.copy_(self.orig)
        if corruptions:
            acc = {}
            for s, j, x, v in corruptions:
                o = self.lay.offset(s, j, x)
                acc[o] = acc.get(o, 0) ^ v
            idx = torch.tensor(list(acc.keys()), dtype=torch.int64, device=self.src.device)
            val = torch.tensor(list(acc.values()), dtype=torch.uint8, device=self.src.device)
            self.src[idx] ^= val

    def run(self, code, corruptions, what, mask_mem="device", stream=None, flags=capi.FEC_FLAG_ASYNC, name=True):
        """Corrupt, verify, check everything; returns the words (ns, W)."""
        self.corrupt(corruptions)
        uploaded = self.src.clone()
        n = self.ns * self.W
        words = np.full(GW + n + GW, FILL, dtype=np.uint32)
        if mask_mem == "device":
            mask = torch.from_numpy(words.view(np.int32)).cuda()
            ptr = mask.data_ptr() + 4 * GW
        elif mask_mem == "pinned":
            mask = torch.from_numpy(words.view(np.int32)).pin_memory()
            ptr = mask.data_ptr() + 4 * GW
        else:
            mask = words
            ptr = words.ctypes.data + 4 * GW
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if flags & capi.FEC_FLAG_LIBRARY_STREAM:
            torch.cuda.synchronize()  # the library's stream does not wait for the upload's
        code.verify_batch(self.src.data_ptr() + IN_OFF, self.lay.bs, self.lay.ss, self.nums, self.sz, self.ns, ptr,
                          stream=st, flags=flags)
        got_name = capi.last_kernel_name()
        torch.cuda.synchronize()
        got = mask if mask_mem == "numpy" else mask.cpu().numpy().view(np.uint32)
        assert (got[:GW] == FILL).all() and (got[GW + n:] == FILL).all(), ("guard words", what)
        got = got[GW:GW + n].reshape(self.ns, self.W)
        want = pack(expected_bits(self.P, self.k, self.ns, corruptions))
        assert (got == want).all(), (what, got_name, np.argwhere(got != want)[:4].tolist())
        assert torch.equal(self.src, uploaded), ("src was written", what)
        if name:
            assert got_name == self.kernel_name(), (what, got_name)
        return got

    def kernel_name(self):
        if self.k <= 4:
            return "matverify_reg<%d,%d>" % (self.k, self.c - 8 * ((self.c - 1) // 8))
        return "rows_differ"


def sweep(k, m, kind, sizes, nss, seed):
    code = capi.Code(k, m)
    for bname, nums in bases(k, m, seed):
        for ns in nss:
            for sz in sizes:
                case = Case(k, m, nums, ns, sz, kind, szmax=max(sizes), nsmax=max(nss))
                for pname, cor in patterns(k, case.c, ns, sz, seed + sz + ns).items():
                    case.run(code, cor, (k, m, kind, bname, ns, sz, pname))


# ---- register path --------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["packed", "padded", "bm"])
@pytest.mark.parametrize("k,m", [(1, 2), (2, 3), (3, 10), (4, 12), (3, 16), (4, 40)])
def test_register_path(k, m, kind):
    """c = 1, 1, 7, 8, 13 (two launches: 8 + 5) and 36 (five launches, W = 2).
    Sizes: the byte tail (1, 15), exact chunks (16, 1024: exactly one wave), the
    overlapped last chunk (17, 1023), one wave plus one unit (1025) and four
    waves plus one unit (4097) per stripe."""
    sweep(k, m, kind, SIZES, NS, seed=100 * k + m)


def test_grid_stride(knobs):
    """Three workgroups (12 waves) walk 37 stripes of 3 waves each: the masks
    equal the uncapped run's.  A step of 12 waves is exactly 4 stripes here
    (gs_w = 0), so the carry of the walk never runs: test_gpu_wave_walk.py
    has the geometries with gs_w != 0."""
    k, m, ns, sz = 3, 10, 37, 2049
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    rng = np.random.default_rng(5)
    cor = [(int(s), int(rng.integers(0, m)), int(rng.integers(0, sz)), 0x40) for s in rng.permutation(ns)[:20]]
    cor += [(36, 9, sz - 1, 1), (0, 3, 0, 1)]
    plain = [case.run(code, c, "uncapped") for c in ([], cor)]
    knobs(ZFEC_HIP_GRID_CAP=3)
    capped = [case.run(code, c, "capped") for c in ([], cor)]
    assert all((a == b).all() for a, b in zip(plain, capped))
    assert plain[1].any()


def test_split_launches(knobs):
    """ZFEC_HIP_LAUNCH_UNITS=1024: 4 KiB stripes go in groups of 4 (the word
    pointer advanced per group), 20000-byte blocks in byte ranges of 16 KiB."""
    knobs(ZFEC_HIP_LAUNCH_UNITS=1024)
    k, m = 3, 10
    code = capi.Code(k, m)
    for ns, sz in ((37, 4096), (5, 20000)):
        case = Case(k, m, range(m), ns, sz)
        for pname, cor in patterns(k, case.c, ns, sz, sz).items():
            case.run(code, cor, (ns, sz, pname))
        case.run(code, [(ns - 1, 9, sz - 1, 1), (ns - 2, 4, 16384 if sz > 16384 else 5, 2)], (ns, sz, "last range"))


# ---- scratch path ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["padded", "bm"])
@pytest.mark.parametrize("k,m", [(10, 16), (20, 60), (33, 36)])
def test_scratch_path(k, m, kind):
    """c = 6, 40 (W = 2) and 3 (k > 32: the wide kernels or accumulating passes
    compute the expected rows)."""
    code = capi.Code(k, m)
    for bname, nums in bases(k, m, seed=k):
        if bname == "parity":  # the primaries and a mixed basis
            continue
        for ns in (1, 5):
            for sz in (17, 4097):
                case = Case(k, m, nums, ns, sz, kind, szmax=4097, nsmax=5)
                for pname, cor in patterns(k, case.c, ns, sz, k + sz + ns).items():
                    case.run(code, cor, (k, m, kind, bname, ns, sz, pname))


def test_scratch_cap_cuts_are_invisible(knobs):
    """A test-only scratch cap of 64 KiB.  K=10/M=16 (6 check rows): 4097-byte
    blocks go in runs of 2 stripes (2 + 2 + 1); 10923-byte blocks are just over
    the cap (6 x 10944 = 65,664 bytes) and go stripe by stripe in byte ranges
    of 10880 and 43 bytes, with corruption placed in the last range."""
    knobs(ZFEC_HIP_VERIFY_SCRATCH=65536)
    k, m = 10, 16
    code = capi.Code(k, m)
    case = Case(k, m, range(m), 5, 4097)
    case.run(code, [], "runs, clean")
    case.run(code, [(4, 12, 4096, 1), (2, 11, 0, 1), (1, 3, 77, 9)], "runs")
    sz = 10923
    case = Case(k, m, range(m), 3, sz)
    for pname, cor in patterns(k, case.c, 3, sz, 1).items():
        case.run(code, cor, ("ranges", pname))
    case.run(code, [(2, 15, sz - 1, 1)], "last byte of the last range")
    case.run(code, [(1, 13, 10880, 4), (0, 10, 10879, 4)], "both sides of the cut")
    case.run(code, [(2, 7, 10900, 0x33)], "basis byte in the last range")


# ---- memory kinds ------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
@pytest.mark.parametrize("mask_mem", ["numpy", "pinned"])
def test_mismatch_in_host_memory(k, m, mask_mem):
    """The words are gathered in device memory the library owns and copied back;
    the call is synchronous whatever the flags."""
    ns, sz = 37, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    for flags in (capi.FEC_FLAG_ASYNC, 0, capi.FEC_FLAG_LIBRARY_STREAM):
        for pname, cor in patterns(k, case.c, ns, sz, 3).items():
            case.run(code, cor, (mask_mem, flags, pname), mask_mem=mask_mem, flags=flags)


@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_src_in_page_locked_host_memory(k, m):
    ns, sz = 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz, src_mem="pinned")
    for mask_mem in ("device", "numpy"):
        for pname, cor in patterns(k, case.c, ns, sz, 4).items():
            case.run(code, cor, (mask_mem, pname), mask_mem=mask_mem, flags=0)


def test_mismatch_on_another_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    k, m, ns, sz = 3, 10, 3, 64
    case = Case(k, m, range(m), ns, sz)
    other = torch.zeros(16, dtype=torch.int32, device="cuda:1")
    with pytest.raises(capi.FecError, match="mismatch lives on device 1, the blocks on device 0"):
        capi.Code(k, m).verify_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns,
                                     other.data_ptr())


def test_empty_calls():
    """nstripes == 0 touches nothing; sz == 0 clears the words."""
    k, m = 3, 10
    code = capi.Code(k, m)
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    mask = torch.full((8,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code.verify_batch(src.data_ptr(), 0, 0, list(range(m)), 16, 0, mask.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert (mask.cpu().numpy().view(np.uint32) == FILL).all()
    code.verify_batch(src.data_ptr(), 0, 0, list(range(m)), 0, 3, mask.data_ptr() + 8, stream=st)
    torch.cuda.synchronize()
    assert mask.cpu().numpy().view(np.uint32).tolist() == [FILL] * 2 + [0] * 3 + [FILL] * 3
    host = np.full(8, FILL, dtype=np.uint32)
    code.verify_batch(src.data_ptr(), 0, 0, list(range(m)), 0, 3, host.ctypes.data + 8, stream=st)
    assert host.tolist() == [FILL] * 2 + [0] * 3 + [FILL] * 3


def test_pageable_src_is_refused():
    k, m = 3, 10
    src = np.zeros(4 * m * 64, dtype=np.uint8)
    mask = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.FecError, match="pageable host memory, which this call does not stage"):
        capi.Code(k, m).verify_batch(src.ctypes.data, 64, m * 64, list(range(m)), 64, 4, mask.data_ptr())


def test_two_streams_share_the_scratch():
    """Asynchronous scratch-path calls back to back on two streams: each waits
    on the GPU for the call that used the thread's scratch before it."""
    k, m, ns, sz = 10, 16, 5, 4097
    code = capi.Code(k, m)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for i in range(6):
        case = Case(k, m, range(m), ns, sz)
        cor = [(i % ns, 10 + i, (i * 700) % sz, 1 + i)]
        case.corrupt(cor)
        mask = torch.full((ns,), -1, dtype=torch.int32, device="cuda")
        runs.append((case, cor, mask))
    torch.cuda.synchronize()
    for i, (case, cor, mask) in enumerate(runs):
        code.verify_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns, mask.data_ptr(),
                          stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, (case, cor, mask) in enumerate(runs):
        want = pack(expected_bits(case.P, k, ns, cor))
        assert (mask.cpu().numpy().view(np.uint32).reshape(ns, 1) == want).all(), i


def test_declines_under_graph_capture():
    k, m, ns, sz = 3, 10, 5, 1025
    code = capi.Code(k, m)
    case = Case(k, m, range(m), ns, sz)
    case.run(code, [(1, 4, 5, 1)], "outside the capture")
    mask = torch.zeros(ns, dtype=torch.int32, device="cuda")
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                code.verify_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns,
                                  mask.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()


# ---- Python API --------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (4, 40), (10, 16)])
def test_python_api(k, m):
    ns, sz = 37, 1025
    dec = zfec_amd.Decoder(k, m)
    rng = np.random.default_rng(m)
    nums = rng.permutation(m).tolist()
    c = m - k
    P = check_rows(k, m, tuple(nums))
    allb = stripes(k, m, ns, sz)
    host = np.ascontiguousarray(allb[:, nums, :])
    cor = [(3, k + c - 1, sz - 1, 1), (4, k, 0, 2), (9, 0, 500, 3), (36, k + c // 2, 17, 4)]
    for s, j, x, v in cor:
        host[s, j, x] ^= v
    want = expected_bits(P, k, ns, cor)
    blocks = torch.from_numpy(host).cuda()
    out = dec.verify_batch(blocks, nums)
    assert out.dtype == torch.bool and tuple(out.shape) == (ns, c) and out.device == blocks.device
    assert (out.cpu().numpy() == want).all()
    assert want[9].all() and want.sum() == c + 3
    # block-major input
    bm = blocks.transpose(0, 1).contiguous().transpose(0, 1)
    assert (dec.verify_batch(bm, nums).cpu().numpy() == want).all()
    # on a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = dec.verify_batch(blocks, nums)
    s.synchronize()
    assert (out.cpu().numpy() == want).all()
    # a clean batch, and empty ones
    clean = torch.from_numpy(np.ascontiguousarray(allb[:, nums, :])).cuda()
    assert not dec.verify_batch(clean, nums).any()
    assert tuple(dec.verify_batch(clean[:0], nums).shape) == (0, c)
    assert tuple(dec.verify_batch(clean[:, :, :0], nums).shape) == (ns, c)
    assert torch.equal(blocks.cpu(), torch.from_numpy(host))
