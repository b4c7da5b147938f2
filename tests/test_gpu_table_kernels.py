"""GPU parity of the v_perm table kernels (zfec_amd/csrc/kernels.hip):
matapply_reg, matapply_rows, matapply_pair and matapply_lds (matapply_small in
the coefficient sweep).  Bit-exact against the CPU oracle (zfec/fec.c:487-505
encode, :527-557 decode) with the launched kernel's name asserted after every
launch:

* every matapply_reg<K,R> and matapply_rows<K,R> instantiation (K = 1..4,
  R = 1..8) in every form a shape has: both store policies, batches, decodes;
* every non-null entry of the paired launch table (70 matapply_pair shapes);
* every nonzero coefficient table through each family;
* every matapply_lds tile height, the few-input and the accumulating variant;
* the grid-stride walk of all of them, reached with ZFEC_HIP_GRID_CAP.

Outputs are pre-filled with 0xA5; the bytes before, between and after the rows
must come back unchanged."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
TAIL = 64


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


@pytest.fixture
def jit_off():
    prev = capi.jit_mode(capi.JIT_OFF)
    yield
    capi.jit_mode(prev)


@pytest.fixture
def lds_only(knobs):
    """JIT off, generic mode 0 (no bit-sliced kernels), matapply_small off:
    shapes past the register kernels run on matapply_lds."""
    prev_j, prev_g = capi.jit_mode(capi.JIT_OFF), capi.generic_mode(0)
    knobs(ZFEC_HIP_SMALL_LANES=0)
    yield
    capi.jit_mode(prev_j)
    capi.generic_mode(prev_g)


def place(nums, k):
    """slot order with primary i at slot i (zfec/_fecmodule.c:482-493)."""
    slots = [None] * k
    sec = iter([n for n in nums if n >= k])
    for n in nums:
        if n < k:
            slots[n] = n
    return [s if s is not None else next(sec) for s in slots]


def flat(blocks):
    """(ns, rows, sz) -> (rows, ns * sz): output byte x depends only on byte x
    of the inputs, so the oracle takes a batch as one long stripe."""
    ns, rows, sz = blocks.shape
    return np.ascontiguousarray(blocks.transpose(1, 0, 2)).reshape(rows, ns * sz)


def unflat(rows2d, ns):
    rows, n = rows2d.shape
    return np.ascontiguousarray(rows2d.reshape(rows, ns, n // ns).transpose(1, 0, 2))


def enc_expect(k, m, data, nums):
    return unflat(oracle.encode(k, m, flat(data), list(nums)), data.shape[0])


def dec_case(k, m, data, recv_nums):
    """Received blocks in slot order, the slots, and the oracle's decode of
    them (which must be the lost primaries)."""
    slots = place(sorted(recv_nums), k)
    missing = [i for i in range(k) if slots[i] >= k]
    f = flat(data)
    allb = np.concatenate([f, oracle.encode(k, m, f)])
    recv = np.ascontiguousarray(allb[slots])
    want = oracle.decode(k, m, recv, slots)
    assert (want == f[missing]).all()
    ns = data.shape[0]
    return unflat(recv, ns), slots, unflat(want, ns)


def covering_block(rng, k, sz):
    """(k, sz) random bytes, sz >= 1024, whose first 1024 bytes hold every byte
    value at every byte position of a dword, in every block: each entry of a
    coefficient's table is read from each byte lane."""
    assert sz >= 1024
    data = rng.integers(0, 256, size=(k, sz), dtype=np.uint8)
    for j in range(k):
        for b in range(4):
            data[j, 256 * b:256 * (b + 1)] = np.roll(np.arange(256, dtype=np.uint8), b + 17 * j)
    return data


class Job(object):
    """One encode ("enc") or decode ("dec") over device buffers laid out
    [stripe][block][ld], `blocks` (ns, k, sz) being the kernel's inputs (for a
    decode: the received blocks in slot order) and `index` the block numbers
    (for a decode: of the slots).  The output holds r rows per stripe."""

    def __init__(self, code, op, index, blocks, r, ld, in_off=3, out_off=5):
        self.code, self.op, self.index, self.r, self.ld = code, op, [int(x) for x in index], r, ld
        self.ns, self.k, self.sz = blocks.shape
        assert ld >= self.sz
        self.out_off = out_off
        src = torch.zeros(in_off + self.ns * self.k * ld + TAIL, dtype=torch.uint8, device="cuda")
        src[in_off:in_off + self.ns * self.k * ld].view(self.ns, self.k, ld)[:, :, :self.sz] = \
            torch.from_numpy(np.ascontiguousarray(blocks)).cuda()
        self.src = src
        self.dst = torch.full((out_off + self.ns * r * ld + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
        self.sp, self.dp = src.data_ptr() + in_off, self.dst.data_ptr() + out_off

    def launch(self):
        """One stripe through the pointer-array entry point, several through
        the batched one; returns the kernel's name."""
        st = torch.cuda.current_stream().cuda_stream
        ld = self.ld
        if self.ns == 1:
            f = self.code.encode_ptrs if self.op == "enc" else self.code.decode_ptrs
            f([self.sp + j * ld for j in range(self.k)], [self.dp + i * ld for i in range(self.r)], self.index,
              self.sz, stream=st)
        else:
            f = self.code.encode_batch if self.op == "enc" else self.code.decode_batch
            f(self.sp, ld, self.k * ld, self.dp, ld, self.r * ld, self.index, self.sz, self.ns, stream=st)
        return capi.last_kernel_name()

    def as_batch_job(self):
        f = capi.encode_job if self.op == "enc" else capi.decode_job
        return f(self.code, self.sp, self.ld, self.k * self.ld, self.dp, self.ld, self.r * self.ld, self.index,
                 self.sz, self.ns)

    def result(self, what=""):
        """The output rows (ns, r, sz) and the whole output buffer, once the
        bytes around the rows have been found untouched."""
        torch.cuda.synchronize()
        host = self.dst.cpu().numpy()
        n = self.ns * self.r * self.ld
        assert (host[:self.out_off] == GUARD).all(), ("write before the output", what)
        assert (host[self.out_off + n:] == GUARD).all(), ("write after the output", what)
        body = host[self.out_off:self.out_off + n].reshape(self.ns, self.r, self.ld)
        assert (body[:, :, self.sz:] == GUARD).all(), ("write past a row", what)
        return body[:, :, :self.sz], host


def run_one(code, op, index, blocks, want, ld, in_off=3, out_off=5, name=None):
    """Launch, check the name, the guards and the bytes; returns the whole
    output buffer."""
    job = Job(code, op, index, blocks, want.shape[1], ld, in_off, out_off)
    got_name = job.launch()
    what = (op, job.k, job.r, job.sz, job.ns, ld, out_off, got_name)
    got, host = job.result(what)
    assert got_name == name, what
    assert (got == want).all(), what
    return host


def run_pair(ja, jb):
    capi.run_batch_jobs([ja.as_batch_job(), jb.as_batch_job()], stream=torch.cuda.current_stream().cuda_stream)
    return capi.last_kernel_name()


def row16(sz):
    """A row stride that keeps every row of a stripe on the alignment of the first."""
    return (sz + 15) // 16 * 16 + 16


# ---- 1. every register-kernel shape ----------------------------------------------

REG_SIZES = (1, 15, 16, 17, 31, 4095, 4096, 4097, 8192 + 9)
BIG_STRIPE = (1 << 18) + 5  # 65 workgroups
ROWS_NS = (64, 65, 67)
ROWS_SIZES = (1025, 1040, 2047, 2048, 2049, 3073, 4095, 4096)


@pytest.mark.parametrize("K,R", [(K, R) for K in range(1, 5) for R in range(1, 9)])
def test_reg_every_shape(jit_off, K, R):
    """matapply_reg<K,R> and matapply_rows<K,R> of the K/(K+8) code's first R
    parity rows, and for R <= K the decode of R lost primaries (the same
    instantiations with another matrix).

    matapply_reg: a single stripe with 16-byte aligned rows (stored nt sc1),
    the same stripe with every row at 6 (mod 16) (stored nt) and a batch of 5
    stripes with rows sz + 24 apart, at sizes around the 16-byte chunk, the
    overlapping last chunk and the 256-lane workgroup, plus one stripe of 65
    workgroups.  Device-pointer launches of these shapes run matapply_reg at
    every size, also below one chunk (kernels.hip launch_apply: the register
    shapes skip matapply_small and the bit-sliced kernels; matapply_one serves
    host memory only), so the name is asserted from 1 byte up.

    matapply_rows: 1 KiB < sz <= 4 KiB from 64 stripes up -- whole and partial
    workgroups of 4 waves, sizes on both sides of each 1 KiB piece a lane owns;
    63 stripes, 1024 and 4097 bytes fall back to matapply_reg."""
    m = K + 8
    code = capi.Code(K, m)
    nums = list(range(K, K + R))
    reg, rows = "matapply_reg<%d,%d>" % (K, R), "matapply_rows<%d,%d>" % (K, R)
    rng = np.random.default_rng(K * 100 + R)
    if R <= K:
        recv = list(range(R, K)) + list(range(m - R, m))  # primaries 0..R-1 lost, the last R parity blocks received

    def both(data, ld, in_off, out_off, name):
        run_one(code, "enc", nums, data, enc_expect(K, m, data, nums), ld, in_off, out_off, name)
        if R <= K:
            blocks, slots, want = dec_case(K, m, data, recv)
            run_one(code, "dec", slots, blocks, want, ld, in_off, out_off, name)

    for sz in REG_SIZES + (BIG_STRIPE,):
        data = rng.integers(0, 256, size=(1, K, sz), dtype=np.uint8)
        both(data, row16(sz), 0, 32, reg)
        if sz == BIG_STRIPE:
            continue
        both(data, row16(sz), 3, 32 + 6, reg)
        both(rng.integers(0, 256, size=(5, K, sz), dtype=np.uint8), sz + 24, 3, 5, reg)
    for ns in ROWS_NS:
        for sz in ROWS_SIZES:
            both(rng.integers(0, 256, size=(ns, K, sz), dtype=np.uint8), sz + 24, 3, 5, rows)
    for ns, sz in ((63, 2048), (64, 1024), (64, 4097)):
        both(rng.integers(0, 256, size=(ns, K, sz), dtype=np.uint8), sz + 24, 3, 5, reg)


# ---- 2. every paired launch --------------------------------------------------------

@pytest.mark.parametrize("K", range(1, 5))
def test_pair_every_shape(jit_off, K):
    """Every non-null entry of kernels.hip g_pair_launch for this K (RA = 1..8,
    RB <= min(RA, K); 70 in all): an encode of the first RA parity rows of the
    K/(K+8) code and a decode of RB lost primaries as two jobs of one
    fec_run_batch_jobs call, 2 stripes of 4097 bytes at an odd stride.  The two
    jobs have different matrices, data and buffers, so a job reading the
    other's tables or pointers fails.  RA = 8 with RB = K also runs with one
    stripe per job (the nt sc1 store variant)."""
    m = K + 8
    code = capi.Code(K, m)
    rng = np.random.default_rng(7000 + K)
    seen = set()
    for RA in range(1, 9):
        for RB in range(1, min(RA, K) + 1):
            forms = [(2, 4097, 4097 + 24, 5)]
            if (RA, RB) == (8, K):
                forms.append((1, 4097, row16(4097), 32))
            for ns, sz, ld, off in forms:
                nums = list(range(K, K + RA))
                da = rng.integers(0, 256, size=(ns, K, sz), dtype=np.uint8)
                db = rng.integers(0, 256, size=(ns, K, sz), dtype=np.uint8)
                recv = list(range(RB, K)) + list(range(m - RB, m))
                blocks, slots, want_b = dec_case(K, m, db, recv)
                ja = Job(code, "enc", nums, da, RA, ld, 3, off)
                jb = Job(code, "dec", slots, blocks, RB, ld, 3, off)
                name = run_pair(ja, jb)
                what = (K, RA, RB, ns, name)
                got_a, _ = ja.result(what)
                got_b, _ = jb.result(what)
                assert name == "matapply_pair<%d,%d,%d>" % (K, RA, RB), what
                assert (got_a == enc_expect(K, m, da, nums)).all(), what
                assert (got_b == want_b).all(), what
                seen.add(name)
    assert len(seen) == sum(min(RA, K) for RA in range(1, 9))


# ---- 3. every coefficient table ----------------------------------------------------

@pytest.mark.parametrize("family", ["reg", "rows", "lds", "small"])
def test_table_every_coefficient(knobs, jit_off, family):
    """Every nonzero coefficient's table (kernels.hip make_bank: kHostBank in
    the register kernels' arguments, g_bank on the device) through each kernel
    family.  The parity rows of the 2/256 code hold every value 2..255 in each
    column; value 1 comes from a k = 1 code, whose parity rows are [1].  The
    inputs hold every byte value at every byte position of a dword.  The set of
    coefficients launched is built from the oracle's matrices and must contain
    1..255.

    Coefficient 0 is not covered: no encode row of these codes holds one, and
    the decode rows of lost primaries hold none either (every square submatrix
    of the parity rows is invertible, so no cofactor is 0; the oracle's decode
    matrices of 400 erasure patterns of the k <= 4 codes confirm it)."""
    prev_g = capi.generic_mode()
    try:
        if family == "lds":
            capi.generic_mode(0)
            knobs(ZFEC_HIP_SMALL_LANES=0)
        rng = np.random.default_rng(255)
        covered = set()
        c2 = capi.Code(2, 256)
        enc2 = oracle.enc_matrix(2, 256)
        if family in ("reg", "rows"):
            ns, sz = (3, 1031) if family == "reg" else (64, 1031)
            name = "matapply_" + family + "<%d,8>"
            c1, enc1 = capi.Code(1, 9), oracle.enc_matrix(1, 9)
            # 32 launches of 8 consecutive rows (the last one overlaps its neighbour)
            launches = [(c2, 2, 256, enc2, list(range(b, b + 8))) for b in list(range(2, 248, 8)) + [248]]
            launches.append((c1, 1, 9, enc1, list(range(1, 9))))
        else:
            ns, sz = 1, 1031
            name = "matapply_lds<8,4,4>" if family == "lds" else "matapply_small"
            c1, enc1 = capi.Code(1, 10), oracle.enc_matrix(1, 10)
            # all 254 rows in one call: row groups of <= 48 (fec_abi.cpp apply_matrix_range)
            launches = [(c2, 2, 256, enc2, list(range(2, 256))), (c1, 1, 10, enc1, list(range(1, 10)))]
        for code, k, m, enc, nums in launches:
            data = np.stack([covering_block(rng, k, sz) for _ in range(ns)])
            want = enc_expect(k, m, data, nums)
            run_one(code, "enc", nums, data, want, sz + 24, 3, 5, name % k if family in ("reg", "rows") else name)
            covered |= set(int(v) for v in enc[nums].ravel())
        assert covered >= set(range(1, 256)), sorted(set(range(1, 256)) - covered)
    finally:
        capi.generic_mode(prev_g)


# ---- 4. every matapply_lds tile height ---------------------------------------------

def lds_name(k, r, acc=False):
    """kernels.hip pick_lds / fill_pad."""
    if acc:
        return "matapply_lds<16,2,2,acc>"
    if k <= 4:
        return "matapply_lds<8,4,4>"
    tiles = -(-r // 20)
    rt = -(-r // tiles)
    return "matapply_lds<%d,2,%d,pad>" % (rt, 4 if rt <= 4 or rt == 8 else 2)


LDS_SHAPES = [(5, r) for r in range(1, 21)] + [(5, 21), (5, 33), (5, 40), (2, 12), (40, 3)]


@pytest.mark.parametrize("k,r", LDS_SHAPES)
def test_lds_every_tile_height(lds_only, k, r):
    """matapply_lds by tile height: k = 5 with r = 1..20 rows is one padded
    tile of r rows (input groups of 4 for r <= 4 and r = 8, else 2); 21, 33 and
    40 rows split into two near-equal tiles (11, 17, 20); k = 2 with 12 rows
    runs the few-input variant in ragged 8-row tiles; k = 40 runs 32 inputs in
    a first pass and the other 8 in the accumulating pass, whose ragged ends
    are byte-wise (an XOR into the output cannot overlap its neighbour).
    Sizes around the 8-byte unit and the row end, one stripe and three at an
    odd stride."""
    m = k + r
    code = capi.Code(k, m)
    nums = list(range(k, m))
    name = lds_name(k, r, acc=k > 32)
    if k == 5:
        assert name.startswith("matapply_lds<%d,2," % (r if r <= 20 else {21: 11, 33: 17, 40: 20}[r])), name
    rng = np.random.default_rng(k * 1000 + r)
    for sz in (1, 7, 8, 9, 2047, 2049):
        for ns, ld, in_off, out_off in ((1, row16(sz), 0, 32), (3, sz + 24, 3, 5)):
            data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
            run_one(code, "enc", nums, data, enc_expect(k, m, data, nums), ld, in_off, out_off, name)


# ---- 5. the grid-stride walk -------------------------------------------------------

# (sz, stripes) with the grid capped at 3 workgroups = 768 lanes.  16-byte
# chunks per stripe (cps) of the register kernels: 7 (768 = 109 * 7 + 5: the
# walk's chunk step gs_c = 5 carries into the stripe index), 1, 1 (every unit a
# byte-wise tail), 5001 (gs_s = 0; the walk ends in the shifted-back last
# chunk), the same across stripes.
WALK_SHAPES = [(100, 1000), (16, 5000), (9, 3000), (16 * 5000 + 5, 1), (16 * 5000 + 5, 3)]
WALK_KERNELS = ["reg<3,7>", "reg<1,6>", "reg<3,3>", "pair<3,7,3>", "rows<3,7>", "lds<7,2,2,pad>", "lds<16,2,2,acc>"]


def walk_calls(kernel):
    """Run the kernel's shapes; every stripe against the oracle.  Returns the
    whole output buffers."""
    outs = []
    rng = np.random.default_rng(768)
    if kernel.startswith("lds"):
        k, r = (5, 7) if kernel.endswith("pad>") else (40, 3)
        m = k + r
        code = capi.Code(k, m)
        for sz, ns in WALK_SHAPES:
            data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
            nums = list(range(k, m))
            outs.append(run_one(code, "enc", nums, data, enc_expect(k, m, data, nums), sz + 24, 3, 5,
                                "matapply_" + kernel))
        return outs
    if kernel == "rows<3,7>":
        # 12 waves: 25 stripes each
        code = capi.Code(3, 11)
        data = rng.integers(0, 256, size=(300, 3, 1366), dtype=np.uint8)
        nums = list(range(3, 10))
        return [run_one(code, "enc", nums, data, enc_expect(3, 11, data, nums), 1366 + 24, 3, 5, "matapply_rows<3,7>")]
    K, R = {"reg<3,7>": (3, 7), "reg<1,6>": (1, 6), "reg<3,3>": (3, 3), "pair<3,7,3>": (3, 7)}[kernel]
    m = K + 8
    code = capi.Code(K, m)
    nums = list(range(K, K + R))
    for sz, ns in WALK_SHAPES:
        data = rng.integers(0, 256, size=(ns, K, sz), dtype=np.uint8)
        want = enc_expect(K, m, data, nums)
        if kernel.startswith("reg"):
            outs.append(run_one(code, "enc", nums, data, want, sz + 24, 3, 5, "matapply_" + kernel))
            continue
        db = rng.integers(0, 256, size=(ns, K, sz), dtype=np.uint8)
        blocks, slots, want_b = dec_case(K, m, db, list(range(m - K, m)))
        ja = Job(code, "enc", nums, data, R, sz + 24, 3, 5)
        jb = Job(code, "dec", slots, blocks, K, sz + 24, 3, 5)
        name = run_pair(ja, jb)
        got_a, host_a = ja.result((kernel, sz, ns))
        got_b, host_b = jb.result((kernel, sz, ns))
        assert name == "matapply_" + kernel, (name, sz, ns)
        assert (got_a == want).all(), ("encode job", sz, ns)
        assert (got_b == want_b).all(), ("decode job", sz, ns)
        outs += [host_a, host_b]
    return outs


@pytest.mark.parametrize("kernel", WALK_KERNELS)
def test_grid_stride_walk(knobs, jit_off, kernel):
    """ZFEC_HIP_GRID_CAP=3: every launch is 3 workgroups (the pair: 3 per
    job), so each lane walks several units grid-stride -- UnitIter::next with
    its carry, the prefetching walk (<3,7> with the tables read from the
    argument segment, <1,6> with the tables in registers) stepping from body
    chunks into the shifted-back last chunk and into byte-wise tails, the plain
    walk (<3,3>), the second job of a pair at its argument offset,
    matapply_rows' wave stride and matapply_lds' walk (a padded tile, and the
    two passes of a 40-input code).  Every stripe is checked against the
    oracle, and the same calls without the hook must give the same bytes,
    guard bytes included."""
    prev_g = capi.generic_mode()
    try:
        if kernel.startswith("lds"):
            capi.generic_mode(0)
            knobs(ZFEC_HIP_SMALL_LANES=0)
        plain = walk_calls(kernel)
        knobs(ZFEC_HIP_GRID_CAP=3)
        capped = walk_calls(kernel)
        assert len(plain) == len(capped)
        for i, (a, b) in enumerate(zip(plain, capped)):
            assert a.shape == b.shape and (a == b).all(), (kernel, i)
    finally:
        capi.generic_mode(prev_g)
