"""GPU parity of matapply_bsg, the bit-sliced kernel that takes the
coefficient matrix as run-time data (zfec_amd/csrc/kernels.hip): it serves
every wide-code launch no compiled JIT kernel serves -- above all decodes of an
erasure pattern seen for the first time (zfec/fec.c:527-557 decodes every
pattern with one code path).  Bit-exact against the CPU oracle across code
shapes (rows not a multiple of 4, k up to 32), block sizes around the 4 KiB
unit and its overlapping last unit, batched strided stripes at misaligned
bases with guard bytes, and random erasure patterns; and codes of more than 32
inputs in one pass, their block pointers and coefficients read from a
device-side table (the reference takes any 1 <= k <= m <= 256,
zfec/fec.c:437-440; its own benchmark times 94/100, benchmark-zfec/Main.hs:17).

launch_bsg shrinks the rows per wave of a launch with little work, so the small
shapes above all run matapply_bsg<2,2...> (<1,2...> for r <= 4).  Every
rows-per-wave instantiation, RT = 1, 2, 3, 4, 5, 6, 8, 10, 12 in the arguments
form and the table form, is launched by name by test_bsg_every_instantiation,
whose batches have the >= 4 x CUs units that keep a large RT; bsg_name mirrors
the launcher's choice, and every test asserts the exact name.  The grid-stride
walk with its carry and its prefetch across units runs under
ZFEC_HIP_GRID_CAP, and every coefficient 1..255 goes through the offset bank."""

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle
from guarded_batch import Batch, check_rows, encode_case, walk_steps

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


@pytest.fixture
def bsg_only(knobs):
    """JIT off, generic kernel on, matapply_small off (these small launches
    would take it)."""
    prev_j, prev_g = capi.jit_mode(capi.JIT_OFF), capi.generic_mode(1)
    knobs(ZFEC_HIP_SMALL_LANES=0)
    yield
    capi.jit_mode(prev_j)
    capi.generic_mode(prev_g)


def place(nums, k):
    slots = [None] * k
    sec = iter([n for n in nums if n >= k])
    for n in nums:
        if n < k:
            slots[n] = n
    return [s if s is not None else next(sec) for s in slots]


BSG_RT = (1, 2, 3, 4, 5, 6, 8, 10, 12)
CHUNK = 4096  # bytes of each block per unit (kernels.hip kBsgChunk)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def bsg_groups(r, rt):
    return -(-r // (4 * rt))


def bsg_name(k, r, units, ncu):
    """kernels.hip launch_bsg: the smallest instantiated RT >= ceil(r / 4); a
    launch of fewer than 4 x CUs (unit, row group) pairs steps down to smaller
    row groups, not below RT 2.  Pointers and coefficients come from a
    device-side table when there is more than one row group, past 32 inputs and
    past 48 rows; else from the kernel arguments."""
    ri = 0
    while ri + 1 < len(BSG_RT) and BSG_RT[ri] < -(-r // 4):
        ri += 1
    while ri > 1 and units * bsg_groups(r, BSG_RT[ri]) < 4 * ncu:
        ri -= 1
    tbl = bsg_groups(r, BSG_RT[ri]) > 1 or k > 32 or r > 48
    return "matapply_bsg<%d,2%s>" % (BSG_RT[ri], ",tbl" if tbl else "")


def units_of(sz, ns=1):
    return ns * -(-sz // CHUNK)


# (k, m), k * (m - k) >= 24: ceil((m - k) / 4) covers 1..12, but at one to three units per launch
# the launcher steps every one of them down to RT 2 (RT 1 for r <= 4), most in the table form
SHAPES = [(7, 11), (6, 12), (6, 13), (10, 16), (4, 16), (5, 20), (7, 24), (20, 40), (8, 31), (6, 37), (20, 60),
          (32, 70), (12, 60)]


@pytest.mark.parametrize("k,m", SHAPES)
def test_bsg_encode_decode_vs_oracle(bsg_only, k, m):
    rng = np.random.default_rng(k * 100 + m)
    for sz in (4096, 4097, 9000):
        data = rng.integers(0, 256, size=(k, sz), dtype=np.uint8)
        ins = [torch.from_numpy(data[i]).cuda() for i in range(k)]
        out = zfec_amd.Encoder(k, m).encode(ins)
        torch.cuda.synchronize()
        assert capi.last_kernel_name() == bsg_name(k, m - k, units_of(sz), cus()), capi.last_kernel_name()
        par = torch.stack(out[k:]).cpu().numpy()
        assert (par == oracle.encode(k, m, data)).all(), (k, m, sz)
        nums = sorted(int(x) for x in rng.choice(m, size=k, replace=False))
        if all(n < k for n in nums):
            nums = list(range(m - k, m))
        dec = zfec_amd.Decoder(k, m).decode([out[n] for n in nums], nums)
        assert (torch.stack(dec).cpu().numpy() == data).all(), (k, m, sz, nums)


@pytest.mark.parametrize("k,m,sz,ns", [(10, 16, 5000, 9), (20, 60, 52429, 7), (6, 13, 4096, 33), (32, 40, 12345, 3)])
def test_bsg_batched_strided_misaligned(bsg_only, k, m, sz, ns):
    """Batched stripes at odd strides and misaligned bases: every stripe
    against the oracle; bytes between rows and after the last one stay 0xA5."""
    r = m - k
    rng = np.random.default_rng(sz + ns)
    data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
    ld = sz + 24
    base_in, base_out = 3, 5
    src = torch.zeros(base_in + ns * k * ld, dtype=torch.uint8, device="cuda")
    view = src[base_in:].view(ns, k, ld)
    view[:, :, :sz] = torch.from_numpy(data).cuda()
    dst = torch.full((base_out + ns * r * ld + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    code = capi.Code(k, m)
    st = torch.cuda.current_stream().cuda_stream
    code.encode_batch(src.data_ptr() + base_in, ld, k * ld, dst.data_ptr() + base_out, ld, r * ld,
                      list(range(k, m)), sz, ns, stream=st)
    torch.cuda.synchronize()
    assert capi.last_kernel_name() == bsg_name(k, r, units_of(sz, ns), cus()), capi.last_kernel_name()
    d = dst.cpu().numpy()
    assert (d[:base_out] == 0xA5).all() and (d[base_out + ns * r * ld:] == 0xA5).all()
    out = d[base_out:base_out + ns * r * ld].reshape(ns, r, ld)
    assert (out[:, :, sz:] == 0xA5).all(), "write past a row"
    for s in range(ns):
        assert (out[s, :, :sz] == oracle.encode(k, m, data[s])).all(), s


def test_bsg_fresh_erasure_patterns(bsg_only):
    """cfg4's code, 20 random erasure patterns, each decoded once (no JIT kernel
    exists for any of them): recovered blocks equal the inputs and the oracle."""
    k, m, sz, ns = 20, 60, 52429, 16
    ld = (sz + 255) // 256 * 256
    g = torch.Generator(device="cuda").manual_seed(20)
    data = torch.randint(0, 256, (ns, k, ld), dtype=torch.uint8, device="cuda", generator=g)
    par = torch.zeros((ns, m - k, ld), dtype=torch.uint8, device="cuda")
    code = capi.Code(k, m)
    st = torch.cuda.current_stream().cuda_stream
    code.encode_batch(data.data_ptr(), ld, k * ld, par.data_ptr(), ld, (m - k) * ld, list(range(k, m)), sz, ns,
                      stream=st)
    allb = torch.cat([data, par], dim=1)
    rng = np.random.default_rng(60)
    for p in range(20):
        nums = sorted(int(x) for x in rng.choice(m, size=k, replace=False))
        sl = place(nums, k)
        miss = [i for i in range(k) if sl[i] >= k]
        if not miss:
            continue
        rv = allb[:, sl, :].contiguous()
        rec = torch.zeros((ns, len(miss), ld), dtype=torch.uint8, device="cuda")
        code.decode_batch(rv.data_ptr(), ld, k * ld, rec.data_ptr(), ld, len(miss) * ld, sl, sz, ns, stream=st)
        torch.cuda.synchronize()
        if len(miss) * k >= 24:
            assert capi.last_kernel_name() == bsg_name(k, len(miss), units_of(sz, ns), cus()), capi.last_kernel_name()
        assert bool(torch.equal(rec[:, :, :sz], data[:, miss, :sz])), nums
        s = int(rng.integers(0, ns))
        want = oracle.decode(k, m, rv[s, :, :sz].cpu().numpy(), sl)
        assert (rec[s, :, :sz].cpu().numpy() == want).all(), nums


def test_bsg_off_gives_identical_bytes():
    """generic mode off: the table kernels serve the same launch, same bytes."""
    k, m, sz = 20, 60, 70000  # 8750 eight-byte units: past matapply_small's threshold
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, size=(k, sz), dtype=np.uint8)
    ins = [torch.from_numpy(data[i]).cuda() for i in range(k)]
    prev_j = capi.jit_mode(capi.JIT_OFF)
    try:
        outs = {}
        for gen in (1, 0):
            prev = capi.generic_mode(gen)
            try:
                outs[gen] = torch.stack(zfec_amd.Encoder(k, m).encode(ins)[k:])
                torch.cuda.synchronize()
                if gen:
                    assert capi.last_kernel_name() == bsg_name(k, m - k, units_of(sz), cus()), capi.last_kernel_name()
                else:
                    assert capi.last_kernel_name().startswith("matapply_lds")
            finally:
                capi.generic_mode(prev)
    finally:
        capi.jit_mode(prev_j)
    assert torch.equal(outs[0], outs[1])


# k > 32: one pass with the device-side table (r <= 48 per launch; wider r in
# near-equal row groups), instead of XOR-accumulating passes of 32 inputs
WIDE_SHAPES = [(33, 41), (47, 60), (94, 100), (64, 112), (128, 150), (200, 256), (255, 256)]


@pytest.mark.parametrize("k,m", WIDE_SHAPES)
def test_bsg_wide_k_vs_oracle(bsg_only, k, m):
    rng = np.random.default_rng(k * 1000 + m)
    for sz in (4096, 6001):
        data = rng.integers(0, 256, size=(k, sz), dtype=np.uint8)
        ins = [torch.from_numpy(data[i]).cuda() for i in range(k)]
        out = zfec_amd.Encoder(k, m).encode(ins)
        torch.cuda.synchronize()
        want = bsg_name(k, m - k, units_of(sz), cus())
        assert capi.last_kernel_name() == want and want.endswith(",tbl>"), capi.last_kernel_name()
        par = torch.stack(out[k:]).cpu().numpy()
        assert (par == oracle.encode(k, m, data)).all(), (k, m, sz)
        # decode from a random k of the m blocks
        nums = sorted(int(x) for x in rng.choice(m, size=k, replace=False))
        dec = zfec_amd.Decoder(k, m).decode([out[n] for n in nums], nums)
        assert (torch.stack(dec).cpu().numpy() == data).all(), (k, m, sz, nums)


def test_bsg_wide_k_batched_guards(bsg_only):
    """94/100 over strided stripes at misaligned bases: every stripe against the
    oracle, bytes between rows and around the buffer untouched; the same batch
    again with the generic kernel off (XOR-accumulating table passes) gives the
    same bytes."""
    k, m, sz, ns = 94, 100, 5000, 5
    r = m - k
    rng = np.random.default_rng(94)
    data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
    ld = sz + 40
    src = torch.zeros(7 + ns * k * ld, dtype=torch.uint8, device="cuda")
    src[7:].view(ns, k, ld)[:, :, :sz] = torch.from_numpy(data).cuda()
    outs = []
    for gen in (1, 0):
        capi.generic_mode(gen)
        dst = torch.full((9 + ns * r * ld + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        code = capi.Code(k, m)
        code.encode_batch(src.data_ptr() + 7, ld, k * ld, dst.data_ptr() + 9, ld, r * ld, list(range(k, m)), sz, ns,
                          stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if gen:
            assert capi.last_kernel_name() == bsg_name(k, r, units_of(sz, ns), cus()), capi.last_kernel_name()
        else:
            assert capi.last_kernel_name().startswith("matapply_lds"), capi.last_kernel_name()
        outs.append(dst.cpu().numpy())
    capi.generic_mode(1)
    assert np.array_equal(outs[0], outs[1])
    d = outs[0]
    assert (d[:9] == 0xA5).all() and (d[9 + ns * r * ld:] == 0xA5).all()
    o = d[9:9 + ns * r * ld].reshape(ns, r, ld)
    assert (o[:, :, sz:] == 0xA5).all(), "write past a row"
    for s_ in range(ns):
        assert (o[s_, :, :sz] == oracle.encode(k, m, data[s_])).all(), s_


def test_bsg_wide_k_table_ring_reuse(bsg_only):
    """More wide launches than the table ring has slots, queued back to back on
    one stream with different matrices (every decode pattern a new one): each
    launch must read its own table, so every result is checked."""
    k, m, sz = 40, 60, 8192
    rng = np.random.default_rng(40)
    data = rng.integers(0, 256, size=(k, sz), dtype=np.uint8)
    ins = [torch.from_numpy(data[i]).cuda() for i in range(k)]
    allb = zfec_amd.Encoder(k, m).encode(ins)
    dec = zfec_amd.Decoder(k, m)
    results = []
    for _ in range(20):  # 20 > 8 ring slots
        nums = sorted(int(x) for x in rng.choice(m, size=k, replace=False))
        results.append((nums, dec.decode([allb[n] for n in nums], nums)))
    torch.cuda.synchronize()
    for nums, got in results:
        assert (torch.stack(got).cpu().numpy() == data).all(), nums


# ---- the grid-stride walk, under ZFEC_HIP_GRID_CAP ---------------------------------------------
# (sz, cap): 20481 bytes are 6 units of 4 KiB (cps), the last overlapping its neighbour by 4095
# bytes; 5 workgroups give gs_s = 0, gs_c = 5.  8193 bytes are 3 units, the last overlapping by
# 1; 7 workgroups give gs_s = 2, gs_c = 1.
WALK_GEOM = [(20481, 5), (8193, 7)]
WALK_NS = 7
# (k, m): the arguments form; the table form in 5 row groups of 8 rows (the launcher's cut of 40
# rows at this size); the table form because k > 32, 6 rows in one group
WALK_SHAPES = [(6, 13), (20, 60), (94, 100)]


def run_walk(knobs, k, m, ns, sz, cap):
    """One encode of every parity block under the capped grid: each workgroup
    makes at least three steps with gs_c != 0; every stripe against the oracle,
    guard bytes included; without the hook, the same kernel and bytes."""
    r = m - k
    cps = units_of(sz)
    name = bsg_name(k, r, ns * cps, cus())
    ng = bsg_groups(r, int(name[13:name.index(",")])) if name.endswith(",tbl>") else 1
    steps = walk_steps(ns * ng * cps, cps, cap)
    rng = np.random.default_rng(k * 1000 + m + sz)
    blocks, want, index = encode_case(k, m, rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8))
    job = Batch(k, m, "enc", index, blocks, r)
    knobs(ZFEC_HIP_GRID_CAP=cap)
    got_name = job.launch()
    knobs(ZFEC_HIP_GRID_CAP=0)
    assert got_name == name, (k, m, sz, got_name)
    check_rows(job.rows((k, m, sz, "capped")), want, (k, m, sz, cap))
    capped = job.dst.clone()
    assert job.launch() == name, "the hook changed the kernel chosen"
    assert torch.equal(job.dst, capped), (k, m, sz, "capped and uncapped bytes differ")
    return name, steps


@pytest.mark.parametrize("geom", [0, 1], ids=["cps6-cap5", "cps3-cap7"])
@pytest.mark.parametrize("k,m", WALK_SHAPES)
def test_bsg_grid_stride_walk(bsg_only, knobs, k, m, geom):
    """The walk runs one step ahead of itself (s2, c2, with the same carry) to
    load the next unit's first inputs during the current unit's last phase."""
    sz, cap = WALK_GEOM[geom]
    assert (cap // units_of(sz), cap % units_of(sz)) == ((0, 5), (2, 1))[geom]
    name, steps = run_walk(knobs, k, m, WALK_NS, sz, cap)
    assert name == ("matapply_bsg<2,2>" if (k, m) == (6, 13) else "matapply_bsg<2,2,tbl>") and steps >= 3


# ---- every instantiation by name -----------------------------------------------------------------
# (k, r, sz, eighths): a batch of `eighths` x CUs / 2 units, i.e. eighths / 8 of the 4 x CUs below
# which launch_bsg steps down.  8: the RT of ceil(r / 4) holds, in the arguments form (one row
# group).  5: one group of the first RT is too few (5/8), two groups of the next smaller RT are
# enough (10/8), so the launch stops there in the table form, its second group short (r = 19:
# groups of 16 and 3 rows on RT 4).  0: three stripes; nothing shrinks below RT 2, and RT 1 is
# chosen by r <= 4 alone.  RT 1 and RT 12 in the table form need k > 32: r <= 4 makes one group,
# and past 48 rows a k <= 32 call is cut before it reaches the launcher.  Odd k: the last phase
# holds one input; r not a multiple of 4: the last waves own fewer rows.
INSTANCES = {
    "matapply_bsg<1,2>": (9, 3, 8193, 0),
    "matapply_bsg<2,2>": (5, 7, 4097, 0),
    "matapply_bsg<3,2>": (5, 9, 4096, 8),
    "matapply_bsg<4,2>": (6, 13, 8193, 8),
    "matapply_bsg<5,2>": (7, 19, 4096, 8),
    "matapply_bsg<6,2>": (5, 22, 8193, 8),
    "matapply_bsg<8,2>": (6, 30, 4096, 8),
    "matapply_bsg<10,2>": (7, 37, 8193, 8),
    "matapply_bsg<12,2>": (5, 47, 4096, 8),
    "matapply_bsg<1,2,tbl>": (33, 3, 8193, 0),
    "matapply_bsg<2,2,tbl>": (5, 12, 4097, 0),
    "matapply_bsg<3,2,tbl>": (7, 16, 8193, 5),
    "matapply_bsg<4,2,tbl>": (5, 19, 4096, 5),
    "matapply_bsg<5,2,tbl>": (7, 23, 8193, 5),
    "matapply_bsg<6,2,tbl>": (5, 31, 4096, 5),
    "matapply_bsg<8,2,tbl>": (6, 39, 8193, 5),
    "matapply_bsg<10,2,tbl>": (5, 46, 4096, 5),
    "matapply_bsg<12,2,tbl>": (33, 49, 4096, 5),
}


def instance_stripes(sz, eighths):
    return -(-(eighths * cus() // 2) // units_of(sz)) if eighths else 3


def test_bsg_instance_table_names_all_18():
    names = {"matapply_bsg<%d,2%s>" % (rt, t) for rt in BSG_RT for t in ("", ",tbl")}
    assert len(names) == 18 and set(INSTANCES) == names
    for want, (k, r, sz, eighths) in INSTANCES.items():
        assert bsg_name(k, r, units_of(sz, instance_stripes(sz, eighths)), cus()) == want, want


def run_instance(k, r, sz, ns, want_name, knobs=None, cap=0):
    """Encode r parity rows of the k/(k + r) code over ns stripes, every stripe
    against the oracle."""
    m = k + r
    rng = np.random.default_rng(k * 1000 + r + sz)
    blocks, want, index = encode_case(k, m, rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8))
    job = Batch(k, m, "enc", index, blocks, r)
    assert job.src.numel() + job.dst.numel() < 1 << 30
    if cap:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    got_name = job.launch()
    if cap:
        knobs(ZFEC_HIP_GRID_CAP=0)
    assert got_name == want_name, (k, r, sz, ns, got_name)
    check_rows(job.rows((want_name, cap)), want, (want_name, cap))


@pytest.mark.parametrize("name", list(INSTANCES))
def test_bsg_every_instantiation(bsg_only, name):
    """Each RT is its own unrolled kernel, with its own bsg_phase_bytes padding,
    coefficient byte packing and register pressure; each runs in both forms."""
    k, r, sz, eighths = INSTANCES[name]
    ns = instance_stripes(sz, eighths)
    assert bsg_name(k, r, units_of(sz, ns), cus()) == name
    run_instance(k, r, sz, ns, name)


def test_bsg_large_rt_grid_stride_walk(bsg_only, knobs):
    """matapply_bsg<10,2> over three-unit stripes on 61 workgroups (gs_s = 20,
    gs_c = 1): a large-RT form with the carry and the prefetch across units."""
    name = "matapply_bsg<10,2>"
    k, r, sz, eighths = INSTANCES[name]
    ns = instance_stripes(sz, eighths)
    assert units_of(sz) == 3 and walk_steps(units_of(sz, ns), 3, 61) >= 3
    run_instance(k, r, sz, ns, name, knobs, 61)


# ---- every coefficient --------------------------------------------------------------------------

def test_bsg_every_coefficient(bsg_only):
    """Every row of the offset bank (g_bsg: 256 coefficients x 16 LDS offsets):
    the 32/72 encode (253 of the 255 nonzero coefficients) and decodes chosen
    until their matrices have used the remaining ones, each against the oracle.
    Coefficient 0 is the padding rows and inputs of the walk order."""
    k, m, sz = 32, 72, 4096
    rng = np.random.default_rng(256)
    data = rng.integers(0, 256, size=(k, sz), dtype=np.uint8)
    ins = [torch.from_numpy(data[i]).cuda() for i in range(k)]
    enc = zfec_amd.Encoder(k, m).encode(ins)
    torch.cuda.synchronize()
    assert capi.last_kernel_name() == bsg_name(k, m - k, 1, cus()), capi.last_kernel_name()
    assert (torch.stack(enc[k:]).cpu().numpy() == oracle.encode(k, m, data)).all()
    cov = set(np.asarray(oracle.enc_matrix(k, m)).reshape(m, k)[k:].flatten().tolist())
    dec = zfec_amd.Decoder(k, m)
    tries = 0
    while not cov >= set(range(1, 256)) and tries < 400:
        tries += 1
        nums = sorted(int(x) for x in rng.choice(m, size=k, replace=False))
        sl = place(nums, k)
        miss = [i for i in range(k) if sl[i] >= k]
        if len(miss) * k < 24:
            continue
        dm = np.asarray(oracle.decode_matrix(k, m, sl)).reshape(k, k)
        new = set(dm[miss].flatten().tolist()) - cov
        if not new:
            continue
        cov |= new
        got = dec.decode([enc[n] for n in nums], nums)
        torch.cuda.synchronize()
        assert capi.last_kernel_name() == bsg_name(k, len(miss), 1, cus()), capi.last_kernel_name()
        recv = np.stack([(data[n] if n < k else enc[n].cpu().numpy()) for n in sl])
        assert (torch.stack(got).cpu().numpy()[miss] == oracle.decode(k, m, recv, sl)).all(), nums
        assert (torch.stack(got).cpu().numpy() == data).all(), nums
    assert cov >= set(range(1, 256)), sorted(set(range(1, 256)) - cov)
