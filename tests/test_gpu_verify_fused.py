"""GPU checks of the fused wide-code verify (fec_verify_batch on 4 < k <= 32:
zfec_amd/csrc/kernels.hip matverify_bsr<RT>, <RT,lds>, <RT,lds,tbl>), with the
discipline of test_gpu_verify.py, whose helpers are used: shares from the CPU
oracle, expected bits from the oracle-built P (tests/verify_ref.py), inputs at
byte offset 3, pre-filled mismatch words between guard words, src compared
byte for byte after every call, and the kernel name checked.

Most cases run under ZFEC_HIP_VERIFY_FUSED_MIN=1 so that launches of a few
2-KiB units take the fused kernels; the gate itself is checked at the default.

The bit-sliced kernels' grid is capped at CUs x 1024 workgroups (2^18 units on
256 CUs, 512 MiB per block), or by ZFEC_HIP_GRID_CAP when that is lower: with
it test_fused_grid_stride_walk walks every form grid-stride, with the carry
from unit into stripe, over blocks whose last unit overlaps its neighbour."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from test_gpu_verify import Case, IN_OFF, check_rows, expected_bits, pack, patterns, stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# Config::verify_fused_min's default (zfec_amd/csrc/config.cpp kVerifyFusedMin)
DEFAULT_FUSED_MIN = 64
OFF = 4294967295

SIZES = (2048, 2049, 4097, 6161)  # one unit; the overlapped last unit; 3 and 4 units
NS = (1, 3, 5)
SZMAX, NSMAX = max(SIZES), max(NS)

# (k, m, blocks held) -> the kernel the call's last launch must be
SHAPES = {
    (10, 16, 16): "matverify_bsr<6>",         # c = 6: one wave
    (6, 22, 22): "matverify_bsr<8,lds>",      # c = 16: two waves, argument addresses
    (5, 25, 25): "matverify_bsr<5,lds>",      # c = 20: four waves
    (20, 60, 60): "matverify_bsr<10,lds,tbl>",  # c = 40: W = 2, rows 30-39 straddle the word boundary
    (20, 60, 57): "matverify_bsr<10,lds,tbl>",  # c = 37: tiles of 9, 9, 9, 10 rows (rows < RT)
    (8, 56, 56): "matverify_bsr<8>",          # c = 48: 40 rows (<10,lds>), then 8 from bit 40
}
SHAPE_IDS = ["%d-%d-%d" % s for s in SHAPES]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def two_bases(k, m, nb, seed):
    """The primaries basis and a mixed one, nb blocks held."""
    rng = np.random.default_rng(seed)
    while True:
        mixed = rng.permutation(m).tolist()
        primary = [b < k for b in mixed[:k]]
        if any(primary) and not all(primary):
            break
    return [("primaries", list(range(nb))), ("mixed", mixed[:nb])]


def unit_patterns(k, c, ns, sz, seed):
    """Corruptions placed by the 2-KiB unit's geometry: a lane's first piece
    ends at byte 1023 of the unit, its second starts at 1024, the unit ends at
    2047; the last unit starts at sz - 2048 and overlaps its neighbour."""
    rng = np.random.default_rng(seed)
    last = sz - 2048
    xs = sorted({x for x in (0, 1023, 1024, 2047, 2048, last - 1, last, last + 1, last + 1023, last + 1024)
                 if 0 <= x < sz})
    spread = [(i % ns, k + int(rng.integers(0, c)), x, 1 << (i % 8)) for i, x in enumerate(xs)]
    return {
        "unit offsets, checks": spread,
        "basis, second piece": [(ns // 2, int(rng.integers(0, k)), last + 1024, 0x81)],
        "basis, both sides of the overlap": [(0, 0, max(0, last - 1), 2), (ns - 1, k - 1, last, 4)],
        "last check, last byte": [(ns - 1, k + c - 1, sz - 1, 0x40)],
    }


def all_patterns(k, c, ns, sz, seed):
    out = dict(patterns(k, c, ns, sz, seed))
    out.update(unit_patterns(k, c, ns, sz, seed))
    return out


class FusedCase(Case):
    expect = "rows_differ"

    def kernel_name(self):
        return self.expect


def make_case(shape, nums, ns, sz, kind="padded", expect=None, **kw):
    k, m, _ = shape
    case = FusedCase(k, m, nums, ns, sz, kind, szmax=max(SZMAX, sz), nsmax=max(NSMAX, ns), **kw)
    case.expect = SHAPES[shape] if expect is None else expect
    return case


# ---- every form, size, batch and layout --------------------------------------------------

@pytest.mark.parametrize("kind", ["padded", "bm"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_fused_forms(shape, kind, knobs):
    knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
    k, m, nb = shape
    code = capi.Code(k, m)
    for bname, nums in two_bases(k, m, nb, seed=k + nb):
        for ns in NS:
            for sz in SIZES:
                case = make_case(shape, nums, ns, sz, kind)
                for pname, cor in all_patterns(k, case.c, ns, sz, k + sz + ns).items():
                    got = case.run(code, cor, (shape, kind, bname, ns, sz, pname))
                    if pname == "every check":
                        assert (got == pack(np.ones((ns, case.c), dtype=bool))).all()


@pytest.mark.parametrize("shape", list(SHAPES), ids=SHAPE_IDS)
def test_fused_bits_equal_two_step_bits(shape, knobs):
    """The same corrupted buffers through both paths: identical words."""
    k, m, nb = shape
    ns, sz = 5, 6161
    code = capi.Code(k, m)
    for bname, nums in two_bases(k, m, nb, seed=k + nb):
        case = make_case(shape, nums, ns, sz)
        pats = all_patterns(k, case.c, ns, sz, 7 * k + nb)
        knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
        fused = {p: case.run(code, cor, ("fused", shape, bname, p)) for p, cor in pats.items()}
        knobs(ZFEC_HIP_VERIFY_FUSED_MIN=OFF)
        case.expect = "rows_differ"
        for p, cor in pats.items():
            assert (case.run(code, cor, ("two-step", shape, bname, p)) == fused[p]).all(), (shape, bname, p)
        assert any(w.any() for w in fused.values())


# ---- the grid-stride walk ------------------------------------------------------------------
# (sz, cap) as in test_gpu_bsr.py: 6 units per stripe on 5 workgroups (gs_s = 0, gs_c = 5, the
# last unit overlapping by 2047 bytes), 3 units on 7 workgroups (gs_s = 2, gs_c = 1, by 1 byte)
WALK_GEOM = [(10241, 5), (4097, 7)]
WALK_NS = 7
WALK_SHAPES = [(10, 16, 16), (6, 22, 22), (5, 25, 25), (20, 60, 60)]  # <6>, <8,lds>, <5,lds>, <10,lds,tbl>


def every_unit_pattern(k, c, ns, sz):
    """One flipped byte in every (stripe, unit) pair, each unit of a stripe in
    another check block and at a byte no other unit covers (a unit's first
    byte; the overlapping last unit's last byte): every walk iteration must
    report, and a unit run twice or not at all changes the words."""
    cps = -(-sz // 2048)
    assert cps <= c
    return [(s, k + (s * cps + u) % c, sz - 1 if u == cps - 1 else u * 2048, 1 + (s + u) % 255)
            for s in range(ns) for u in range(cps)]


@pytest.mark.parametrize("geom", [0, 1], ids=["cps6-cap5", "cps3-cap7"])
@pytest.mark.parametrize("shape", WALK_SHAPES, ids=["%d-%d-%d" % s for s in WALK_SHAPES])
def test_fused_grid_stride_walk(shape, geom, knobs):
    """ZFEC_HIP_GRID_CAP below the units of the call: each workgroup makes at
    least three steps of the walk (the one-wave form's u += gridDim.x; the
    LDS-phase forms' c += gs_c; s += gs_s with the carry, gs_c != 0).  A clean
    run leaves every word zero; then the usual corruptions and one in every
    (stripe, unit) pair; words from the oracle's P, src unchanged, guard words
    intact (Case.run).  Without the hook: the same kernel and words."""
    k, m, nb = shape
    sz, cap = WALK_GEOM[geom]
    ns, cps = WALK_NS, -(-sz // 2048)
    assert (cap // cps, cap % cps) == ((0, 5), (2, 1))[geom] and ns * cps >= 3 * cap
    code = capi.Code(k, m)
    for bname, nums in two_bases(k, m, nb, seed=k + nb):
        case = make_case(shape, nums, ns, sz)
        pats = all_patterns(k, case.c, ns, sz, k + sz + ns)
        pats["every unit"] = every_unit_pattern(k, case.c, ns, sz)
        assert pats.pop("clean") == []
        knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1, ZFEC_HIP_GRID_CAP=cap)
        assert not case.run(code, [], (shape, bname, sz, "clean, capped")).any()
        capped = {p: case.run(code, cor, (shape, bname, sz, p, "capped")) for p, cor in pats.items()}
        knobs(ZFEC_HIP_GRID_CAP=0)
        for p, cor in pats.items():
            assert (case.run(code, cor, (shape, bname, sz, p, "uncapped")) == capped[p]).all(), (shape, bname, p)
        unit_bits = expected_bits(case.P, k, ns, pats["every unit"])
        assert (unit_bits.sum(axis=1) == cps).all()
        assert (capped["every check"] == pack(np.ones((ns, case.c), dtype=bool))).all()


# ---- the gate ------------------------------------------------------------------------------

def test_gate_at_the_default_threshold():
    """K=10/M=16 in one-unit blocks: exactly the default number of units runs
    the fused kernel, one unit fewer the two steps, with identical words."""
    k, m, sz = 10, 16, 2048
    shape = (k, m, m)
    code = capi.Code(k, m)
    got = []
    for ns, name in ((DEFAULT_FUSED_MIN, "matverify_bsr<6>"), (DEFAULT_FUSED_MIN - 1, "rows_differ")):
        case = make_case(shape, range(m), ns, sz, expect=name)
        cor = [(0, 3, 5, 1), (20, 12, 2047, 2), (30, 15, 1024, 4), (7, k, 0, 8)]  # (the default is never below 32)
        case.run(code, [], (ns, "clean"))
        got.append(case.run(code, cor, (ns, "corrupt")))
    assert (got[0][:DEFAULT_FUSED_MIN - 1] == got[1]).all() and not got[0][DEFAULT_FUSED_MIN - 1].any()
    assert got[1][0, 0] == 0x3F and got[1][7, 0] == 1 and got[1][30, 0] == 0x20


def test_short_blocks_keep_the_two_steps(knobs):
    knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
    k, m, ns, sz = 10, 16, 5, 2047
    code = capi.Code(k, m)
    case = make_case((k, m, m), range(m), ns, sz, expect="rows_differ")
    for pname, cor in patterns(k, case.c, ns, sz, 3).items():
        case.run(code, cor, (sz, pname))


def test_page_locked_src_keeps_the_two_steps(knobs):
    knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
    k, m, ns, sz = 10, 16, 5, 1025
    code = capi.Code(k, m)
    case = make_case((k, m, m), range(m), ns, sz, expect="rows_differ", src_mem="pinned")
    case.run(code, [(1, 12, 5, 1)], "pinned src", flags=0)


# ---- memory kinds, streams -----------------------------------------------------------------

@pytest.mark.parametrize("mask_mem", ["numpy", "pinned"])
@pytest.mark.parametrize("shape", [(10, 16, 16), (20, 60, 60)], ids=["10-16", "20-60"])
def test_mismatch_in_host_memory(shape, mask_mem, knobs):
    knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
    k, m, nb = shape
    ns, sz = 5, 4097
    code = capi.Code(k, m)
    case = make_case(shape, range(nb), ns, sz)
    for flags in (capi.FEC_FLAG_ASYNC, 0, capi.FEC_FLAG_LIBRARY_STREAM):
        for pname, cor in all_patterns(k, case.c, ns, sz, 3).items():
            case.run(code, cor, (mask_mem, flags, pname), mask_mem=mask_mem, flags=flags)


def test_library_stream(knobs):
    knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
    shape = (6, 22, 22)
    k, m, nb = shape
    ns, sz = 3, 6161
    code = capi.Code(k, m)
    case = make_case(shape, range(nb), ns, sz)
    for pname, cor in all_patterns(k, case.c, ns, sz, 11).items():
        case.run(code, cor, ("library stream", pname), flags=capi.FEC_FLAG_LIBRARY_STREAM)


@pytest.mark.parametrize("shape", [(10, 16, 16), (20, 60, 60)], ids=["10-16", "20-60"])
def test_two_streams(shape, knobs):
    """Six asynchronous calls alternating over two streams, device masks: the
    fused path shares no buffer between them, and every result is exact."""
    knobs(ZFEC_HIP_VERIFY_FUSED_MIN=1)
    k, m, nb = shape
    ns, sz = 5, 4097
    c = nb - k
    W = (c + 31) // 32
    code = capi.Code(k, m)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for i in range(6):
        case = make_case(shape, range(nb), ns, sz)
        cor = [(i % ns, k + (7 * i) % c, (i * 700) % sz, 1 + i), ((i + 1) % ns, k + c - 1 - i, sz - 1 - i, 0x80)]
        case.corrupt(cor)
        mask = torch.full((ns * W,), -1, dtype=torch.int32, device="cuda")
        runs.append((case, cor, mask))
    torch.cuda.synchronize()
    for i, (case, cor, mask) in enumerate(runs):
        code.verify_batch(case.src.data_ptr() + IN_OFF, case.lay.bs, case.lay.ss, case.nums, sz, ns, mask.data_ptr(),
                          stream=streams[i % 2].cuda_stream)
        assert capi.last_kernel_name() == SHAPES[shape]
    torch.cuda.synchronize()
    for i, (case, cor, mask) in enumerate(runs):
        want = pack(expected_bits(case.P, k, ns, cor))
        assert (mask.cpu().numpy().view(np.uint32).reshape(ns, W) == want).all(), i


# ---- Python API ----------------------------------------------------------------------------

def test_python_api_at_the_default_gate():
    """Decoder.verify_batch on a batch past the default threshold: the fused
    kernel, bits from the oracle's P."""
    k, m, sz = 10, 16, 4097  # 3 units per stripe
    ns = DEFAULT_FUSED_MIN // 3 + 2
    dec = zfec_amd.Decoder(k, m)
    nums = np.random.default_rng(m).permutation(m).tolist()
    c = m - k
    P = check_rows(k, m, tuple(nums))
    allb = stripes(k, m, ns, sz)
    host = np.ascontiguousarray(allb[:, nums, :])
    cor = [(3, k + c - 1, sz - 1, 1), (4, k, 0, 2), (9, 0, 2500, 3), (ns - 1, k + c // 2, 2048, 4)]
    for s, j, x, v in cor:
        host[s, j, x] ^= v
    want = expected_bits(P, k, ns, cor)
    blocks = torch.from_numpy(host).cuda()
    out = dec.verify_batch(blocks, nums)
    assert capi.last_kernel_name() == "matverify_bsr<6>"
    assert out.dtype == torch.bool and tuple(out.shape) == (ns, c)
    assert (out.cpu().numpy() == want).all()
    assert want[9].all() and want.sum() == c + 3
    bm = blocks.transpose(0, 1).contiguous().transpose(0, 1)  # block-major
    assert (dec.verify_batch(bm, nums).cpu().numpy() == want).all()
    assert capi.last_kernel_name() == "matverify_bsr<6>"
    clean = torch.from_numpy(np.ascontiguousarray(allb[:, nums, :])).cuda()
    assert not dec.verify_batch(clean, nums).any()
    assert torch.equal(blocks.cpu(), torch.from_numpy(host))
