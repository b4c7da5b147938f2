"""The carry of the wave walk (zfec_amd/csrc/kernels.hip: `w += gs_w; s += gs_s;
if (w >= wps) { w -= wps; ++s; }`) in every kernel the launcher's fill_walk
feeds: matapply_mixed<K>, matrepair_mixed<K,R>, matverify_reg<K,R>,
rows_differ, matlocate_reg<K,R>, rows_locate, matcorrect_reg<K> and
rows_correct.  A launch walks only past CUs x 8192 workgroups, and the carry
runs only where the step is no whole number of stripes (gs_w != 0), which the
test_grid_stride tests of test_gpu_verify / locate / correct / mixed / repair
never have.  ZFEC_HIP_GRID_CAP brings it to 37 small stripes:

          cap   waves per step   sz     wps   (gs_s, gs_w)
    G1    3     12               4097   5     (2, 2)
    G2    1     4                4097   5     (0, 4)   a step shorter than one stripe
    G3    5     20               6160   7     (2, 6)

The geometry is computed with the launcher's arithmetic and asserted before any
launch (scrub_matrix.wave_walk: gs_w != 0, at least 3 steps per wave).  Every
result is checked against the CPU oracle or the numpy models by the harness of
the kernel's own test file, the kernel name is asserted, and the hooked call
must give what the same call gives without the hook.

Writing kernels: 0xA5-filled outputs at odd offsets, every stripe bit-exact,
guards untouched, so a unit the walk skipped shows as untouched bytes.  Reading
kernels: wps rounds, round t corrupting one byte in wave (s + t) mod wps of
stripe s, in check s mod c; every (stripe, wave) pair carries a bit that a
skipped visit loses.  The byte is one no other wave reads (not in the
overlapped last chunk).  Correction: the same placement in slot s mod (k + c),
so every wave of every stripe has a byte only it can put right."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from scrub_matrix import wave_walk
import test_gpu_correct
import test_gpu_locate
import test_gpu_mixed
import test_gpu_repair
import test_gpu_verify

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NS = 37
GEOMETRIES = {"G1": (3, 4097, 5, (2, 2)), "G2": (1, 4097, 5, (0, 4)), "G3": (5, 6160, 7, (2, 6))}
FUSED_OFF = 4294967295

MIXED = [1, 2, 3, 4]
REPAIR = [(1, 1), (3, 7), (4, 8)]
READERS = [("matverify_reg<3,7>", 3, 10), ("matlocate_reg<3,7>", 3, 10), ("rows_differ", 10, 16),
           ("rows_locate", 10, 16)]
CORRECTORS = [("matcorrect_reg<3>", 3, 10), ("rows_correct", 10, 16)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def geometry(geom):
    """(cap, sz, wps) of a geometry, once the launcher's arithmetic has given
    the table's step and at least three steps per wave."""
    cap, sz, wps, step = GEOMETRIES[geom]
    got_wps, gs_s, gs_w, steps = wave_walk(cap, sz, NS)
    assert (got_wps, (gs_s, gs_w)) == (wps, step) and gs_w != 0 and steps >= 3
    return cap, sz, wps


def own_byte(sz, wps, v, salt):
    """A byte of wave v (64 chunks of 16 bytes from 1024 v) that no other wave
    reads: the overlapped last chunk [sz - 16, sz) belongs to the last wave."""
    lo = 1024 * v
    hi = min(lo + 1024, sz) if v == wps - 1 else min(lo + 1024, sz - 16)
    assert lo < hi
    return lo + salt % (hi - lo)


def rounds(sz, wps, nslots, first):
    """wps corruption lists [(stripe, slot, byte, value)]: round t touches wave
    (s + t) mod wps of stripe s, in slot first + s mod nslots."""
    return [[(s, first + s % nslots, own_byte(sz, wps, (s + t) % wps, 7 * s + 13 * t), 1 + (3 * s + t) % 255)
             for s in range(NS)] for t in range(wps)]


def as_arrays(cor):
    return [(s, j, np.array([x]), np.array([v], dtype=np.uint8)) for s, j, x, v in cor]


# ---- writing kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("K", MIXED)
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_mixed_carry(knobs, geom, K):
    """matapply_mixed<K>, a pattern per stripe: test_gpu_mixed.check holds every
    stripe against the original data, the guards and the kernel name."""
    cap, sz, wps = geometry(geom)
    m = K + 4
    code = capi.Code(K, m)
    pats = test_gpu_mixed.random_patterns(np.random.default_rng(10 * K + cap), K, m, NS)
    assert test_gpu_mixed.OUT_OFF % 2 == 1
    plain = test_gpu_mixed.check(code, K, m, NS, sz, pats, np.arange(NS))
    knobs(ZFEC_HIP_GRID_CAP=cap)
    capped = test_gpu_mixed.check(code, K, m, NS, sz, pats, np.arange(NS))
    assert capi.last_kernel_name() == "matapply_mixed<%d>" % K
    assert (plain == capped).all()


@pytest.mark.parametrize("K,R", REPAIR)
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_repair_carry(knobs, geom, K, R):
    """matrepair_mixed<K,R> with the patterns of its sweep (NONE rows keep the
    guard): test_gpu_repair.check holds every row against the oracle's blocks."""
    cap, sz, wps = geometry(geom)
    m = K + 8
    name = "matrepair_mixed<%d,%d>" % (K, R)
    code = capi.Code(K, m)
    pres, tgts = test_gpu_repair.sweep_patterns(np.random.default_rng(10 * K + R + cap), K, m, R, NS)
    plain = test_gpu_repair.check(code, K, m, NS, sz, pres, tgts, np.arange(NS), name=name)
    knobs(ZFEC_HIP_GRID_CAP=cap)
    capped = test_gpu_repair.check(code, K, m, NS, sz, pres, tgts, np.arange(NS), name=name)
    assert (plain == capped).all()


# ---- reading kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k,m", READERS)
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_reader_carry(knobs, geom, name, k, m):
    cap, sz, wps = geometry(geom)
    c = m - k
    code = capi.Code(k, m)
    locate = "locate" in name
    if locate:
        case = test_gpu_locate.Case(k, m, range(m), NS, sz, szmax=sz)
        assert test_gpu_locate.kernel_name(k, c) == name
        want = [k + s % c for s in range(NS)]
        run = lambda cor, what: case.run(code, as_arrays(cor), what)  # noqa: E731
    else:
        case = test_gpu_verify.Case(k, m, range(m), NS, sz, szmax=sz, nsmax=test_gpu_locate.NSMAX)
        assert case.kernel_name() == name
        want = [[1 << (s % c)] for s in range(NS)]
        run = lambda cor, what: case.run(code, cor, what)  # noqa: E731
    cors = rounds(sz, wps, c, k)
    hook = dict(ZFEC_HIP_VERIFY_FUSED_MIN=FUSED_OFF) if name == "rows_differ" else {}
    if hook:
        knobs(**hook)
    plain = [run(cor, (geom, "plain", t)) for t, cor in enumerate(cors)]
    assert capi.last_kernel_name() == name
    knobs(ZFEC_HIP_GRID_CAP=cap, **hook)
    for t, cor in enumerate(cors):
        got = run(cor, (geom, "capped", t))
        assert capi.last_kernel_name() == name
        assert got.tolist() == want and (got == plain[t]).all(), (geom, name, t)


# ---- correction -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k,m", CORRECTORS)
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_correct_carry(knobs, geom, name, k, m):
    """Slot s mod (k + c) of stripe s is named and rewritten: the verdicts and
    the whole buffer against correct_ref (Case.run), and every block clean."""
    cap, sz, wps = geometry(geom)
    code = capi.Code(k, m)
    case = test_gpu_correct.Case(k, m, range(m), NS, sz, szmax=sz)
    assert test_gpu_correct.kernel_name(k) == name
    cors = rounds(sz, wps, m, 0)
    plain = [case.run(code, as_arrays(cor), (geom, "plain", t)) for t, cor in enumerate(cors)]
    knobs(ZFEC_HIP_GRID_CAP=cap)
    for t, cor in enumerate(cors):
        got, after = case.run(code, as_arrays(cor), (geom, "capped", t))
        assert capi.last_kernel_name() == name
        assert got.tolist() == [s % m for s in range(NS)] and (got == plain[t][0]).all(), (geom, name, t)
        assert (after == case.clean).all() and (after == plain[t][1]).all()


def test_every_walk_case_is_collected():
    """Three geometries of 4 + 3 + 4 + 2 kernels: every kernel fill_walk feeds."""
    per_geometry = len(MIXED) + len(REPAIR) + len(READERS) + len(CORRECTORS)
    assert (len(GEOMETRIES), per_geometry) == (3, 13)
    names = {"matapply_mixed", "matrepair_mixed"} | {n.split("<")[0] for n, _, _ in READERS + CORRECTORS}
    assert names == {"matapply_mixed", "matrepair_mixed", "matverify_reg", "rows_differ", "matlocate_reg",
                     "rows_locate", "matcorrect_reg", "rows_correct"}
