"""Every <K,R> form of the k <= 4 scrub kernels (zfec_amd/csrc/kernels.hip):
all 32 matverify_reg<K,R>, all 28 matlocate_reg<K,R> and matcorrect_reg<K>
behind each of them, launched by name on the designed error matrix of
tests/scrub_matrix.py -- one stripe per case: clean, a single error in every
slot, every (basis j, check i) pair, every pair of basis slots, and the double
errors that satisfy rows 0 and 1 of a wrong hypothesis.  Each form has its own
register allocation and its own way of reading its tables (reg_argload,
locate_argload), and the Q tables of locate are reached on dirty data only: a
pair (j, i) breaks exactly row i of hypothesis j, so a skipped or mis-read
qtab entry names slot j where MANY is due.

Code (K, K + 8); the slots are the first K + R of the all-parity and of the
mixed basis, so checks include primaries.  Sizes 15, 17, 1024, 1025 and 4097
with the layouts packed, padded and block-major rotating over them; inputs
start at byte offset 3; mask and verdict words sit between guard words.  The
harnesses are those of test_gpu_verify, test_gpu_locate and test_gpu_correct:
expected masks from verify_ref, verdicts from locate_ref, the whole block
buffer from correct_ref, never from the library; and the verdicts the matrix
was designed for are asserted on top.  Every form runs once more under
ZFEC_HIP_GRID_CAP=3 on 4097-byte stripes (5 waves each, a step of 12 waves:
gs_w = 2), so each compiled kernel takes the carry of the wave walk
(test_gpu_wave_walk.py has the other geometries)."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from locate_ref import CLEAN, MANY, oracle_PQ
from scrub_matrix import error_matrix, flat, form_bases, matrix_size, pair_of, select, wave_walk
import test_gpu_correct
import test_gpu_locate
import test_gpu_verify
from test_gpu_verify import bases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = (15, 17, 1024, 1025, 4097)
LAYOUTS = ("packed", "padded", "bm")
NSMAX, SZMAX = 70, 4097
WALK_CAP, WALK_SZ, WALK_NS = 3, 4097, 8  # G1 of test_gpu_wave_walk.py; at least 8 stripes = 40 waves

VERIFY_FORMS = [(K, R) for K in range(1, 5) for R in range(1, 9)]
LOCATE_FORMS = [(K, R) for K, R in VERIFY_FORMS if R >= 2]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def runs(K, R):
    """(basis name, block numbers, sz, layout) of every run of form <K,R>."""
    for b, (bname, nums) in enumerate(form_bases(K, R)):
        for i, sz in enumerate(SIZES):
            yield bname, nums, sz, LAYOUTS[(i + b + K + R) % 3]


def matrix(K, m, nums, sz):
    P, Q = oracle_PQ(K, m, tuple(nums))
    R = len(nums) - K
    cor, designed, kinds = error_matrix(K, R, P, Q, sz, np.random.default_rng(1000 * K + 10 * R + sz))
    assert len(designed) == matrix_size(K, R) <= NSMAX
    return cor, designed, kinds


def walk_run(K, R):
    """The mixed basis, 4097 bytes, padded, at least WALK_NS stripes (the ones
    past the matrix are clean); the geometry is checked before any launch."""
    bname, nums = form_bases(K, R)[-1]
    assert bname == "mixed"
    cor, designed, kinds = matrix(K, K + 8, nums, WALK_SZ)
    ns = max(len(designed), WALK_NS)
    designed = designed + [CLEAN] * (ns - len(designed))
    wps, gs_s, gs_w, steps = wave_walk(WALK_CAP, WALK_SZ, ns)
    assert (wps, gs_s, gs_w) == (5, 2, 2)
    return nums, cor, designed, ns


def check_designed(got, designed, kinds, what):
    for s, d in enumerate(designed):
        if d is not None:
            assert got[s] == d, (what, s, kinds[s] if s < len(kinds) else "clean", hex(int(got[s])), d)


def fooled_present(K, R, got, kinds):
    """Wherever K >= 2 the call held double errors built to satisfy rows 0 and 1
    of a wrong hypothesis: named (miscorrected) with two checks, MANY with three."""
    fooled = [s for s, kind in enumerate(kinds) if kind.startswith("fooled")]
    assert len(fooled) == (2 * K if K >= 3 else K if K == 2 else 0)
    if R == 2:
        assert sorted({int(got[s]) for s in fooled}) == (list(range(K)) if K >= 2 else [])
    else:
        assert all(got[s] == MANY for s in fooled)


# ---- matverify_reg<K,R> -----------------------------------------------------------------------

def verify_once(code, K, m, nums, cor, designed, ns, sz, kind, name, what):
    case = test_gpu_verify.Case(K, m, nums, ns, sz, kind, szmax=SZMAX, nsmax=NSMAX)
    assert case.kernel_name() == name  # Case.run asserts the launch's name against it
    assert not case.run(code, [], what + ("clean",)).any()
    words = case.run(code, flat(cor), what)
    assert capi.last_kernel_name() == name
    dirty = words.any(axis=1)
    assert all(dirty[s] == (d != CLEAN) for s, d in enumerate(designed) if d is not None), what
    return words


@pytest.mark.parametrize("K,R", VERIFY_FORMS)
def test_verify_form(knobs, K, R):
    """c = R: one launch of matverify_reg<K,R> on clean data and on the singles
    and (basis, check) stripes; then c = 8 + R of code (K, K + 16): launches
    <K,8> + <K,R>, the second with bit0 = 8, its pairs on checks 8..8+R-1."""
    name = "matverify_reg<%d,%d>" % (K, R)
    m = K + 8
    code = capi.Code(K, m)
    keep = lambda s, kind: kind in ("clean", "single", "pair")  # noqa: E731
    for bname, nums, sz, kind in runs(K, R):
        cor, designed, kinds = select(*matrix(K, m, nums, sz), keep)
        words = verify_once(code, K, m, nums, cor, designed, len(designed), sz, kind, name, (K, R, bname, sz, kind))
        # a single error in check i sets bit i alone, one in a basis slot every bit (P has no zero)
        for s in range(1, 1 + K + R):
            assert words[s, 0] == ((1 << R) - 1 if s - 1 < K else 1 << (s - 1 - K)), (bname, sz, s)
    # two launches
    m2, c2 = K + 16, 8 + R
    code2 = capi.Code(K, m2)
    for b, (bname, nums) in enumerate(bases(K, m2, seed=50 * K)[1:]):
        nums = nums[:K + c2]
        for i, sz in enumerate((17, 1025)):
            P, Q = oracle_PQ(K, m2, tuple(nums))
            full = error_matrix(K, c2, P, Q, sz, np.random.default_rng(sz + R))
            late = lambda s, kind: kind in ("clean", "single") or (  # noqa: E731
                kind == "pair" and pair_of(K, c2, s)[1] >= 8)
            cor, designed, kinds = select(*full, late)
            assert len(designed) == 1 + K + c2 + K * R <= NSMAX
            verify_once(code2, K, m2, nums, cor, designed, len(designed), sz, LAYOUTS[(i + b + R) % 3], name,
                        (K, c2, bname, sz))
    # the carry of the wave walk
    nums, cor, designed, ns = walk_run(K, R)
    knobs(ZFEC_HIP_GRID_CAP=WALK_CAP)
    verify_once(code, K, m, nums, cor, designed, ns, WALK_SZ, "padded", name, (K, R, "walk"))


# ---- matlocate_reg<K,R> -----------------------------------------------------------------------

@pytest.mark.parametrize("K,R", LOCATE_FORMS)
def test_locate_form(knobs, K, R):
    """The whole matrix in one call: verdicts exact against the model and
    against the design, guards and src unchanged (Case.run), the kernel name."""
    name = "matlocate_reg<%d,%d>" % (K, R)
    m = K + 8
    code = capi.Code(K, m)
    assert test_gpu_locate.kernel_name(K, R) == name
    for bname, nums, sz, kind in runs(K, R):
        cor, designed, kinds = matrix(K, m, nums, sz)
        case = test_gpu_locate.Case(K, m, nums, len(designed), sz, kind)
        what = (K, R, bname, sz, kind)
        got = case.run(code, cor, what)
        assert capi.last_kernel_name() == name
        check_designed(got, designed, kinds, what)
        fooled_present(K, R, got, kinds)
    nums, cor, designed, ns = walk_run(K, R)
    case = test_gpu_locate.Case(K, m, nums, ns, WALK_SZ, "padded")
    knobs(ZFEC_HIP_GRID_CAP=WALK_CAP)
    got = case.run(code, cor, (K, R, "walk"))
    assert capi.last_kernel_name() == name
    check_designed(got, designed, [], (K, R, "walk"))


# ---- matcorrect_reg<K> behind every locate form -------------------------------------------------

def correct_once(code, case, cor, designed, kinds, name, what):
    got, after = case.run(code, cor, what)
    assert capi.last_kernel_name() == name
    check_designed(got, designed, kinds, what)
    named = got < case.nb
    assert named.sum() >= case.nb  # at least every single
    again, still = case.run(code, None, what + ("again",), blocks=after)
    assert (again[named] == CLEAN).all() and (still == after).all(), what
    return got


@pytest.mark.parametrize("K,R", LOCATE_FORMS)
def test_correct_form(knobs, K, R):
    """The same matrix through fec_correct_batch: verdicts and the whole block
    buffer, prefill bytes included, exact against correct_ref (Case.run); a
    second call on the result answers CLEAN wherever a slot was named."""
    name = "matcorrect_reg<%d>" % K
    m = K + 8
    code = capi.Code(K, m)
    assert test_gpu_correct.kernel_name(K) == name
    for bname, nums, sz, kind in runs(K, R):
        cor, designed, kinds = matrix(K, m, nums, sz)
        case = test_gpu_correct.Case(K, m, nums, len(designed), sz, kind)
        got = correct_once(code, case, cor, designed, kinds, name, (K, R, bname, sz, kind))
        fooled_present(K, R, got, kinds)
    nums, cor, designed, ns = walk_run(K, R)
    case = test_gpu_correct.Case(K, m, nums, ns, WALK_SZ, "padded")
    knobs(ZFEC_HIP_GRID_CAP=WALK_CAP)
    correct_once(code, case, cor, designed, [], name, (K, R, "walk"))


# ---- nothing skipped or sampled -------------------------------------------------------------------

def forms_of(test):
    (mark,) = [mk for mk in test.pytestmark if mk.name == "parametrize"]
    return list(mark.args[1])


def test_every_form_is_collected():
    """32 verify, 28 locate and 28 correct ids: every instantiation of
    matverify_reg and matlocate_reg is named by one of them."""
    v, l, c = forms_of(test_verify_form), forms_of(test_locate_form), forms_of(test_correct_form)
    assert (len(v), len(l), len(c)) == (32, 28, 28)
    assert {"matverify_reg<%d,%d>" % f for f in v} == {"matverify_reg<%d,%d>" % (K, R)
                                                      for K in (1, 2, 3, 4) for R in range(1, 9)}
    assert {"matlocate_reg<%d,%d>" % f for f in l} == {"matlocate_reg<%d,%d>" % (K, R)
                                                      for K in (1, 2, 3, 4) for R in range(2, 9)}
    assert l == c
