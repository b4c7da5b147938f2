"""CPU check of the designed error matrix (tests/scrub_matrix.py) that
test_gpu_scrub_forms.py feeds to every matverify_reg / matlocate_reg /
matcorrect_reg form: for every K in 1..4, every R in 1..8 and both bases the
numpy model of the definition (tests/locate_ref.py) gives exactly the verdicts
the matrix was designed for, on zero data (the model is linear).  It also shows
that the matrix pins what it is meant to pin: a model that leaves out any one
row r >= 1 of the hypothesis tests, or every row >= 2, answers differently on
it.  Last, a model of the wave walk shows that the three geometries of
test_gpu_wave_walk.py take the carry in every wave, that a walk without the
carry loses units there, and that the older grid-stride tests never carried.
No GPU and no library call."""
import numpy as np
import pytest

from locate_ref import CLEAN, MANY, UNKNOWN, oracle_PQ, syndromes, verdicts
from scrub_matrix import KINDS, blocks_of, error_matrix, form_bases, matrix_size, pair_of, positions, wave_walk
from verify_ref import mul_table

SIZES = (15, 17, 1024, 1025, 4097)
FORMS = [(K, R) for K in range(1, 5) for R in range(1, 9)]


def verdicts_with_rows(P, Q, blocks, rows):
    """locate_ref's rules with the hypotheses tested against `rows` only (a
    subset of 1..c-1): the model of a kernel that skips the others."""
    mul = mul_table()
    c, k = P.shape
    sig = syndromes(P, blocks)
    out = np.full(blocks.shape[0], CLEAN, dtype=np.uint32)
    for s in range(blocks.shape[0]):
        bad = np.nonzero(sig[s].any(axis=1))[0]
        if len(bad) == 0:
            continue
        left = [j for j in range(k)
                if not any((sig[s, i] != mul[Q[i - 1, j]][sig[s, 0]]).any() for i in rows)]
        out[s] = k + bad[0] if len(bad) == 1 else left[0] if len(left) == 1 else MANY
    return out


def walk_visits(cap, sz, ns, carry=True, limit=1000):
    """How often each (stripe, wave) unit is visited when 4 * cap waves walk as
    the kernels do (gw -> (s, w); w += gs_w; s += gs_s; the carry), how many
    carries were taken, and whether every wave left its loop within `limit`
    iterations.  A wave whose w is past wps has no live lane."""
    wps, gs_s, gs_w, steps = wave_walk(cap, sz, ns)
    seen = np.zeros((ns, wps), dtype=np.int64)
    carries, ended = 0, True
    for gw in range(4 * cap):
        s, w = divmod(gw, wps)
        n = 0
        while s < ns and n < limit:
            if w < wps:
                seen[s, w] += 1
            w += gs_w
            s += gs_s
            if carry and w >= wps:
                w -= wps
                s += 1
                carries += 1
            n += 1
        ended = ended and s >= ns
        assert not carry or n >= steps
    return seen, carries, ended


GEOMETRIES = [(3, 4097, (5, 2, 2)), (1, 4097, (5, 0, 4)), (5, 6160, (7, 2, 6))]


@pytest.mark.parametrize("cap,sz,step", GEOMETRIES)
def test_walk_geometries_take_the_carry(cap, sz, step):
    """The three geometries of test_gpu_wave_walk.py on 37 stripes: with the
    carry every unit is visited exactly once and every wave carries; without it
    units are lost (or, where a step is shorter than a stripe, no wave ends)."""
    ns = 37
    assert wave_walk(cap, sz, ns)[:3] == step
    seen, carries, ended = walk_visits(cap, sz, ns)
    assert ended and (seen == 1).all() and carries >= 4 * cap
    seen, carries, ended = walk_visits(cap, sz, ns, carry=False)
    assert (seen == 0).any() and ended == (step[1] != 0)


@pytest.mark.parametrize("cap,sz", [(3, 2049), (2, 1040), (2, 4096)])
def test_the_older_grid_stride_geometries_never_carry(cap, sz):
    """test_grid_stride of test_gpu_verify / locate / correct (cap 3, 2049
    bytes) and of test_gpu_mixed / repair (cap 2, 1040 and 4096 bytes): a step
    is a whole number of stripes."""
    with pytest.raises(AssertionError, match="gs_w == 0"):
        wave_walk(cap, sz, 37)


def build(K, R, nums, sz, seed):
    P, Q = oracle_PQ(K, K + 8, tuple(nums))
    cor, designed, kinds = error_matrix(K, R, P, Q, sz, np.random.default_rng(seed))
    return P, Q, cor, designed, kinds


def test_positions_are_the_documented_ones():
    assert positions(4097) == [0, 4096, 4085, 4096, 503, 4096]
    assert positions(6160) == [0, 6159, 6149, 6144, 503, 6147]
    assert positions(1025) == [0, 1024, 1013, 1024, 503, 1024]
    assert positions(1024) == [0, 1023, 1013, 1008, 503, 19]
    assert positions(17) == [0, 16, 5, 16, 16, 16]
    assert positions(15) == [0, 14, 7, 0, 7, 3]


@pytest.mark.parametrize("K,R", FORMS)
def test_model_gives_the_designed_verdicts(K, R):
    for bname, nums in form_bases(K, R):
        assert len(nums) == K + R and any(b >= K for b in nums[:K])  # a parity block in the basis
        assert R < 8 or any(b < K for b in nums[K:])                  # and a primary among all 8 checks
        for sz in SIZES:
            P, Q, cor, designed, kinds = build(K, R, nums, sz, seed=sz + R)
            ns = len(designed)
            assert ns == matrix_size(K, R) <= 70 and set(kinds) <= set(KINDS)
            got = verdicts(P, Q, blocks_of(cor, ns, K + R, sz))
            for s in range(ns):
                if designed[s] is not None:
                    assert got[s] == designed[s], (bname, sz, s, kinds[s], hex(got[s]), designed[s])
            assert kinds.count("single") == K + R and kinds.count("pair") == K * R
            assert sorted(pair_of(K, R, s) for s in range(ns) if kinds[s] == "pair") == \
                [(j, i) for j in range(K) for i in range(R)]
            if R == 1:
                # (two basis errors at one byte may cancel in a single check)
                assert all(got[s] == UNKNOWN for s in range(1, ns) if kinds[s] != "basis2")
                continue
            assert {CLEAN, MANY} | set(range(K + R)) <= set(got.tolist())
            if K >= 3:
                assert kinds.count("fooled2") == K
            if K >= 2:
                assert kinds.count("fooledchk") == K
            fooled = [s for s in range(ns) if kinds[s].startswith("fooled")]
            if R == 2:  # miscorrected with two checks: every basis slot is named by a double error
                assert sorted({int(got[s]) for s in fooled}) == (list(range(K)) if K >= 2 else [])
            else:       # refused with three
                assert all(got[s] == MANY for s in fooled)


@pytest.mark.parametrize("K,R", [(K, R) for K, R in FORMS if R >= 3])
def test_every_hypothesis_row_is_pinned(K, R):
    """Leaving out row r of the hypothesis tests names basis slot j on the pair
    (j, check r) for every j; testing row 1 alone names the wrong slot on every
    fooled case."""
    for bname, nums in form_bases(K, R):
        for sz in (17, 4097):
            P, Q, cor, designed, kinds = build(K, R, nums, sz, seed=sz + R)
            ns = len(designed)
            blocks = blocks_of(cor, ns, K + R, sz)
            want = verdicts(P, Q, blocks)
            assert (verdicts_with_rows(P, Q, blocks, range(1, R)) == want).all()
            for r in range(1, R):
                got = verdicts_with_rows(P, Q, blocks, [i for i in range(1, R) if i != r])
                wrong = {pair_of(K, R, s) for s in np.nonzero(got != want)[0] if kinds[s] == "pair"}
                assert {(j, r) for j in range(K)} <= wrong, (bname, sz, r, sorted(wrong))
            got = verdicts_with_rows(P, Q, blocks, [1])
            fooled = [s for s in range(ns) if kinds[s].startswith("fooled")]
            assert len(fooled) == (2 * K if K >= 3 else K if K == 2 else 0)
            assert all(got[s] < K and want[s] == MANY for s in fooled), (bname, sz)
