"""A designed error matrix for the k <= 4 scrub kernels (matverify_reg<K,R>,
matlocate_reg<K,R>, matcorrect_reg<K>), shared by test_scrub_matrix.py (CPU)
and test_gpu_scrub_forms.py.  One stripe per case, so one call carries every
case, and every case has a verdict known by construction from P and Q (built
from the CPU oracle, locate_ref.oracle_PQ), not read off a model run:

  clean                 one untouched stripe                          CLEAN
  single                one byte of each of the K + R slots           that slot
  pair                  every (basis j, check i): K * R stripes,      MANY
                        alternately both at one byte and in different (UNKNOWN for
                        waves (bytes 0 and sz - 1, when sz > 1024)    R == 1)
  basis2                every pair of basis slots at one byte, random the model's
                        values                                        (None here)
  fooled2    (K >= 3)   for each j, e_a and e_b in two other basis    j for R == 2,
                        slots with s_1 = Q[1][j] . s_0                MANY for R >= 3
  fooledchk  (K >= 2)   for each j, e in basis a != j and             j for R == 2,
                        f = P[1][a].e ^ Q[1][j].P[0][a].e in check 1  MANY for R >= 3

A single error in basis slot j gives s_r = P[r][j] . e at that byte, so a pair
(j, i) breaks exactly row i of hypothesis j: a kernel that skipped or mis-read
row i of its Q tables for slot j names j where MANY is due.  The fooled cases
are the double errors that satisfy rows 0 and 1 of a wrong hypothesis: two
checks miscorrect them, a third refuses them (README).  Byte positions cycle
through the first byte, the last byte, the last full chunk, the tail, a middle
lane of wave 0 and a lane of the last wave.

With R == 1 (verify only) there are no fooled cases and every dirty stripe is
UNKNOWN."""
import numpy as np

from locate_ref import CLEAN, MANY, UNKNOWN
from verify_ref import mul_table

KINDS = ("clean", "single", "pair", "basis2", "fooled2", "fooledchk")


def positions(sz):
    """The byte positions the cases cycle through, all inside [0, sz)."""
    cps = (sz + 15) // 16
    wps = (cps + 63) // 64
    last_full = 16 * (sz // 16 - 1) + 5 if sz >= 16 else sz // 2
    tail = sz - sz % 16 if sz % 16 and sz > 16 else max(0, sz - 16)
    mid_lane = 16 * min(31, cps - 1) + 7
    last_wave = 16 * min(64 * (wps - 1) + 1, cps - 1) + 3
    return [min(max(int(x), 0), sz - 1) for x in (0, sz - 1, last_full, tail, mid_lane, last_wave)]


def survivors(Q, syn):
    """Basis slots j whose hypothesis the syndromes `syn` (R,) of one byte do
    not refute: syn[r] == Q[r-1][j] . syn[0] for every r >= 1."""
    mul = mul_table()
    return [j for j in range(Q.shape[1]) if all(syn[r] == mul[Q[r - 1, j], syn[0]] for r in range(1, len(syn)))]


def gf_div(a, b):
    (q,) = np.nonzero(mul_table()[b] == a)[0]
    return int(q)


def error_matrix(K, R, P, Q, sz, rng):
    """(corruptions, designed, kinds) of one call: corruptions is a list of
    (stripe, slot, positions, xor values) as test_gpu_locate.patterns builds
    them, designed[s] the verdict of stripe s by construction (None where only
    the model knows), kinds[s] one of KINDS."""
    mul = mul_table()
    P = np.asarray(P, dtype=np.uint8)
    assert P.shape == (R, K) and P.all()
    assert R == 1 or Q.shape == (R - 1, K)
    pos = positions(sz)
    cor, designed, kinds = [], [], []
    turn = [0]

    def nz():
        return int(rng.integers(1, 256))

    def place():
        turn[0] += 1
        return pos[(turn[0] - 1) % len(pos)]

    def one(s, slot, x, v):
        assert 0 <= x < sz and 0 < v < 256 and 0 <= slot < K + R
        return (s, slot, np.array([x]), np.array([v], dtype=np.uint8))

    def stripe(kind, verdict, errors):
        s = len(designed)
        cor.extend(one(s, slot, x, v) for slot, x, v in errors)
        designed.append(verdict)
        kinds.append(kind)

    dirty = UNKNOWN if R == 1 else None
    stripe("clean", CLEAN, [])
    for slot in range(K + R):
        stripe("single", dirty if R == 1 else slot, [(slot, place(), nz())])
    n = 0
    for j in range(K):
        for i in range(R):
            e, x = nz(), place()
            if n % 2 == 1 and sz > 1024:
                # different waves: each sees a single-slot error, only the OR gives MANY
                errors = [(j, 0, e), (K + i, sz - 1, nz())]
            else:
                # one byte: f must not cancel row i, and (R == 2) must leave no slot standing
                while True:
                    f = nz()
                    syn = np.array([mul[P[r, j], e] ^ (f if r == i else 0) for r in range(R)], dtype=np.uint8)
                    if R == 1:
                        if syn[0]:
                            break
                    elif np.count_nonzero(syn) >= 2 and not survivors(Q, syn):
                        break
                errors = [(j, x, e), (K + i, x, f)]
            n += 1
            stripe("pair", dirty if R == 1 else MANY, errors)
    for a in range(K):
        for b in range(a + 1, K):
            x = place()
            stripe("basis2", None, [(a, x, nz()), (b, x, nz())])
    if R >= 2:
        fooled = lambda j: j if R == 2 else MANY  # noqa: E731
        if K >= 3:
            for j in range(K):
                a, b = (j + 1) % K, (j + 2) % K
                q, ea, x = int(Q[0, j]), nz(), place()
                eb = gf_div(mul[ea, P[1, a] ^ mul[q, P[0, a]]], mul[q, P[0, b]] ^ P[1, b])
                stripe("fooled2", fooled(j), [(a, x, ea), (b, x, eb)])
        if K >= 2:
            for j in range(K):
                a = (j + 1) % K
                q, e, x = int(Q[0, j]), nz(), place()
                f = int(mul[P[1, a], e] ^ mul[q, mul[P[0, a], e]])
                stripe("fooledchk", fooled(j), [(a, x, e), (K + 1, x, f)])
    return cor, designed, kinds


def pair_of(K, R, s):
    """(basis j, check i) of stripe s when it is a pair stripe, else None."""
    p = s - (1 + K + R)
    return divmod(p, R) if 0 <= p < K * R else None


def form_bases(K, R):
    """The slots of form <K,R>: the first K + R block numbers of the all-parity
    and of the mixed basis of code (K, K + 8), so checks include primaries."""
    from test_gpu_verify import bases
    return [(name, nums[:K + R]) for name, nums in bases(K, K + 8, seed=40 * K) if name in ("parity", "mixed")]


def wave_walk(cap, sz, ns):
    """(wps, gs_s, gs_w, steps) of `cap` workgroups of four waves walking ns
    stripes of sz bytes, by the arithmetic of the launcher (kernels.hip
    fill_walk): a wave's 64 chunks of 16 bytes lie in one stripe, so a stripe
    has wps waves and a step of 4 * cap waves is gs_s stripes and gs_w waves.
    The carry (w >= wps) runs only where gs_w != 0; steps is the fewest
    iterations a wave makes.  As guarded_batch.walk_steps, both are asserted."""
    cps = (sz + 15) // 16
    wps = (cps + 63) // 64
    waves = ns * wps
    assert (waves + 3) // 4 > cap, "the launch is not capped"
    step = 4 * cap
    gs_s, gs_w = divmod(step, wps)
    assert gs_w != 0, "gs_w == 0: the walk never carries"
    steps = waves // step
    assert steps >= 3, (waves, step)
    return wps, gs_s, gs_w, steps


def matrix_size(K, R):
    """Stripes error_matrix(K, R, ...) returns."""
    n = 1 + (K + R) + K * R + K * (K - 1) // 2
    if R >= 2:
        n += (K if K >= 3 else 0) + (K if K >= 2 else 0)
    return n


def select(cor, designed, kinds, keep):
    """The stripes s with keep(s, kinds[s]) true, renumbered from 0."""
    new = {}
    for s, kind in enumerate(kinds):
        if keep(s, kind):
            new[s] = len(new)
    return ([(new[s], j, xs, vs) for s, j, xs, vs in cor if s in new], [designed[s] for s in new],
            [kinds[s] for s in new])


def flat(cor):
    """The corruption list as test_gpu_verify takes it: (stripe, slot, byte, xor value)."""
    return [(s, j, int(x), int(v)) for s, j, xs, vs in cor for x, v in zip(xs, vs)]


def blocks_of(cor, ns, nb, sz, clean=None):
    """(ns, nb, sz) blocks: zeros (the model is linear) or `clean`, corrupted."""
    blocks = np.zeros((ns, nb, sz), dtype=np.uint8) if clean is None else clean.copy()
    for s, j, xs, vs in cor:
        blocks[s, j, xs] ^= vs
    return blocks
