"""CPU model of pair location and correction (fec_locate2_batch,
fec_correct2_batch), shared by test_locate2_surface.py, test_gpu_locate2.py and
test_gpu_correct2.py.  Everything comes from the CPU oracle through locate_ref
and correct_ref (oracle_P, mul_table, inv_table); no library call feeds it.

With p_h column h of the c x nb matrix [P | I], the verdict of a stripe is two
words: rules 1-4 of locate_ref.verdicts give (CLEAN | UNKNOWN | slot, NONE);
where they say MANY and the pair pass is eligible (c >= 4, nb <= 32) the pair
(a, b), a < b, is refuted iff at some byte the syndrome vector is not in
span(p_a, p_b); exactly one pair left gives (a, b), anything else (MANY, NONE).
A pair verdict has slots a and b rewritten from the k lowest other slots by the
oracle's own check rows for those block numbers."""
import itertools

import numpy as np

from correct_ref import corrected
from locate_ref import CLEAN, MANY, UNKNOWN, inv_table, mul_table, syndromes, verdicts
from verify_ref import oracle_P

NONE = 0xFFFFFFFC


def eligible(k, c):
    return c >= 4 and k + c <= 32


def pair_index(nb, a, b):
    return a * nb - a * (a + 1) // 2 + (b - a - 1)


def columns(P):
    """[P | I], (c, nb)."""
    c = P.shape[0]
    return np.concatenate([P, np.eye(c, dtype=np.uint8)], axis=1)


def in_span(pa, pb, sig):
    """bool (n,): whether column x of sig (c, n) is a combination of pa and pb,
    by a 2 x 2 solve on two rows with a nonzero minor, checked on every row."""
    mul, inv = mul_table(), inv_table()
    c = len(pa)
    for r0, r1 in itertools.combinations(range(c), 2):
        det = int(mul[pa[r0], pb[r1]]) ^ int(mul[pa[r1], pb[r0]])
        if det:
            break
    else:
        raise AssertionError("dependent columns")
    idet = inv[det]
    x = mul[idet][mul[pb[r1]][sig[r0]] ^ mul[pb[r0]][sig[r1]]]
    y = mul[idet][mul[pa[r1]][sig[r0]] ^ mul[pa[r0]][sig[r1]]]
    ok = np.ones(sig.shape[1], dtype=bool)
    for i in range(c):
        ok &= sig[i] == (mul[pa[i]][x] ^ mul[pb[i]][y])
    return ok


def surviving_pairs(P, stripe):
    """The pairs no byte of `stripe` (nb, sz) refutes."""
    M = columns(P)
    sig = syndromes(P, stripe[None])[0]
    sig = np.ascontiguousarray(sig[:, sig.any(axis=0)])  # a zero syndrome vector lies in every span
    nb = M.shape[1]
    return [(a, b) for a, b in itertools.combinations(range(nb), 2) if in_span(M[:, a], M[:, b], sig).all()]


def verdicts2(P, Q, blocks, pass_on=None):
    """uint32 (2, ns): the two verdict planes of blocks (ns, k + c, sz)."""
    c, k = P.shape
    blocks = np.asarray(blocks, dtype=np.uint8)
    out = np.full((2, blocks.shape[0]), NONE, dtype=np.uint32)
    out[0] = verdicts(P, Q, blocks)
    if pass_on is None:
        pass_on = eligible(k, c)
    if not pass_on:
        return out
    for s in np.nonzero(out[0] == MANY)[0]:
        left = surviving_pairs(P, blocks[s])
        assert len(left) <= 1, ("more than one pair survives", int(s), left)
        if len(left) == 1:
            out[:, s] = left[0]
    return out


def pair_rows(k, m, nums, a, b):
    """(sources, rows (2, k)): the k lowest slots outside {a, b} and the
    oracle's check rows of blocks nums[a], nums[b] over those sources."""
    sources = [j for j in range(len(nums)) if j not in (a, b)][:k]
    rows = oracle_P(k, m, tuple([nums[j] for j in sources] + [nums[a], nums[b]]))
    return sources, rows


def corrected2(k, m, nums, P, Q, blocks):
    """(verdict planes (2, ns), blocks_after): single slots healed as
    correct_ref.corrected heals them, pairs from pair_rows."""
    mul = mul_table()
    blocks = np.asarray(blocks, dtype=np.uint8)
    v = verdicts2(P, Q, blocks)
    single, after = corrected(P, Q, blocks)
    assert (single[v[1] == NONE] == v[0][v[1] == NONE]).all()
    for s in np.nonzero(v[1] != NONE)[0]:
        a, b = int(v[0, s]), int(v[1, s])
        sources, rows = pair_rows(k, m, list(nums), a, b)
        for t, h in enumerate((a, b)):
            acc = np.zeros(blocks.shape[2], dtype=np.uint8)
            for l, j in enumerate(sources):
                acc ^= mul[rows[t, l]][blocks[s, j, :]]
            after[s, h, :] = acc
    return v, after
