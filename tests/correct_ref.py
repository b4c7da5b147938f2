"""CPU model of the batched in-place correction (fec_correct_batch), shared by
test_correct_surface.py and test_gpu_correct.py.  Everything comes from the CPU
oracle through locate_ref (oracle_PQ, mul_table, inv_table); no library call
feeds it.

A stripe whose verdict (locate_ref.verdicts) is a slot h < nb has slot h
rewritten from k other slots: the sources S_h are slots 0..k-1 for h >= k; for
h < k they are 0..k-1 with slot h replaced by slot k (check 0).  The row
applied, in the order of S_h, is P[h-k] for h >= k and, for h < k,
R[l] = P[0][l] / P[0][h] for l != h, R[h] = 1 / P[0][h]: check 0's equation
solved for slot h.  Every other stripe stays as it is."""
import numpy as np

from locate_ref import inv_table, mul_table, verdicts


def correct_rows(P):
    """(R, S): R (nb, k) uint8, row h the coefficients applied to the slots
    S[h] (a list of k slot indices), by the definition above."""
    mul, inv = mul_table(), inv_table()
    c, k = P.shape
    R = np.zeros((k + c, k), dtype=np.uint8)
    S = []
    for h in range(k + c):
        if h >= k:
            R[h] = P[h - k]
            S.append(list(range(k)))
            continue
        ih = inv[P[0, h]]
        for l in range(k):
            R[h, l] = ih if l == h else mul[P[0, l], ih]
        S.append([k if l == h else l for l in range(k)])
    return R, S


def corrected(P, Q, blocks):
    """(verdicts (ns,) uint32, blocks_after (ns, k + c, sz)): the verdicts of
    the blocks as given, then the culprit slot of every slot-verdict stripe
    recomputed with the oracle's GF products."""
    mul = mul_table()
    c, k = P.shape
    blocks = np.asarray(blocks, dtype=np.uint8)
    v = verdicts(P, Q, blocks)
    after = blocks.copy()
    if blocks.shape[2] == 0:
        return v, after
    R, S = correct_rows(P)
    for s in np.nonzero(v < k + c)[0]:
        h = int(v[s])
        acc = np.zeros(blocks.shape[2], dtype=np.uint8)
        for l in range(k):
            acc ^= mul[R[h, l]][blocks[s, S[h][l], :]]
        after[s, h, :] = acc
    return v, after
