"""CPU model of single-block error location (fec_locate_batch), shared by
test_locate_surface.py and test_gpu_locate.py.  Everything comes from the CPU
oracle (verify_ref.oracle_P, oracle.gf_mul); no library call feeds it.

Slot j of a stripe holds block nums[j], the first k slots the basis, the other
c the checks.  With P = E[checks] . inverse(E[basis]) the syndromes at every
byte are s_i = stored check i ^ sum_j P[i][j] . basis_j, and for c >= 2
Q[i][j] = P[i][j] / P[0][j], i = 1..c-1.  Per stripe: mismatch bit i iff
s_i != 0 somewhere; excluded bit j iff s_i != Q[i][j] . s_0 somewhere for some
i >= 1.  The verdict: no mismatch bit -> CLEAN; c == 1 -> UNKNOWN; exactly one
mismatch bit i0 -> slot k + i0; exactly one basis slot not excluded -> that
slot; else MANY."""
import functools

import numpy as np

from verify_ref import mul_table, oracle_P

CLEAN, MANY, UNKNOWN = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD


@functools.lru_cache(maxsize=None)
def inv_table():
    """inv[a] for a != 0, read off the oracle's products; inv[0] = 0."""
    mul = mul_table()
    inv = np.zeros(256, dtype=np.uint8)
    for a in range(1, 256):
        (b,) = np.nonzero(mul[a] == 1)[0]
        inv[a] = b
    inv.setflags(write=False)
    return inv


@functools.lru_cache(maxsize=None)
def oracle_PQ(k, m, nums):
    """(P, Q) of the block numbers `nums` (a tuple): P (c, k) with no zero
    entry, Q (c - 1, k)."""
    P = oracle_P(k, m, nums)
    assert P.all(), ("P has a zero entry", nums)
    mul, inv = mul_table(), inv_table()
    Q = np.zeros((P.shape[0] - 1, k), dtype=np.uint8)
    for i in range(1, P.shape[0]):
        Q[i - 1] = mul[P[i], inv[P[0]]]
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


def syndromes(P, blocks):
    """(ns, c, sz) from blocks (ns, k + c, sz)."""
    mul = mul_table()
    c, k = P.shape
    sig = blocks[:, k:, :].copy()
    for i in range(c):
        for j in range(k):
            sig[:, i, :] ^= mul[P[i, j]][blocks[:, j, :]]
    return sig


def bits(P, Q, blocks):
    """(mismatch (ns, c), excluded (ns, k)) bool arrays of the definition."""
    mul = mul_table()
    c, k = P.shape
    sig = syndromes(P, blocks)
    mismatch = sig.any(axis=2)
    excluded = np.zeros((blocks.shape[0], k), dtype=bool)
    dirty = np.nonzero(mismatch.any(axis=1))[0]  # a stripe whose syndromes are all zero refutes nothing
    for j in range(k):
        for i in range(1, c):
            excluded[dirty, j] |= (sig[dirty, i, :] != mul[Q[i - 1, j]][sig[dirty, 0, :]]).any(axis=1)
    return mismatch, excluded


def verdicts(P, Q, blocks):
    """uint32 (ns,): rules 1-5 applied to full blocks (ns, k + c, sz)."""
    c, k = P.shape
    blocks = np.asarray(blocks, dtype=np.uint8)
    ns = blocks.shape[0]
    out = np.full(ns, CLEAN, dtype=np.uint32)
    if blocks.shape[2] == 0:
        return out
    mismatch, excluded = bits(P, Q, blocks)
    for s in range(ns):
        bad = np.nonzero(mismatch[s])[0]
        if len(bad) == 0:
            continue
        if c == 1:
            out[s] = UNKNOWN
            continue
        left = np.nonzero(~excluded[s])[0]
        assert len(left) <= 1, ("more than one basis slot survives", s, left.tolist())
        if len(bad) == 1:
            out[s] = k + bad[0]
        elif len(left) == 1:
            out[s] = left[0]
        else:
            out[s] = MANY
    return out
