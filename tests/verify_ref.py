"""CPU reference of the parity verification (fec_verify_batch), shared by
test_verify_surface.py and test_gpu_verify.py: the matrix
P = E[checks] . inverse(E[basis]) and GF(2^8) matrix products, built from the
CPU oracle only (oracle.enc_matrix, oracle_invert_mat, oracle.gf_mul)."""
import functools

import numpy as np

from oracle import oracle


@functools.lru_cache(maxsize=None)
def mul_table():
    """256 x 256 products: one oracle.gf_mul per pair, then numpy indexing."""
    t = np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    t.setflags(write=False)
    return t


def gf_matmul(a, b):
    """a (r, k) times b (k, n) over GF(2^8)."""
    mul = mul_table()
    a = np.asarray(a, dtype=np.uint8)
    b = np.asarray(b, dtype=np.uint8)
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.uint8)
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            out[i] ^= mul[a[i, j]][b[j]]
    return out


def oracle_P(k, m, nums):
    """(c, k): the check rows of block numbers `nums` (first k the basis)."""
    nums = list(nums)
    enc = oracle.enc_matrix(k, m)
    inv = np.ascontiguousarray(enc[nums[:k]])
    assert oracle.lib().oracle_invert_mat(oracle._u8(inv), k) == 0, "singular basis"
    return gf_matmul(enc[nums[k:]], inv)
