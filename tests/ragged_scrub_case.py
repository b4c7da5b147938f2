"""Shared by test_ragged_scrub_surface.py (CPU) and test_gpu_ragged_scrub.py:
one ragged scrub call (fec_verify_batch_ragged / fec_locate_batch_ragged) laid
out on the host, and the mismatch bits and verdicts the CPU model expects of it.

The arena follows ragged_case.py: the base handed to the library is IN_OFF = 5
bytes into the source tensor, the tensor holds BACKGROUND (0x3C) wherever no
block lies, and in the packed layouts stripes are placed with a gap of
13 + (s % 3) bytes, so that a read past a stripe's end meets bytes that are not
its neighbour's and shows up as a false mismatch.

The expectation is per stripe and comes from the CPU model alone: the nb
blocks are the oracle's encoding (oracle.encode), the corruptions are applied
to them, and stripe s's bits and verdict are locate_ref.bits and
locate_ref.verdicts on its (1, nb, sz) array with P and Q from
locate_ref.oracle_PQ.  No library call feeds it.  Stripes that hold no
corruption are judged together, as one long stripe (the arithmetic is
bytewise): the model must find no syndrome in them, which makes each of them
clean."""
import numpy as np

from oracle import oracle

import locate_ref
import ragged_case as rc
from ragged_case import BACKGROUND, IN_OFF, gap  # noqa: F401  (re-exported for the tests)

TAIL = 64
CLEAN, MANY, UNKNOWN, UNFIT = locate_ref.CLEAN, locate_ref.MANY, locate_ref.UNKNOWN, 0xFFFFFFFB
NUMS = [7, 0, 4, 1, 9, 2, 5]  # K=3/M=10: basis 7, 0, 4; checks 1, 9, 2, 5


def positions(sz):
    """The byte positions a test cycles its corruptions through, where they exist."""
    return [p for p in (0, sz - 1, 1023, 1024, sz - 17) if 0 <= p < sz]


class ScrubCase(object):
    """nums: the block in every slot (the first k the basis).  corrupt: a list
    of (stripe, slot, byte, xor) applied to the stored blocks.  layout "packed"
    (block stride 0, stripes in order), "shuffled" (the same, the stripes
    placed in the arena in the order `place`) or "block" (a fixed block stride
    of total + 7, offsets the prefix sum of the sizes)."""

    def __init__(self, k, m, nums, sizes, corrupt=(), layout="packed", place=None, seed=0):
        self.k, self.m, self.nums, self.layout = k, m, list(nums), layout
        self.nb = nb = len(self.nums)
        self.c = c = nb - k
        self.words = (c + 31) // 32
        self.sizes = [int(x) for x in sizes]
        self.ns = ns = len(self.sizes)
        total = sum(self.sizes)
        data = np.random.default_rng(seed).integers(0, 256, size=(k, total), dtype=np.uint8)
        blocks = np.ascontiguousarray(np.concatenate([data, oracle.encode(k, m, data)])[self.nums])
        start = np.cumsum([0] + self.sizes)
        self.corrupt = [(int(s), int(j), int(p), int(x)) for s, j, p, x in corrupt]
        for s, j, p, x in self.corrupt:
            assert 0 <= s < ns and 0 <= j < nb and 0 <= p < self.sizes[s] and 0 < x < 256, (s, j, p, x)
            blocks[j, int(start[s]) + p] ^= x
        # the model's bits and verdicts
        P, Q = locate_ref.oracle_PQ(k, m, tuple(self.nums))
        self.bits = np.zeros((ns, c), dtype=bool)
        self.verdict = np.full(ns, CLEAN, dtype=np.uint32)
        dirty = sorted(set(s for s, _, _, _ in self.corrupt))
        keep = np.ones(total, dtype=bool)
        for s in dirty:
            a, b = int(start[s]), int(start[s + 1])
            keep[a:b] = False
            one = blocks[:, a:b].reshape(1, nb, b - a)
            self.bits[s] = locate_ref.bits(P, Q, one)[0][0]
            self.verdict[s] = locate_ref.verdicts(P, Q, one)[0]
        rest = np.ascontiguousarray(blocks[:, keep]).reshape(1, nb, -1)
        if rest.shape[2]:
            assert not locate_ref.bits(P, Q, rest)[0].any(), "the model finds a syndrome in uncorrupted stripes"
        # the arena
        if layout == "block":
            self.sbs = total + 7
            self.soff = [int(x) for x in start[:-1]]
            in_len = (nb - 1) * self.sbs + total
        else:
            self.sbs = 0
            order = list(range(ns)) if layout == "packed" else list(place)
            assert sorted(order) == list(range(ns))
            self.soff = [0] * ns
            a = 0
            for s in order:
                self.soff[s] = a
                a += nb * self.sizes[s] + gap(s)
            in_len = a
        self.src_bytes = in_len
        self.src = np.full(IN_OFF + in_len + TAIL, BACKGROUND, dtype=np.uint8)
        for s, sz in enumerate(self.sizes):
            a, b = int(start[s]), int(start[s + 1])
            for j in range(nb):
                o = IN_OFF + self.soff[s] + j * (self.sbs or sz)
                self.src[o:o + sz] = blocks[j, a:b]
        self.src.setflags(write=False)

    def stripe_blocks(self, s):
        """(1, nb, sz): stripe s as the arena holds it."""
        sz = self.sizes[s]
        return np.stack([self.src[IN_OFF + self.soff[s] + j * (self.sbs or sz):][:sz]
                         for j in range(self.nb)]).reshape(1, self.nb, sz)

    @property
    def want_words(self):
        """The W mismatch words per stripe, (ns, W) uint32."""
        out = np.zeros((self.ns, self.words), dtype=np.uint32)
        for i in range(self.c):
            out[:, i // 32] |= self.bits[:, i].astype(np.uint32) << np.uint32(i % 32)
        return out

    def all_bits(self):
        """The words of a stripe every check of which is set (an unfit stripe)."""
        return np.array([(1 << min(32, self.c - 32 * w)) - 1 for w in range(self.words)], dtype=np.uint32)


def third_corrupt(sizes, nb, seed):
    """A third of the nonempty stripes (s % 3 == 1) with one to three random
    (slot, byte) corruptions each: single blocks, pairs and triples."""
    rng = np.random.default_rng(seed)
    out = []
    for s, sz in enumerate(sizes):
        if sz and s % 3 == 1:
            for _ in range(1 + (s // 3) % 3):
                out.append((s, int(rng.integers(0, nb)), int(rng.integers(0, sz)), int(rng.integers(1, 256))))
    return out


def cycled_corrupt(sizes, nb, last_byte_of=None):
    """One flipped byte in every nonempty stripe with s % 3 != 0, the position
    cycling through positions(sz) and the slot through all nb slots; a stripe
    of last_byte_of bytes has its last byte flipped."""
    out, n = [], 0
    for s, sz in enumerate(sizes):
        if sz and s % 3:
            pos = positions(sz)
            out.append((s, n % nb, sz - 1 if sz == last_byte_of else pos[n % len(pos)], 1 + (37 * n) % 255))
            n += 1
    return out


__all__ = ["ScrubCase", "third_corrupt", "cycled_corrupt", "positions", "rc"]
