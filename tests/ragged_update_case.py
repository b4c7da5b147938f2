"""Shared by test_ragged_update_surface.py (CPU) and test_gpu_ragged_update.py:
one ragged parity update (fec_update_batch_ragged) laid out on the host, and
the whole row arena the CPU oracle expects of it.

The arenas follow ragged_case.py: the base handed to the library is IN_OFF = 5
bytes into the input tensors and OUT_OFF = 3 into the row tensor; the inputs
hold BACKGROUND wherever no slot lies and must come back unchanged; the row
arena holds the stripes' stored blocks BEFORE the change, with GUARD in every
gap and in the tail.  `rows0` is that arena and `want` the whole arena after
the call -- so one comparison checks the updated rows, the rows that are to be
left alone, the gaps and the tail.

Expected bytes come from the CPU oracle alone: random primaries are encoded,
the live slots' deltas XOR-ed into the primaries they name, and the result
encoded again (the arithmetic is bytewise, so the batch is one long stripe).
A none slot carries random bytes that must not matter."""
import numpy as np

from oracle import oracle

import ragged_case as rc
from ragged_case import BACKGROUND, GUARD, IN_OFF, OUT_OFF, TAIL, gap  # noqa: F401  (re-exported for the tests)

NONE = -1


def all_blocks(k, m, data):
    """(m, n) from the primaries (k, n): the primaries, then the oracle's parity."""
    if data.shape[1] == 0:
        return np.zeros((m, 0), dtype=np.uint8)
    return np.concatenate([data, oracle.encode(k, m, np.ascontiguousarray(data))])


class UpdateCase(object):
    """sizes [ns]; nums: the block number of every stored row; changed [ns][c]
    (NONE = -1); form "delta" (new holds old ^ new) or "oldnew".  layout
    "packed" (block stride 0 on both sides, stripes in order), "shuffled" (the
    same, stripes placed in the order `place`) or "block" (fixed block
    strides, offsets the prefix sum of the sizes).  skip: stripes the call is
    to leave alone, dead: (stripe, slot) pairs it is to take for none (a test
    spoils their descriptor or number afterwards)."""

    def __init__(self, k, m, sizes, nums, changed, form="delta", layout="packed", place=None, seed=0, skip=(),
                 dead=()):
        self.k, self.m, self.form, self.layout = k, m, form, layout
        self.sizes = [int(x) for x in sizes]
        self.nums = [int(x) for x in nums]
        ch = np.asarray(changed, dtype=np.int64)
        self.changed = ch.reshape(len(self.sizes), ch.shape[1] if ch.ndim == 2 else 1)
        self.ns = ns = len(self.sizes)
        self.c = c = self.changed.shape[1]
        self.r = r = len(self.nums)
        total = sum(self.sizes)
        rng = np.random.default_rng([k, m, ns, c, seed])
        data = rng.integers(0, 256, size=(k, total), dtype=np.uint8)
        deltas = rng.integers(0, 256, size=(c, total), dtype=np.uint8)
        junk = rng.integers(0, 256, size=(c, total), dtype=np.uint8)
        old = rng.integers(0, 256, size=(c, total), dtype=np.uint8)
        start = np.cumsum([0] + self.sizes)
        after = data.copy()
        live = np.zeros((c, total), dtype=bool)
        for s in range(ns):
            a, b = int(start[s]), int(start[s + 1])
            for i in range(c):
                j = int(self.changed[s, i])
                if j != NONE:
                    live[i, a:b] = True
                    if s not in skip and (s, i) not in dead:
                        after[j, a:b] ^= deltas[i, a:b]
        before_rows = all_blocks(k, m, data)[self.nums]
        after_rows = all_blocks(k, m, after)[self.nums]
        if form == "delta":
            new, old = np.where(live, deltas, junk), None
        else:
            new = np.where(live, old ^ deltas, junk)
        if layout == "block":
            self.ibs, self.rbs = total + 7, total + 11
            self.ioff = [int(x) for x in start[:-1]]
            self.roff = list(self.ioff)
            in_len, row_len = (c - 1) * self.ibs + total, (r - 1) * self.rbs + total
        else:
            self.ibs = self.rbs = 0
            order = list(range(ns)) if layout == "packed" else list(place)
            assert sorted(order) == list(range(ns))
            self.ioff, self.roff = [0] * ns, [0] * ns
            a = b = 0
            for s in order:
                self.ioff[s], self.roff[s] = a, b
                a += c * self.sizes[s] + gap(s)
                b += r * self.sizes[s] + gap(s)
            in_len, row_len = a, b
        self.in_bytes, self.row_bytes = in_len, row_len
        self.newb = np.full(IN_OFF + in_len + TAIL, BACKGROUND, dtype=np.uint8)
        self.oldb = self.newb.copy() if old is not None else None
        self.rows0 = np.full(OUT_OFF + row_len + TAIL, GUARD, dtype=np.uint8)
        self.want = self.rows0.copy()
        for s, sz in enumerate(self.sizes):
            a, b = int(start[s]), int(start[s + 1])
            for i in range(c):
                o = IN_OFF + self.ioff[s] + i * (self.ibs or sz)
                self.newb[o:o + sz] = new[i, a:b]
                if old is not None:
                    self.oldb[o:o + sz] = old[i, a:b]
            for i in range(r):
                o = OUT_OFF + self.roff[s] + i * (self.rbs or sz)
                self.rows0[o:o + sz] = before_rows[i, a:b]
                self.want[o:o + sz] = after_rows[i, a:b]
        for a in (self.newb, self.oldb, self.rows0, self.want):
            if a is not None:
                a.setflags(write=False)

    def row_spans(self, s):
        """[begin, end) of every stored row of stripe s in the row tensor."""
        sz = self.sizes[s]
        return [(OUT_OFF + self.roff[s] + i * (self.rbs or sz), OUT_OFF + self.roff[s] + i * (self.rbs or sz) + sz)
                for i in range(self.r)]

    def explain(self, got):
        """What differs from `want`: the first wrong (stripe, row, size, first
        wrong byte of the row) tuples, and the wrong bytes outside every row."""
        bad = np.flatnonzero(got != self.want)
        if not bad.size:
            return None
        inside = np.zeros(got.shape, dtype=bool)
        wrong = []
        for s in range(self.ns):
            for i, (a, b) in enumerate(self.row_spans(s)):
                inside[a:b] = True
                d = np.flatnonzero(got[a:b] != self.want[a:b])
                if d.size:
                    wrong.append((s, i, self.sizes[s], int(d[0])))
        stray = bad[~inside[bad]]
        return ("wrong (stripe, row, size, first byte)", wrong[:8], "bytes written outside the rows",
                stray[:8].tolist())


__all__ = ["UpdateCase", "NONE", "all_blocks", "rc"]
