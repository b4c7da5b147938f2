"""Shared by test_ragged_repair_surface.py (CPU), test_gpu_ragged_repair.py and
test_gpu_ragged_correct.py: one ragged repair call (fec_repair_batch_ragged)
laid out on the host with the whole output arena the CPU oracle expects of it,
and the writable arena of a ragged correction (fec_correct_batch_ragged).

The arenas follow ragged_case.py: the base handed to the library is IN_OFF = 5
bytes into the source tensor and OUT_OFF = 3 into the output tensor, the
source holds BACKGROUND wherever no block lies, the output is pre-filled with
GUARD, and `want` is the WHOLE output arena -- GUARD everywhere but in the rows
that are to be written -- so one comparison checks the rows, the rows of NONE
targets, the gaps, the stripes that are to be skipped and the tail.

Expected bytes come from the CPU oracle alone, per pattern over that pattern's
stripes taken as one long stripe (the arithmetic is bytewise): the present
blocks are put into the slot order the oracle's decode wants (primary i at
slot i), decoded to the k primaries -- which must equal the data -- and each
target is the primary itself or the oracle's encoding of it."""
import numpy as np

from oracle import oracle

import ragged_case as rc
from ragged_case import BACKGROUND, GUARD, IN_OFF, OUT_OFF, TAIL, gap  # noqa: F401  (re-exported for the tests)

NONE = -1

# K=3/M=10, three targets: present sets and slot orders differ, pattern 2 is
# parity only; live-row masks of 1, 2 and 3 targets and one all-NONE pattern;
# pattern 4 has a target that is also present (a copy row), pattern 1 a
# duplicate target
PRESENT = [[0, 1, 5], [7, 2, 0], [9, 4, 6], [1, 8, 2], [3, 0, 2], [6, 5, 1]]
TARGETS = [[2, NONE, NONE], [1, 1, 9], [0, NONE, 2], [NONE, NONE, NONE], [0, 1, 4], [NONE, 0, 3]]


def cycled_ids(ns, npat):
    """Ids 0, 1, ..., npat-1, 0, ...: adjacent stripes never share a pattern."""
    return [s % npat for s in range(ns)]


def oracle_rows(k, m, blocks, present, targets):
    """blocks: (k, n) the present blocks in slot order; returns {i: (n,) bytes}
    for every target i that is not NONE: decode, then encode the target."""
    n = blocks.shape[1]
    lost = [i for i in range(k) if i not in present]
    extra = [j for j, b in enumerate(present) if b >= k]
    index, slots = list(range(k)), [None] * k
    for j, b in enumerate(present):
        if b < k:
            slots[b] = blocks[j]
    for i, j in zip(lost, extra):  # a parity block stands in every lost primary's slot
        index[i], slots[i] = present[j], blocks[j]
    data = np.stack(slots) if n else np.zeros((k, 0), dtype=np.uint8)
    if lost and n:
        data = data.copy()
        data[lost] = oracle.decode(k, m, np.ascontiguousarray(np.stack(slots)), index)
    out = {}
    for i, t in enumerate(targets):
        if t == NONE:
            continue
        out[i] = data[t] if t < k else (oracle.encode(k, m, data, [t])[0] if n else np.zeros(0, dtype=np.uint8))
    return data, out


class RepairCase(object):
    """present [P][k], targets [P][t] (NONE = -1), ids [ns].  layout "packed"
    (block stride 0 on both sides, stripes in order), "shuffled" (the same,
    stripes placed in the order `place`) or "block" (fixed block strides,
    offsets the prefix sum of the sizes).  skip: stripes the call is to leave
    unwritten (a test spoils their descriptor or id afterwards): their rows
    keep GUARD in `want`."""

    def __init__(self, k, m, sizes, present, targets, ids, layout="packed", place=None, seed=0, skip=()):
        self.k, self.m, self.layout = k, m, layout
        self.sizes = [int(x) for x in sizes]
        self.present = [list(p) for p in present]
        self.targets = [list(t) for t in targets]
        self.ids = [int(x) for x in ids]
        self.ns = ns = len(self.sizes)
        self.t = t = len(self.targets[0])
        total = sum(self.sizes)
        data = np.random.default_rng(seed).integers(0, 256, size=(k, total), dtype=np.uint8)
        allb = np.concatenate([data, oracle.encode(k, m, data)]) if total else np.zeros((m, 0), dtype=np.uint8)
        start = np.cumsum([0] + self.sizes)
        # per pattern, its stripes as one long stripe
        rows = np.zeros((t, total), dtype=np.uint8)
        src_blocks = np.zeros((k, total), dtype=np.uint8)
        for p in range(len(self.present)):
            cols = np.zeros(total, dtype=bool)
            for s in range(ns):
                if self.ids[s] == p:
                    cols[int(start[s]):int(start[s + 1])] = True
            if not cols.any():
                continue
            blk = np.ascontiguousarray(allb[self.present[p]][:, cols])
            src_blocks[:, cols] = blk
            got_data, out = oracle_rows(k, m, blk, self.present[p], self.targets[p])
            assert (got_data == data[:, cols]).all(), "the oracle's decode does not return the data"
            for i, row in out.items():
                rows[i, cols] = row
        if layout == "block":
            self.sbs, self.dbs = total + 7, total + 11
            self.soff = [int(x) for x in start[:-1]]
            self.doff = list(self.soff)
            in_len, out_len = (k - 1) * self.sbs + total, (t - 1) * self.dbs + total
        else:
            self.sbs = self.dbs = 0
            order = list(range(ns)) if layout == "packed" else list(place)
            assert sorted(order) == list(range(ns))
            self.soff, self.doff = [0] * ns, [0] * ns
            a = b = 0
            for s in order:
                self.soff[s], self.doff[s] = a, b
                a += k * self.sizes[s] + gap(s)
                b += t * self.sizes[s] + gap(s)
            in_len, out_len = a, b
        self.src_bytes, self.dst_bytes = in_len, out_len
        self.src = np.full(IN_OFF + in_len + TAIL, BACKGROUND, dtype=np.uint8)
        self.want = np.full(OUT_OFF + out_len + TAIL, GUARD, dtype=np.uint8)
        for s, sz in enumerate(self.sizes):
            a, b = int(start[s]), int(start[s + 1])
            for j in range(k):
                o = IN_OFF + self.soff[s] + j * (self.sbs or sz)
                self.src[o:o + sz] = src_blocks[j, a:b]
            if s in skip:
                continue
            for i, tg in enumerate(self.targets[self.ids[s]]):
                if tg != NONE:
                    o = OUT_OFF + self.doff[s] + i * (self.dbs or sz)
                    self.want[o:o + sz] = rows[i, a:b]
        self.src.setflags(write=False)

    def row_spans(self, s):
        """[begin, end) of every output row of stripe s in the output tensor."""
        sz = self.sizes[s]
        return [(OUT_OFF + self.doff[s] + i * (self.dbs or sz), OUT_OFF + self.doff[s] + i * (self.dbs or sz) + sz)
                for i in range(self.t)]

    def explain(self, got):
        """What differs from `want`: the first wrong (stripe, row) pairs, and
        the wrong bytes outside every row that was to be written."""
        bad = np.flatnonzero(got != self.want)
        if not bad.size:
            return None
        inside = np.zeros(got.shape, dtype=bool)
        wrong = []
        for s in range(self.ns):
            for i, (a, b) in enumerate(self.row_spans(s)):
                if self.targets[self.ids[s]][i] != NONE:
                    inside[a:b] = True
                if (got[a:b] != self.want[a:b]).any():
                    wrong.append((s, i, self.sizes[s], self.ids[s]))
        stray = bad[~inside[bad]]
        return ("wrong (stripe, row, size, id)", wrong[:8], "bytes written outside the rows", stray[:8].tolist())


__all__ = ["RepairCase", "PRESENT", "TARGETS", "NONE", "cycled_ids", "oracle_rows", "rc"]
