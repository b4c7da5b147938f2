"""Shared by test_ragged_surface.py (CPU) and test_gpu_ragged.py: one ragged
call (fec_encode_batch_ragged / fec_decode_batch_ragged) laid out on the host,
and the whole output arena the CPU oracle expects of it.

The arenas follow guarded_batch.py: the base handed to the library is 5 bytes
into the source tensor and 3 into the output tensor, the output is pre-filled
with 0xA5, and `want` is the WHOLE output arena -- 0xA5 everywhere but in the
rows -- so one comparison checks the rows and every byte before, between and
after them.  Packed rows have no gap between them; stripes are placed with a
gap of 13 + (s % 3) bytes.

The arithmetic is bytewise, so the oracle takes a ragged batch as one long
stripe: block j of every stripe concatenated."""
import numpy as np

from oracle import oracle

GUARD = 0xA5
BACKGROUND = 0x3C
IN_OFF, OUT_OFF, TAIL = 5, 3, 64

# test_edge_sizes_k3: the byte tail, the overlapped last chunk, the wave
# boundary at 1 KiB on both sides, zero-size stripes first, last and adjacent,
# and one stripe of 69 units
EDGE_SIZES = [0, 1, 15, 16, 17, 31, 33, 1008, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4095, 4096, 4097, 0, 0, 5000,
              70001, 3, 0]
# ranges of 27 units that begin on a stripe boundary right after zero-size
# stripes (units 27 and 54) and mid-stripe (unit 81)
BOUNDARY_SIZES = [1024] * 27 + [0, 0] + [1024] * 27 + [0] + [2048] * 27


def units(sizes):
    """numpy's fec_ragged_units: the exclusive prefix sum of ceil(size / 1024)."""
    u = (np.asarray(sizes, dtype=np.uint64) + np.uint64(1023)) // np.uint64(1024)
    return [0] + [int(x) for x in np.cumsum(u, dtype=np.uint64)]


def wave_ranges(total, waves):
    """[first, end) of every wave: the shard_range rule."""
    q, e = divmod(total, waves)
    return [(g * q + min(g, e), g * q + min(g, e) + q + (1 if g < e else 0)) for g in range(waves)]


def stripe_of(ustart, unit):
    """The stripe that holds `unit`: the last s with ustart[s] <= unit."""
    return max(s for s in range(len(ustart) - 1) if ustart[s] <= unit)


def gap(s):
    return 13 + (s % 3)


class Case(object):
    """op "enc" (nums: the blocks to produce) or "dec" (nums: the block in
    every slot; all_primaries: FEC_FLAG_ALL_PRIMARIES).  layout "packed"
    (block stride 0 on both sides, stripes in order), "shuffled" (the same,
    the stripes placed in the arena in the order `place`) or "block" (fixed
    block strides, offsets the prefix sum of the sizes)."""

    def __init__(self, k, m, op, sizes, nums=None, all_primaries=False, layout="packed", place=None, seed=0):
        self.k, self.m, self.op, self.layout = k, m, op, layout
        self.sizes = [int(x) for x in sizes]
        ns, total = len(self.sizes), sum(self.sizes)
        self.ns = ns
        data = np.random.default_rng(seed).integers(0, 256, size=(k, total), dtype=np.uint8)
        if op == "enc":
            self.nums = list(range(k, m)) if nums is None else list(nums)
            blocks, rows = data, oracle.encode(k, m, data, self.nums)
        else:
            self.nums = list(nums)
            blocks = np.ascontiguousarray(np.concatenate([data, oracle.encode(k, m, data)])[self.nums])
            lost = [i for i in range(k) if self.nums[i] >= k]
            rows = oracle.decode(k, m, blocks, self.nums)
            assert (rows == data[lost]).all()
            if all_primaries:
                rows = data
        self.all_primaries = all_primaries
        self.r = r = rows.shape[0]
        start = np.cumsum([0] + self.sizes)
        if layout == "block":
            self.sbs, self.dbs = total + 7, total + 11
            self.soff = [int(x) for x in start[:-1]]
            self.doff = list(self.soff)
            in_len, out_len = (k - 1) * self.sbs + total, (r - 1) * self.dbs + total if r else 0
        else:
            self.sbs = self.dbs = 0
            order = list(range(ns)) if layout == "packed" else list(place)
            assert sorted(order) == list(range(ns))
            self.soff, self.doff = [0] * ns, [0] * ns
            a = b = 0
            for s in order:
                self.soff[s], self.doff[s] = a, b
                a += k * self.sizes[s] + gap(s)
                b += r * self.sizes[s] + gap(s)
            in_len, out_len = a, b
        self.src_bytes, self.dst_bytes = in_len, out_len
        self.src = np.full(IN_OFF + in_len + TAIL, BACKGROUND, dtype=np.uint8)
        self.want = np.full(OUT_OFF + out_len + TAIL, GUARD, dtype=np.uint8)
        for s, sz in enumerate(self.sizes):
            a, b = int(start[s]), int(start[s + 1])
            for j in range(k):
                o = IN_OFF + self.soff[s] + j * (self.sbs or sz)
                self.src[o:o + sz] = blocks[j, a:b]
            for i in range(r):
                o = OUT_OFF + self.doff[s] + i * (self.dbs or sz)
                self.want[o:o + sz] = rows[i, a:b]

    def row_spans(self, s):
        """[begin, end) of every output row of stripe s in the output tensor."""
        sz = self.sizes[s]
        return [(OUT_OFF + self.doff[s] + i * (self.dbs or sz), OUT_OFF + self.doff[s] + i * (self.dbs or sz) + sz)
                for i in range(self.r)]

    def explain(self, got):
        """What differs from `want`: the first wrong stripes, and the wrong
        bytes outside every row."""
        bad = np.flatnonzero(got != self.want)
        if not bad.size:
            return None
        inside = np.zeros(got.shape, dtype=bool)
        wrong = []
        for s in range(self.ns):
            for a, b in self.row_spans(s):
                inside[a:b] = True
                if (got[a:b] != self.want[a:b]).any() and s not in wrong:
                    wrong.append(s)
        stray = bad[~inside[bad]]
        return ("wrong stripes", wrong[:8], "their sizes", [self.sizes[s] for s in wrong[:8]],
                "bytes written outside the rows", stray[:8].tolist())
