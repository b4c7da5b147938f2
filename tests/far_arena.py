"""Shared by test_far_layout.py (CPU) and test_gpu_far_offsets.py: batched calls
whose stripes lie GiBs apart inside one large allocation that is touched only
where blocks lie, so that every kernel family forms addresses past 2^31 and
2^32 bytes from its base pointer with a few MiB of data.

The arena is LEAD + SPAN + TAIL bytes and the base handed to the library is
arena + LEAD + odd (5 for sources, 3 for outputs, as guarded_batch.py).  A block
that truly starts o bytes past the base would, after a truncation of its offset
somewhere, be addressed at one of aliases(o): o mod 2^32, o mod 2^31, or the
sign extension of the low 32 bits.  LEAD >= 2^31 and every o < SPAN, so all of
them lie inside the arena: a wrong kernel reads background bytes (or another
row) and writes guard bytes, and fails a comparison instead of faulting.

Geometries, each (block_stride, stripe_stride) for given rows, sz and ns:

  far_stripes  rows (sz + 12) | 1 apart inside a stripe, stripes an odd number
               just under 64 MiB apart: row 0 of stripe 32 straddles byte 2^31,
               row 0 of stripe 64 byte 2^32, stripes 33.. begin past 2^31 and
               65..69 past 2^32
  far_pair     3 stripes an odd number just under 2^31 apart, the same
               straddles in row 0 of stripes 1 and 2: kernels that need no batch
  far_blocks   block-major without the collapse: stripes sz + 8 apart (sz would
               make batch_geometry fold the batch into one long stripe), blocks
               an odd number of about SPAN / rows apart, chosen so that one row
               of some slot j straddles 2^31 and one of slot 2 j straddles 2^32.
               1, 2, 4, 6 and 8 rows leave no room for both inside SPAN
               (far_blocks_both): their last slot straddles 2^32 only, and a
               single row has no block stride to test

The checker's rules are plain functions of numpy arrays and counts (judge,
judge_source), so test_far_layout.py can feed them synthetic results; Arena
applies them on the device, where nothing but the gathered rows ever leaves it.

Data is fixed: numpy default_rng(SEED + a per-case number), and BACKGROUND is
held against every case's inputs by test_far_layout.py."""
import bisect

import numpy as np

GUARD = 0xA5        # fill of the destination arena
BACKGROUND = 0x3C   # fill of the source arena
SEED = 2031         # of every case's data
SRC_ODD, DST_ODD = 5, 3
LEAD = 2**31 + 2**20
SPAN = 2**32 + 2**29
TAIL = 4096
NS = 70
CHUNK = 1 << 26     # bytes per counting / summing slice (the 64-bit sum widens each to 8 x that)


def aliases(o):
    """Where a truncated offset would address byte o (measured from the base)."""
    lo = o % 2**32
    return (lo, o % 2**31, lo - 2**32 if lo >= 2**31 else lo)


def far_stripes(rows, sz, ns=NS):
    d = (sz // 128) | 1
    assert 64 * d < sz, "byte 2^32 must fall inside row 0 of stripe 64"
    bs = (sz + 12) | 1
    ss = 2**26 - d
    assert rows * bs <= ss and ns > 65
    return bs, ss


def far_pair(rows, sz, ns=3):
    d = (sz // 4) | 1
    assert 2 * d < sz and ns == 3
    bs = (sz + 12) | 1
    ss = 2**31 - d
    assert rows * bs <= ss
    return bs, ss


def far_blocks(rows, sz, ns=NS):
    ss = sz + 8
    room = SPAN - ((ns - 1) * ss + sz)
    # slot j of stripe s straddles 2^31 at byte x (t = s * ss + x), slot 2 j of
    # stripe 2 s straddles 2^32 at byte 2 x: the largest odd stride that fits
    for j in range(1, (rows - 1) // 2 + 1):
        if (rows - 1) * ((2**31 - (ns // 2) * ss) // j) > room:
            continue
        for s in range((ns - 1) // 2):
            for x in range(1, (sz + 1) // 2):
                num = 2**31 - (s * ss + x)
                if num % j == 0 and (num // j) % 2 == 1 and (rows - 1) * (num // j) <= room:
                    return num // j, ss
    # no such stride (far_blocks_both): the last slot straddles 2^32 in a middle stripe
    j = max(1, rows - 1)
    for s in range(ns // 2, ns - 1):
        for x in range(1, sz):
            num = 2**32 - (s * ss + x)
            if num % j == 0 and (num // j) % 2 == 1:
                return num // j, ss
    raise AssertionError(("no far_blocks stride", rows, sz, ns))


def far_blocks_both(rows, sz, ns=NS):
    """Whether `rows` block arrays can straddle both 2^31 and 2^32 inside SPAN.
    The straddling rows lie in slots j and j' with j bs ~ 2^31 and j' bs ~ 2^32
    to within the ns * (sz + 8) bytes of a slot, so j' = 2 j <= rows - 1, and
    the last slot must fit: (rows - 1) * 2^31 / j <= SPAN, that is
    j >= (rows - 1) / 2.25.  Rows 3, 5, 7 and every count from 9 have such a
    j; 1, 2, 4, 6 and 8 have none."""
    room = SPAN - ((ns - 1) * (sz + 8) + sz)
    return any((rows - 1) * ((2**31 - (ns // 2) * (sz + 8)) // j) <= room for j in range(1, (rows - 1) // 2 + 1))


GEOMETRIES = {"far_stripes": far_stripes, "far_pair": far_pair, "far_blocks": far_blocks}


class Layout(object):
    """`rows` rows of sz bytes in each of ns stripes under one geometry; `first`
    is the byte offset of row 0 of stripe 0 from the base (sub-layouts)."""

    def __init__(self, kind, rows, sz, ns=None, first=0, strides=None):
        self.kind, self.rows, self.sz, self.first = kind, rows, sz, first
        self.ns = ns if ns is not None else (3 if kind == "far_pair" else NS)
        self.bs, self.ss = strides if strides is not None else GEOMETRIES[kind](rows, sz, self.ns)

    def sub(self, j0, rows):
        """Rows j0 .. j0 + rows of every stripe: the layout of one of two jobs."""
        assert j0 + rows <= self.rows
        return Layout(self.kind, rows, self.sz, self.ns, self.first + j0 * self.bs, (self.bs, self.ss))

    def start(self, s, j):
        return self.first + s * self.ss + j * self.bs

    def starts(self):
        return [(s, j, self.start(s, j)) for s in range(self.ns) for j in range(self.rows)]

    @property
    def extent(self):
        """What the call passes: (ns-1)*sss + (rows-1)*sbs + sz."""
        return (self.ns - 1) * self.ss + (self.rows - 1) * self.bs + self.sz

    def straddlers(self, edge):
        return [(s, j) for s, j, o in self.starts() if o < edge < o + self.sz]

    def beginners(self, lo, hi=None):
        """(stripe, row) of the rows that begin at or past byte lo (and before hi)."""
        return [(s, j) for s, j, o in self.starts() if o >= lo and (hi is None or o < hi)]

    def far_rows(self):
        """One row beginning in [2^31, 2^32) and one beginning past 2^32 (the
        last such row of each range), where the layout has them."""
        a, b = self.beginners(2**31, 2**32), self.beginners(2**32)
        return (a[-1] if a else None), (b[-1] if b else None)

    def __repr__(self):
        return "%s(rows=%d, sz=%d, ns=%d, first=%d)" % (self.kind, self.rows, self.sz, self.ns, self.first)


def data(case_no, ns, rows, sz):
    """The fixed random blocks (ns, rows, sz) of case number `case_no`."""
    return np.random.default_rng(SEED + case_no).integers(0, 256, size=(ns, rows, sz), dtype=np.uint8)


# ---- the checker's rules ---------------------------------------------------------------------

def judge(got, want, not_fill, fill, what=""):
    """The rows gathered from the true locations equal the oracle's, and the
    whole arena holds exactly as many bytes other than `fill` as those rows do:
    a row written at an alias as well, or anywhere else, moves the count."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        bad = sorted(set(map(tuple, np.argwhere((got != want).any(axis=2)).tolist())))
        untouched = [b for b in bad if (got[b][got[b] != want[b]] == fill).all()]
        raise AssertionError((what, "wrong (stripe, row)", bad[:8], "of them only untouched bytes", untouched[:8]))
    expect = int(np.count_nonzero(want != fill))
    assert not_fill == expect, (what, "bytes other than the fill in the whole arena", not_fill, "in the rows", expect)


def judge_source(sum_before, sum_after, what=""):
    assert sum_before == sum_after, (what, "the source arena was written", sum_before, sum_after)


class Sparse(object):
    """A byte-addressed model of an arena for the CPU tests: `fill` everywhere
    but where rows were written; offsets are measured from the base and may be
    negative (the lead).  Later writes win."""

    def __init__(self, fill):
        self.fill = fill
        self.keys, self.writes, self.longest = [], [], 0

    def write(self, o, row):
        row = np.asarray(row, dtype=np.uint8)
        bisect.insort(self.keys, (o, len(self.writes)))
        self.writes.append((o, row))
        self.longest = max(self.longest, len(row))

    def place(self, lay, blocks):
        assert blocks.shape == (lay.ns, lay.rows, lay.sz), (blocks.shape, lay)
        for s, j, o in lay.starts():
            self.write(o, blocks[s, j])

    def read(self, o, n):
        out = np.full(n, self.fill, dtype=np.uint8)
        lo = bisect.bisect_left(self.keys, (o - self.longest + 1, -1))
        hi = bisect.bisect_left(self.keys, (o + n, -1))
        for _, i in sorted(self.keys[lo:hi], key=lambda key: key[1]):
            w, row = self.writes[i]
            a, b = max(o, w), min(o + n, w + len(row))
            if a < b:
                out[a - o:b - o] = row[a - w:b - w]
        return out

    def gather(self, lay):
        return np.stack([np.stack([self.read(lay.start(s, j), lay.sz) for j in range(lay.rows)])
                         for s in range(lay.ns)])

    def count_not(self, v):
        """Bytes other than the fill v, over the union of everything written."""
        assert v == self.fill
        n, end = 0, None
        for o, i in self.keys:
            ln = len(self.writes[i][1])
            a = o if end is None else max(o, end)
            if a < o + ln:
                n += int(np.count_nonzero(self.read(a, o + ln - a) != v))
                end = o + ln
        return n


# ---- the arena on the device -----------------------------------------------------------------

class Arena(object):
    """One torch.uint8 device tensor of LEAD + SPAN + TAIL bytes holding `fill`.
    Rows are placed, gathered and cleared through strided views of it; the
    counts and sums read it in slices of CHUNK bytes and stay on the device."""

    def __init__(self, torch, fill, odd):
        self.torch, self.fill, self.odd = torch, fill, odd
        self.t = torch.full((LEAD + SPAN + TAIL,), fill, dtype=torch.uint8, device="cuda")

    @property
    def base(self):
        """The pointer handed to the library."""
        return self.t.data_ptr() + LEAD + self.odd

    def view(self, lay):
        assert lay.first >= 0 and lay.first + lay.extent <= SPAN, lay
        return self.t.as_strided((lay.ns, lay.rows, lay.sz), (lay.ss, lay.bs, 1), LEAD + self.odd + lay.first)

    def row(self, lay, s, j):
        """Row j of stripe s by plain slicing."""
        o = LEAD + self.odd + lay.start(s, j)
        return self.t[o:o + lay.sz]

    def place(self, lay, blocks):
        assert blocks.shape == (lay.ns, lay.rows, lay.sz), (blocks.shape, lay)
        self.view(lay).copy_(self.torch.from_numpy(np.ascontiguousarray(blocks)).cuda())

    def gather(self, lay):
        return self.view(lay).contiguous().cpu().numpy()

    def clear(self, lay):
        self.view(lay).fill_(self.fill)

    def reset(self):
        self.t.fill_(self.fill)

    def count_not(self, v, lo=0, hi=None):
        """Bytes other than v in arena bytes [lo, hi) (the whole arena by default)."""
        hi = self.t.numel() if hi is None else hi
        n = self.torch.zeros((), dtype=self.torch.int64, device="cuda")
        for a in range(lo, hi, CHUNK):
            n += (self.t[a:min(hi, a + CHUNK)] != v).sum()
        return int(n.item())

    def total(self):
        """The 64-bit sum of every byte."""
        n = self.torch.zeros((), dtype=self.torch.int64, device="cuda")
        for a in range(0, self.t.numel(), CHUNK):
            n += self.t[a:a + CHUNK].sum(dtype=self.torch.int64)
        return int(n.item())

    def check(self, lay, want, what=""):
        """judge() the rows of `lay` against `want`, then clear them; a failed
        check refills the whole arena so that later tests start clean."""
        self.torch.cuda.synchronize()
        try:
            got = self.gather(lay)
            # the strided view against plain slices, at the rows that matter most
            for s, j in lay.straddlers(2**31) + lay.straddlers(2**32) + [r for r in lay.far_rows() if r]:
                assert (self.row(lay, s, j).cpu().numpy() == got[s, j]).all(), (what, "view and slice differ", s, j)
            judge(got, want, self.count_not(self.fill), self.fill, what)
        except AssertionError:
            self.reset()
            raise
        self.clear(lay)
