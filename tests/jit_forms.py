"""The shape table of the generated bit-sliced kernels' forms, shared by
tests/test_jit_forms_source.py (CPU: the markers of each form in the generated
source) and tests/test_gpu_jit_forms.py (GPU: kernel name and bytes).

zfec_amd/csrc/bitslice.cpp writes one of five structurally different kernels
for an r x k matrix, chosen from (k, r) alone (options_for, bitslice_tiles,
bitslice_split, bitslice_ksplit; rows per tile <= 10, tiles near-equal):

  ONE       k <= 32, r <= 10: one row tile, four units per workgroup of 256
  KSPLIT    k > 32,  r <= 10: a unit's inputs split over 4 waves, partial
            planes reduced through LDS (red[])
  SPLIT     k > 32,  2-8 tiles: a wave per row tile, every wave loads all k
            inputs itself, no LDS
  RESIDENT  k <= 32, 2-8 tiles: a wave per tile, all k inputs' planes in LDS
  DMA       k <= 32, 2-3 tiles and 24 k > 160 tiles: double-buffered LDS-DMA
            phases of 4 inputs

expected_form() restates that choice; the CPU test holds every entry's claimed
form against both it and the generated source, so a shape that moves to another
form when options_for changes fails there instead of silently leaving a form
without GPU coverage."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE, KSPLIT, SPLIT, RESIDENT, DMA = "one", "ksplit", "split", "resident", "dma"
FORMS = (ONE, KSPLIT, SPLIT, RESIDENT, DMA)

MAX_TILE = 10    # bitslice.hpp kBsMaxTile
MAX_COEF = 1600  # bitslice.hpp kJitMaxCoef
ALL_PRIMARIES = 4  # include/zfec_hip.h FEC_FLAG_ALL_PRIMARIES


def place(nums, k):
    """slot order with primary i at slot i (zfec/_fecmodule.c:482-493)."""
    slots = [None] * k
    sec = iter([n for n in nums if n >= k])
    for n in nums:
        if n < k:
            slots[n] = n
    return [s if s is not None else next(sec) for s in slots]


def tiles_of(r):
    return -(-r // MAX_TILE)


def expected_form(k, r):
    """(form, tiles) of the kernel for k inputs and r rows."""
    nt = tiles_of(r)
    assert k * r <= MAX_COEF and 1 <= nt <= 8, (k, r)
    if nt == 1:
        return (KSPLIT if k > 32 else ONE), 1
    if k > 32:
        return SPLIT, nt
    if 24 * k > 160 * nt and nt <= 3:  # (then k >= 14: more inputs than a phase of 4)
        return DMA, nt
    return RESIDENT, nt


class Shape(object):
    """One launch shape.  op "enc": an encode of block numbers `nums` (r of
    them); op "dec": a FEC_FLAG_ALL_PRIMARIES decode from the received block
    numbers `nums` (k of them; r = k, a present primary's row is a unit
    vector).  `unit_cols`: {row: column} of the unit-vector rows, None if the
    matrix is dense; `zero_slices`: whether some wave of the ksplit form sees
    only zero coefficients of some row."""

    def __init__(self, k, m, form, tiles, op="enc", nums=None, unit_cols=None, zero_slices=False):
        self.k, self.m, self.form, self.tiles, self.op = k, m, form, tiles, op
        self.nums = list(nums) if nums is not None else list(range(k, m))
        self.r = k if op == "dec" else len(self.nums)
        self.unit_cols = unit_cols
        self.zero_slices = zero_slices
        assert op in ("enc", "dec") and form in FORMS
        assert op == "enc" or len(self.nums) == k

    @property
    def flags(self):
        return ALL_PRIMARIES if self.op == "dec" else 0

    @property
    def index(self):
        """What the call takes: block numbers (encode) or the slot list (decode)."""
        return self.nums if self.op == "enc" else place(self.nums, self.k)

    @property
    def id(self):
        tag = "" if self.op == "enc" and self.unit_cols is None else ("-allprim" if self.op == "dec" else "-unitrows")
        return "%s-%d_%d%s" % (self.form, self.k, self.m, tag)

    def kernel_prefix(self):
        return "zfec_hip_bitslice_k%d_r%d" % (self.k, self.r)


def _received(k, m, lost):
    """k received block numbers with the primaries `lost` replaced by the last secondaries."""
    return [i for i in range(k) if i not in lost] + list(range(m - len(lost), m))


def _dec(k, m, form, tiles, lost):
    return Shape(k, m, form, tiles, op="dec", nums=_received(k, m, lost),
                 unit_cols={i: i for i in range(k) if i not in lost})


SHAPES = [
    # one tile
    Shape(1, 2, ONE, 1),
    Shape(32, 42, ONE, 1),                       # r = 10: the last one-tile row count
    # ksplit
    Shape(33, 34, KSPLIT, 1),                    # r = 1: only wave 0 stores; input slices of 8, 8, 8, 9
    Shape(33, 43, KSPLIT, 1),                    # r = 10: 80 KiB of red[]
    # primaries 0, 20 and 39 (unit rows) among 7 parity rows: for each of them three of the four
    # waves (slices of 10 inputs) hold only zero coefficients and store all-zero partial planes
    Shape(40, 48, KSPLIT, 1, nums=[0, 20, 39] + list(range(40, 47)), unit_cols={0: 0, 1: 20, 2: 39},
          zero_slices=True),
    # split, not shared
    Shape(33, 44, SPLIT, 2),                     # r = 11: the first row count past ksplit
    Shape(50, 82, SPLIT, 4),                     # k r = 1600 = kJitMaxCoef
    Shape(34, 80, SPLIT, 5),                     # r = 46
    _dec(40, 48, SPLIT, 4, lost=(0, 9, 10, 19, 25, 30, 39)),  # r = 40, k r = 1600, unit rows among dense ones
    # shared, all inputs resident
    Shape(13, 33, RESIDENT, 2),                  # 24 k = 312 <= 160 * 2
    Shape(20, 50, RESIDENT, 3),                  # 24 k = 480 = 160 * 3: exactly at the threshold
    _dec(12, 20, RESIDENT, 2, lost=(1, 4, 5, 11)),
    # shared, double-buffered DMA phases of 4
    Shape(21, 51, DMA, 3),                       # 504 > 480; 5 phases of 4 and a last one of 1
    Shape(32, 62, DMA, 3),                       # 8 full phases
    _dec(22, 30, DMA, 3, lost=(0, 7, 8, 15, 21)),
]

# k r = 1640 > kJitMaxCoef: no generated kernel of the whole matrix
PAST_LIMIT = (41, 81)

# one shape per form for the batched and the grid-stride tests; the ksplit one has the all-zero slices
ONE_PER_FORM = [s for s in SHAPES if s.id in ("one-32_42", "ksplit-40_48-unitrows", "split-33_44", "resident-13_33",
                                              "dma-21_51")]
assert [s.form for s in ONE_PER_FORM] == list(FORMS)

# encodes whose rows apply_matrix_range cuts into groups (at most 48 rows per launch, near-equal),
# each group its own generated kernel: (k, m, row counts of the groups)
ROW_GROUPS = [(2, 256, [42, 42, 43, 42, 42, 43]), (8, 108, [33, 33, 34])]


def row_groups(r, rmax=48):
    """[(first row, rows)] as fec_abi.cpp apply_matrix_range cuts r rows."""
    n = -(-r // rmax)
    return [(g * r // n, (g + 1) * r // n - g * r // n) for g in range(n)]


def generated_sources(tmp_path, k, m, op, nums, flags=0):
    """{file name: text} of the kernels generated for an encode of the block
    numbers `nums` (op "enc") or a decode from the slot list `nums` (op "dec",
    with `flags`), compiled in a fresh process: the JIT registry is per process,
    and another test's code may already hold the kernel in memory (fec_new
    prefetches the kernels the in-tree cache holds), which would compile -- and
    dump -- nothing."""
    dump = tmp_path / "dump"
    dump.mkdir()
    env = dict(os.environ, ZFEC_HIP_JIT_CACHE=str(tmp_path / "cache"), ZFEC_HIP_JIT_DUMP=str(dump))
    call = "jit_prepare_encode(%r)" % (list(nums),) if op == "enc" else "jit_prepare_decode(%r, %d)" % (list(nums), flags)
    prog = ("import sys; sys.path.insert(0, %r)\n"
            "from zfec_amd import capi\n"
            "c = capi.Code(%d, %d)\n"
            "c.%s\n" % (ROOT, k, m, call))
    subprocess.run([sys.executable, "-c", prog], env=env, check=True, timeout=300)
    return {f.name: f.read_text() for f in sorted(dump.glob("zfec_hip_bitslice_k%d_r*.hip" % k))}
