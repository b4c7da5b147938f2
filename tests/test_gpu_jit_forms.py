"""GPU parity of every generated form of the run-time specialised bit-sliced
kernels (zfec_amd/csrc/bitslice.cpp): the one-tile form, ksplit, split without
LDS, LDS-shared with all inputs resident, and LDS-shared in double-buffered DMA
phases -- the shape table of tests/jit_forms.py, whose forms
tests/test_jit_forms_source.py holds against the generated source.  Bit-exact
against the CPU oracle (zfec/fec.c:487-505 encode, :527-557 decode) under
forced JIT, with the launched kernel's name asserted after every launch:

* every table entry at block sizes of one unit, two units overlapping by 2047
  bytes and by 1, and four with a one-byte tail;
* one shape per form batched at an odd row stride from odd bases;
* every coefficient value 1..255 through generated kernels (0: the unit-row
  entries of the table), and calls of more than 48 rows, cut into row groups;
* the grid-stride walk with its carry, reached with ZFEC_HIP_GRID_CAP.

Outputs are pre-filled with 0xA5; the bytes before, between and after the rows
must come back unchanged."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

import jit_forms
from jit_forms import ONE_PER_FORM, SHAPES, Shape
from test_gpu_table_kernels import covering_block

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
TAIL = 64
IN_OFF, OUT_OFF, PAD = 5, 3, 13


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


@pytest.fixture
def force_jit():
    prev = capi.jit_mode(capi.JIT_FORCE)
    yield
    capi.jit_mode(prev)


def flat(blocks):
    """(ns, rows, sz) -> (rows, ns * sz): output byte x depends only on byte x
    of the inputs, so the oracle takes a batch as one long stripe."""
    ns, rows, sz = blocks.shape
    return np.ascontiguousarray(blocks.transpose(1, 0, 2)).reshape(rows, ns * sz)


def unflat(rows2d, ns):
    rows, n = rows2d.shape
    return np.ascontiguousarray(rows2d.reshape(rows, ns, n // ns).transpose(1, 0, 2))


def oracle_case(shape, data):
    """The kernel's inputs (ns, k, sz) for the stripes `data` (ns, k, sz) and
    the rows (ns, r, sz) the oracle expects of the call."""
    k, m, ns = shape.k, shape.m, data.shape[0]
    f = flat(data)
    if shape.op == "enc":
        return data, unflat(oracle.encode(k, m, f, shape.nums), ns)
    # all-primaries decode: the k outputs are the stripe in order -- a present
    # primary's row copies its slot, a lost one's is the oracle's decode
    slots = shape.index
    recv = np.ascontiguousarray(np.concatenate([f, oracle.encode(k, m, f)])[slots])
    want = recv.copy()
    want[[i for i in range(k) if slots[i] >= k]] = oracle.decode(k, m, recv, slots)
    assert (want == f).all()
    return unflat(recv, ns), unflat(want, ns)


class Job(object):
    """One call over device buffers laid out [stripe][block][ld] at odd bases,
    the output pre-filled with GUARD."""

    def __init__(self, shape, blocks, ld=None):
        self.shape = shape
        self.ns, self.k, self.sz = blocks.shape
        self.r = shape.r
        self.ld = ld = ld if ld is not None else self.sz + PAD
        assert ld >= self.sz and self.k == shape.k
        self.code = capi.Code(shape.k, shape.m)
        src = torch.zeros(IN_OFF + self.ns * self.k * ld + TAIL, dtype=torch.uint8, device="cuda")
        src[IN_OFF:IN_OFF + self.ns * self.k * ld].view(self.ns, self.k, ld)[:, :, :self.sz] = \
            torch.from_numpy(np.ascontiguousarray(blocks)).cuda()
        self.src = src
        self.dst = torch.empty(OUT_OFF + self.ns * self.r * ld + TAIL, dtype=torch.uint8, device="cuda")
        self.sp, self.dp = src.data_ptr() + IN_OFF, self.dst.data_ptr() + OUT_OFF

    def launch(self):
        """One stripe through the pointer-array entry point, several through
        the batched one; returns the last kernel's name."""
        self.dst.fill_(GUARD)
        st = torch.cuda.current_stream().cuda_stream
        s, ld = self.shape, self.ld
        flags = capi.FEC_FLAG_ASYNC | s.flags
        if self.ns == 1:
            f = self.code.encode_ptrs if s.op == "enc" else self.code.decode_ptrs
            f([self.sp + j * ld for j in range(self.k)], [self.dp + i * ld for i in range(self.r)], s.index, self.sz,
              stream=st, flags=flags)
        else:
            f = self.code.encode_batch if s.op == "enc" else self.code.decode_batch
            f(self.sp, ld, self.k * ld, self.dp, ld, self.r * ld, s.index, self.sz, self.ns, stream=st, flags=flags)
        return capi.last_kernel_name()

    def result(self, what=""):
        """The output rows (ns, r, sz) and the whole output buffer, once the
        bytes around the rows have been found untouched."""
        torch.cuda.synchronize()
        host = self.dst.cpu().numpy()
        n = self.ns * self.r * self.ld
        assert (host[:OUT_OFF] == GUARD).all(), ("write before the output", what)
        assert (host[OUT_OFF + n:] == GUARD).all(), ("write after the output", what)
        body = host[OUT_OFF:OUT_OFF + n].reshape(self.ns, self.r, self.ld)
        assert (body[:, :, self.sz:] == GUARD).all(), ("write past a row", what)
        return body[:, :, :self.sz], host


def run_one(shape, data, served=True):
    """Launch, check the name, the guards and the bytes; returns the job and
    the whole output buffer."""
    blocks, want = oracle_case(shape, data)
    job = Job(shape, blocks)
    name = job.launch()
    what = (shape.id, job.sz, job.ns, name)
    got, host = job.result(what)
    if served:
        assert name.startswith(shape.kernel_prefix() + "_"), what
    else:
        assert not name.startswith("zfec_hip_bitslice"), what
    assert (got == want).all(), what
    return job, host


SIZES = (2048, 2049, 4095, 6145)


@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
def test_every_form_vs_oracle(force_jit, shape):
    """One stripe per call: one unit; two units overlapping by 2047 bytes; two
    overlapping by 1; four with a one-byte tail."""
    rng = np.random.default_rng(shape.k * 1000 + shape.m)
    for sz in SIZES:
        run_one(shape, rng.integers(0, 256, size=(1, shape.k, sz), dtype=np.uint8))


def test_past_the_limit_is_not_served(force_jit):
    """41/81, k r = 1640 > kJitMaxCoef: no generated kernel takes the matrix.
    The call runs as passes of 32 and 9 inputs; the accumulating second pass is
    never a generated kernel, so the last kernel's name is another one's."""
    k, m = jit_forms.PAST_LIMIT
    shape = Shape(k, m, jit_forms.SPLIT, 4)  # (the form it would have)
    rng = np.random.default_rng(4181)
    for sz in SIZES:
        run_one(shape, rng.integers(0, 256, size=(1, k, sz), dtype=np.uint8), served=False)


BATCHED = ONE_PER_FORM + [s for s in SHAPES if s.id in ("split-40_48-allprim", "resident-12_20-allprim",
                                                        "dma-22_30-allprim")]


@pytest.mark.parametrize("shape", BATCHED, ids=[s.id for s in BATCHED])
def test_every_form_batched_guarded(force_jit, shape):
    """3 stripes of 2049 bytes, rows sz + 13 apart, inputs from base + 5,
    outputs at base + 3: a store past sz, or before a row, lands on a guard
    byte instead of in allocator slack."""
    rng = np.random.default_rng(shape.k * 1000 + shape.m + 3)
    run_one(shape, rng.integers(0, 256, size=(3, shape.k, 2049), dtype=np.uint8))


def covering_stripe(rng, k, sz):
    """covering_block in both 1 KiB halves of the first unit: a lane owns 16
    bytes of each, 32 bytes to a bit-plane transpose."""
    assert sz >= 2048
    data = covering_block(rng, k, sz)
    data[:, 1024:2048] = np.roll(data[:, :1024], 5, axis=1)
    return data[None]


def test_every_coefficient_through_generated_kernels(force_jit):
    """Every coefficient value 1..255 through the four-Russians emitter (the
    combinations of planes 0-3 and 4-7 and the first-assignment / ^= / x3
    branches are chosen per coefficient).  The 254 parity rows of the 2/256
    code hold every value 2..255 in each column; one call runs them as six row
    groups of 42 / 43 rows (shared, resident, 5 tiles).  Value 1 comes from the
    1/10 code's rows (one tile).  Coefficient 0: the unit-row entries of the
    table.  The 8/108 encode (100 rows) runs as groups of 33 / 33 / 34.

    fec_last_kernel_name names the last launch of a call only, so after the one
    call every row group is also launched on its own: the same matrix, hence the
    same registry entry and kernel name as the group's launch inside the call."""
    rng = np.random.default_rng(255)
    covered = set()
    for (k, m, sz) in ((2, 256, 2049), (1, 10, 2049), (8, 108, 4097)):
        enc = oracle.enc_matrix(k, m)
        data = covering_stripe(rng, k, sz)
        whole = Shape(k, m, jit_forms.RESIDENT if k > 1 else jit_forms.ONE, 1)
        groups = jit_forms.row_groups(m - k)
        if k > 1:
            assert [n for _, n in groups] == dict((a, c) for a, _, c in jit_forms.ROW_GROUPS)[k]
        blocks, want = oracle_case(whole, data)
        job = Job(whole, blocks)
        name = job.launch()
        got, _ = job.result((k, m, name))
        assert name.startswith("zfec_hip_bitslice_k%d_r%d_" % (k, groups[-1][1])), name
        assert (got == want).all(), (k, m)
        names = set()
        for i0, rg in groups:
            nums = list(range(k + i0, k + i0 + rg))
            run_one(Shape(k, m, jit_forms.expected_form(k, rg)[0], jit_forms.tiles_of(rg), nums=nums), data)
            names.add(capi.last_kernel_name())
            covered |= set(int(v) for v in enc[nums].ravel())
        assert len(names) == len(groups) and name in names, (names, name)
    enc2 = oracle.enc_matrix(2, 256)[2:]
    assert all(set(int(v) for v in enc2[:, j]) == set(range(2, 256)) for j in range(2))
    assert covered >= set(range(1, 256)), sorted(set(range(1, 256)) - covered)


# (sz, stripes) with the grid capped at 3 workgroups.  Forms of one unit per workgroup: 2049 x 7 is
# 2 units per stripe (cps) and 3 per step, gs_c = 1, gs_s = 1: the carry fires on alternate trips;
# 20000 x 2 is cps = 10, gs_c = 3, gs_s = 0: the stripe index advances by the carry alone.  The
# one-tile form (4 units per workgroup, 12 per step): 9000 x 9 is cps = 5, gs_c = 2, gs_s = 2, 45
# units in 4 trips, the last one partly past the end.  Every form runs all three.
WALK_SHAPES = [(2049, 7), (20000, 2), (9000, 9)]


@pytest.mark.parametrize("shape", ONE_PER_FORM, ids=[s.id for s in ONE_PER_FORM])
def test_grid_stride_walk(knobs, force_jit, shape):
    """ZFEC_HIP_GRID_CAP=3: every launch is 3 workgroups, so each walks several
    units grid-stride: c += gs_c; s += gs_s; if (c >= cps) { c -= cps; ++s; }.
    Every stripe is checked against the oracle, guard bytes included; the same
    calls on the same buffers without the hook must give the same bytes."""
    rng = np.random.default_rng(shape.k * 1000 + shape.m + 768)
    knobs(ZFEC_HIP_GRID_CAP=3)
    capped = [run_one(shape, rng.integers(0, 256, size=(ns, shape.k, sz), dtype=np.uint8)) for sz, ns in WALK_SHAPES]
    knobs(ZFEC_HIP_GRID_CAP=0)
    for job, host in capped:
        name = job.launch()
        _, plain = job.result((shape.id, job.sz, job.ns, "uncapped"))
        assert name.startswith(shape.kernel_prefix() + "_"), name
        assert (plain == host).all(), (shape.id, job.sz, job.ns)
