"""Every kernel family addressed past 2 GiB and 4 GiB from its base pointer.

Each case is one batched call whose stripes (far_stripes, far_pair) or block
arrays (far_blocks) lie GiBs apart inside the two arenas of tests/far_arena.py:
a source filled with one background byte and a destination filled with 0xA5,
both touched only where rows lie.  The sizes are the smallest at which a kernel
still has a full unit, an overlapped last unit and a tail: 4097 bytes for the
16-byte-unit and the 2-KiB-unit kernels, 1366 for matapply_rows, 9000 for
matapply_bsg.  Data is fixed-seed random; the expected bytes come from the CPU
oracle or the numpy models of the scrub calls, never from the library; every
case asserts the launched kernel's name.

After a call the output rows are gathered from their true places and compared,
the bytes of the whole destination arena that differ from 0xA5 are counted and
must be exactly those of the expected rows (a write anywhere in 6.5 GiB moves
the count), and the source arena's 64-bit sum must be what it was.  The lead
before the base and the span after it hold every address a 32-bit truncation
or sign extension of an offset could form, so a wrong kernel fails these
comparisons instead of faulting; tests/test_far_layout.py holds that design,
for every layout and every input of this module, on the CPU.

The cases are listed by all_cases() for that test.  Two arenas of 6.5 GiB and
slices of 256 MiB: the module holds under 14 GiB of device memory."""
import zlib

import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

import far_arena
import jit_forms
import test_gpu_mixed as mixed
import test_gpu_repair as repair
import test_gpu_verify as verify
from correct_ref import corrected
from far_arena import BACKGROUND, GUARD, Layout, judge, judge_source
from guarded_batch import decode_case, encode_case
from locate_ref import CLEAN, oracle_PQ, verdicts
from test_gpu_bsg import bsg_name, bsg_only, cus, units_of  # noqa: F401  (fixtures)
from test_gpu_bsr import bsr_exact, bsr_only, tbl_name  # noqa: F401
from test_gpu_jit_forms import force_jit, oracle_case  # noqa: F401
from test_gpu_table_kernels import jit_off, lds_name, lds_only  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5A5A5A5
GW = 4  # guard words before and after the mask / verdict words
FUSED_OFF = 4294967295
SZ, SZ_ROWS, SZ_BSG = 4097, 1366, 9000
BIG = 2**32 + 4097


def case_no(name):
    return zlib.crc32(name.encode()) % 100000


# ---- the cases: plain data and numpy, so that the CPU test can read them ------------------------

class Apply(object):
    """One encode or decode call from the source arena into the destination
    arena.  `sel`: the block numbers of an encode (default: every parity block)
    or the slot list of a decode; `shape`: a jit_forms.Shape instead."""

    def __init__(self, fam, k, m, op, geom, name, sz=SZ, sel=None, shape=None):
        self.fam, self.k, self.m, self.op, self.geom, self.name, self.sz = fam, k, m, op, geom, name, sz
        self.sel, self.shape = sel, shape
        if shape is not None:
            self.r = shape.r
        elif op == "enc":
            self.r = m - k if sel is None else len(sel)
        else:
            self.r = sum(1 for b in sel if b >= k)
        self.id = "%s-%d_%d-%s-%s" % (fam, k, m, op, geom)
        self.lin, self.lout = Layout(geom, k, sz), Layout(geom, self.r, sz)
        self.ns = self.lin.ns

    def data(self):
        return far_arena.data(case_no(self.id), self.ns, self.k, self.sz)

    def build(self):
        """(inputs (ns, k, sz), expected rows (ns, r, sz), index, flags)."""
        if self.shape is not None:
            blocks, want = oracle_case(self.shape, self.data())
            return blocks, want, self.shape.index, self.shape.flags
        if self.op == "enc":
            blocks, want, index = encode_case(self.k, self.m, self.data(), self.sel)
        else:
            blocks, want, index = decode_case(self.k, self.m, self.data(), self.sel)
        return blocks, want, index, 0

    def inputs(self):
        return self.data() if self.op == "enc" else self.build()[0]

    def placed(self):
        return [(self.lin, self.inputs())]

    def outs(self):
        return [self.lout]


def both(fam, k, m, op, name, geoms=("far_stripes", "far_blocks"), **kw):
    return [Apply(fam, k, m, op, g, name, **kw) for g in geoms]


REG = (both("reg", 3, 10, "enc", "matapply_reg<3,7>") + both("reg", 3, 10, "dec", "matapply_reg<3,3>", sel=[7, 8, 9]) +
       both("reg", 4, 12, "enc", "matapply_reg<4,8>"))
ROWS = [Apply("rows", 3, 10, "enc", "far_stripes", "matapply_rows<3,7>", sz=SZ_ROWS)]
LDS = both("lds", 10, 16, "enc", lds_name(10, 6))
SMALL = [Apply("small", 20, 60, "enc", "far_pair", "matapply_small")]
# the arguments form and the table form (more than one row group)
BSG = [Apply("bsg", k, m, "enc", "far_stripes",
             lambda k=k, m=m: bsg_name(k, m - k, units_of(SZ_BSG, far_arena.NS), cus()), sz=SZ_BSG)
       for k, m in ((10, 16), (20, 60))]
UNITS = far_arena.NS * -(-SZ // 2048)
# one wave; LDS phases with the addresses in the arguments; in the table; shared combinations
BSR = (both("bsr", 10, 16, "enc", bsr_exact(10, 6, UNITS)) +
       [Apply("bsr", 9, 20, "enc", "far_stripes", bsr_exact(9, 11, UNITS)),
        Apply("bsr", 20, 60, "enc", "far_stripes", bsr_exact(20, 40, UNITS)),
        Apply("bsr", 128, 256, "enc", "far_stripes", tbl_name(128, UNITS, 128))])
assert [c.name for c in BSR] == ["matapply_bsr<6>", "matapply_bsr<6>", "matapply_bsr<6,lds>",
                                 "matapply_bsr<10,lds,tbl>", "matapply_bsr<8,lds,tbl,cmb>"]
# inputs split over the waves: one row group, and row groups of 8 past ten rows
KS = [Apply("ks", 94, 100, "enc", "far_pair", "matapply_bsr<6,ks,tbl>"),
      Apply("ks", 64, 109, "enc", "far_pair", tbl_name(45, 3 * -(-SZ // 2048), 64))]
assert KS[1].name == "matapply_bsr<8,ks,tbl>"
JIT = [Apply("jit-" + s.form, s.k, s.m, s.op, "far_stripes", s.kernel_prefix() + "_", shape=s)
       for s in jit_forms.ONE_PER_FORM]


class Pair(object):
    """An encode and a decode of the 3/10 code as the two jobs of one
    fec_run_batch_jobs call: rows 0-2 and 3-5 of every source stripe, rows 0-6
    and 7-9 of every destination stripe."""
    id, name, geom, sz = "pair-3_10-far_stripes", "matapply_pair<3,7,3>", "far_stripes", SZ

    def __init__(self):
        self.lin, self.lout = Layout(self.geom, 6, self.sz), Layout(self.geom, 10, self.sz)
        self.ns = self.lin.ns

    def build(self):
        a = encode_case(3, 10, far_arena.data(case_no(self.id), self.ns, 3, self.sz))
        b = decode_case(3, 10, far_arena.data(case_no(self.id) + 1, self.ns, 3, self.sz), [7, 8, 9])
        return a, b

    def placed(self):
        a, b = self.build()
        return [(self.lin.sub(0, 3), a[0]), (self.lin.sub(3, 3), b[0])]

    def outs(self):
        return [self.lout]


class Mixed(object):
    """fec_decode_batch_mixed, a pattern per stripe: matapply_mixed<K>."""

    def __init__(self, K, geom):
        self.k, self.m, self.geom, self.sz = K, K + 4, geom, SZ
        self.id, self.name = "mixed-%d-%s" % (K, geom), "matapply_mixed<%d>" % K
        self.lin = self.lout = Layout(geom, K, SZ)
        self.ns = self.lin.ns

    def build(self):
        """(received blocks, expected rows, patterns, ids)."""
        data, allb = mixed.stripes(self.k, self.m, self.ns, self.sz, seed=far_arena.SEED)
        pats = mixed.random_patterns(np.random.default_rng(far_arena.SEED + self.k), self.k, self.m, self.ns)
        ids = np.arange(self.ns, dtype=np.uint32)
        return mixed.received(allb, pats, ids, self.sz), np.asarray(data), pats, ids

    def placed(self):
        return [(self.lin, self.build()[0])]

    def outs(self):
        return [self.lout]


class Repair(object):
    """fec_repair_batch, a pattern per stripe, some rows FEC_REPAIR_NONE: matrepair_mixed<K,R>."""

    def __init__(self, K, m, t, geom):
        self.k, self.m, self.t, self.geom, self.sz = K, m, t, geom, SZ
        self.id, self.name = "repair-%d_%d-%s" % (K, t, geom), "matrepair_mixed<%d,%d>" % (K, t)
        self.lin, self.lout = Layout(geom, K, SZ), Layout(geom, t, SZ)
        self.ns = self.lin.ns

    def build(self):
        """(received blocks, expected rows, present, targets, ids)."""
        _, allb = mixed.stripes(self.k, self.m, self.ns, self.sz, seed=far_arena.SEED)
        rng = np.random.default_rng(far_arena.SEED + self.t)
        pres, tgts = repair.sweep_patterns(rng, self.k, self.m, self.t, self.ns)
        assert any(repair.NONE in tg for tg in tgts)
        ids = np.arange(self.ns, dtype=np.uint32)
        return mixed.received(allb, pres, ids, self.sz), repair.expected(allb, tgts, ids, self.sz), pres, tgts, ids

    def placed(self):
        return [(self.lin, self.build()[0])]

    def outs(self):
        return [self.lout]


class Scrub(object):
    """The first nb blocks of every stripe of the k/m code, the first k the
    basis, under one geometry: the inputs of a verify, locate or correct call.
    `knob`: the value of ZFEC_HIP_VERIFY_FUSED_MIN, or None; `scratch`: a
    ZFEC_HIP_VERIFY_SCRATCH cap, under which the two-step paths cut the batch
    into runs of stripes (64 KiB: runs of 2 for the 6 check rows of 10/16)."""

    def set_knobs(self, knobs):
        if self.knob is not None:
            knobs(ZFEC_HIP_VERIFY_FUSED_MIN=self.knob)
        if self.scratch is not None:
            knobs(ZFEC_HIP_VERIFY_SCRATCH=self.scratch)

    def __init__(self, fam, k, m, nb, geom, name, knob=None, scratch=None):
        self.fam, self.k, self.m, self.nb, self.geom, self.name, self.sz = fam, k, m, nb, geom, name, SZ
        self.knob, self.scratch = knob, scratch
        self.c = nb - k
        self.id = "%s-%d_%d_%d-%s-%s%s" % (fam, k, m, nb, name, geom, "-cut" if scratch else "")
        self.nums = list(range(nb))
        self.lay = Layout(geom, nb, SZ)
        self.ns = self.lay.ns

    def clean(self):
        return np.ascontiguousarray(verify.stripes(self.k, self.m, self.ns, self.sz)[:, self.nums, :])

    def far_errors(self):
        """(stripe, slot) of a row that begins in [2^31, 2^32) and of one that
        begins past 2^32 (a basis row there, where the layout has one), in
        different stripes; and the stripe of a double error in the last two
        slots of the last stripe, which lie past 2^32 in both geometries."""
        a, b = self.lay.beginners(2**31, 2**32), self.lay.beginners(2**32)
        ea = a[len(a) // 2]
        b = [r for r in b if r[0] not in (ea[0], self.ns - 1)]
        basis = [r for r in b if r[1] < self.k]
        eb = basis[len(basis) // 2] if basis else b[len(b) // 2]
        assert len({ea[0], eb[0], self.ns - 1}) == 3
        assert min(self.lay.start(self.ns - 1, self.nb - 2), self.lay.start(self.ns - 1, self.nb - 1)) >= 2**32
        return ea, eb

    def placed(self):
        return [(self.lay, self.clean())]

    def outs(self):
        return []


def scrub_cases(fam, shapes):
    """Every shape under both geometries; the two-step paths once more under a
    64 KiB scratch cap, whose run cutting forms addresses of its own."""
    out = [Scrub(fam, k, m, nb, g, name, knob) for k, m, nb, name, knob in shapes
           for g in ("far_stripes", "far_blocks")]
    return out + [Scrub(fam, k, m, nb, "far_stripes", name, knob, scratch=65536) for k, m, nb, name, knob in shapes
                  if name.startswith("rows_")]


VERIFY = scrub_cases("verify", [(3, 10, 10, "matverify_reg<3,7>", None), (10, 16, 16, "matverify_bsr<6>", 1),
                                (6, 22, 22, "matverify_bsr<8,lds>", 1), (20, 60, 60, "matverify_bsr<10,lds,tbl>", 1),
                                (10, 16, 16, "rows_differ", FUSED_OFF)])
LOCATE = scrub_cases("locate", [(3, 10, 10, "matlocate_reg<3,7>", None), (10, 16, 16, "rows_locate", None)])
CORRECT = scrub_cases("correct", [(3, 10, 10, "matcorrect_reg<3>", None), (4, 12, 12, "matcorrect_reg<4>", None),
                                  (10, 16, 16, "rows_correct", None)])
MIXED = [Mixed(K, g) for K in (1, 2, 3, 4) for g in ("far_stripes", "far_blocks")]
REPAIR = [Repair(K, m, t, g) for K, m, t in ((3, 10, 7), (4, 12, 8)) for g in ("far_stripes", "far_blocks")]
APPLY = {"reg": REG, "rows": ROWS, "lds": LDS, "small": SMALL, "bsg": BSG, "bsr": BSR, "ks": KS, "jit": JIT}


def all_cases():
    """Every case of this module that places rows in an arena."""
    for cases in APPLY.values():
        for c in cases:
            yield c
    yield Pair()
    for c in MIXED + REPAIR + VERIFY + LOCATE + CORRECT:
        yield c


def ids(cases):
    return [c.id for c in cases]


# ---- the arenas ---------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


HELD = []  # bytes torch held on the device before the arenas were made


@pytest.fixture(scope="module")
def arenas():
    """(source, destination), the source at the lower address so that one
    positive block stride leads from it into the destination."""
    torch.cuda.reset_peak_memory_stats()
    HELD.append(torch.cuda.memory_allocated())
    src = far_arena.Arena(torch, BACKGROUND, far_arena.SRC_ODD)
    dst = far_arena.Arena(torch, GUARD, far_arena.DST_ODD)
    if src.t.data_ptr() > dst.t.data_ptr():
        src.t, dst.t = dst.t, src.t
        src.reset()
        dst.reset()
    torch.cuda.synchronize()
    yield src, dst
    del src.t, dst.t
    del src, dst
    torch.cuda.empty_cache()


def stream():
    return torch.cuda.current_stream().cuda_stream


def name_of(case):
    return case.name() if callable(case.name) else case.name


class Source(object):
    """Rows placed in the source arena for one call: its sum is taken once they
    lie there and must be the same once the call is done."""

    def __init__(self, src, placed, what):
        self.src, self.placed, self.what = src, placed, what

    def __enter__(self):
        for lay, blocks in self.placed:
            self.src.place(lay, blocks)
        self.before = self.src.total()
        return self

    def unchanged(self):
        torch.cuda.synchronize()
        judge_source(self.before, self.src.total(), self.what)

    def __exit__(self, kind, value, tb):
        if kind is None:
            for lay, _ in self.placed:
                self.src.clear(lay)
        else:
            self.src.reset()


def run_apply(arenas, case):
    src, dst = arenas
    blocks, want, index, flags = case.build()
    lin, lout = case.lin, case.lout
    code = capi.Code(case.k, case.m)
    f = code.encode_batch if case.op == "enc" else code.decode_batch
    with Source(src, [(lin, blocks)], case.id) as placed:
        f(src.base, lin.bs, lin.ss, dst.base, lout.bs, lout.ss, index, case.sz, case.ns, stream=stream(),
          flags=capi.FEC_FLAG_ASYNC | flags)
        torch.cuda.synchronize()
        name = capi.last_kernel_name()
        dst.check(lout, want, (case.id, name))
        placed.unchanged()
    return name


# ---- encode and decode kernels --------------------------------------------------------------------

@pytest.mark.parametrize("case", REG, ids=ids(REG))
def test_reg(arenas, jit_off, case):
    """matapply_reg's walking form: <3,7> (prefetching, tables read from the
    argument segment), <4,8>, and the plain walk of the 3-row decode."""
    assert run_apply(arenas, case) == case.name


@pytest.mark.parametrize("case", ROWS, ids=ids(ROWS))
def test_rows(arenas, jit_off, case):
    assert run_apply(arenas, case) == case.name


def test_pair(arenas, jit_off):
    src, dst = arenas
    case = Pair()
    (a_in, a_want, a_idx), (b_in, b_want, b_idx) = case.build()
    code = capi.Code(3, 10)
    la, lb = case.lin.sub(0, 3), case.lin.sub(3, 3)
    oa, ob = case.lout.sub(0, 7), case.lout.sub(7, 3)
    jobs = capi.BatchJobs([
        capi.encode_job(code, src.base + la.first, la.bs, la.ss, dst.base + oa.first, oa.bs, oa.ss, a_idx, case.sz,
                        case.ns),
        capi.decode_job(code, src.base + lb.first, lb.bs, lb.ss, dst.base + ob.first, ob.bs, ob.ss, b_idx, case.sz,
                        case.ns)])
    with Source(src, [(la, a_in), (lb, b_in)], case.id) as placed:
        jobs.run(stream())
        torch.cuda.synchronize()
        name = capi.last_kernel_name()
        dst.check(case.lout, np.concatenate([a_want, b_want], axis=1), (case.id, name))
        placed.unchanged()
    assert name == case.name


@pytest.mark.parametrize("case", LDS, ids=ids(LDS))
def test_lds(arenas, lds_only, case):
    assert run_apply(arenas, case) == case.name


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_small(arenas, jit_off, case):
    """At the default ZFEC_HIP_SMALL_LANES: three stripes of 4097 bytes are 1539 lanes."""
    assert run_apply(arenas, case) == case.name


@pytest.mark.parametrize("case", BSG, ids=ids(BSG))
def test_bsg(arenas, bsg_only, case):
    name = run_apply(arenas, case)
    assert name == name_of(case)
    assert name.endswith(",tbl>") == (case.k == 20), name


@pytest.mark.parametrize("case", BSR, ids=ids(BSR))
def test_bsr(arenas, bsr_only, case):
    assert run_apply(arenas, case) == case.name


@pytest.mark.parametrize("case", KS, ids=ids(KS))
def test_bsr_ks(arenas, bsr_only, case):
    assert run_apply(arenas, case) == case.name


@pytest.mark.parametrize("case", JIT, ids=ids(JIT))
def test_generated(arenas, force_jit, case):
    """One shape per generated form: one tile, ksplit, split without LDS, resident, DMA phases."""
    name = run_apply(arenas, case)
    assert name.startswith(case.name), (case.id, name)


# ---- a pattern per stripe -------------------------------------------------------------------------

def device_ids(ids_):
    return torch.from_numpy(np.ascontiguousarray(ids_, dtype=np.uint32).view(np.int32)).cuda()


@pytest.mark.parametrize("case", MIXED, ids=ids(MIXED))
def test_mixed(arenas, case):
    src, dst = arenas
    recv, want, pats, ids_ = case.build()
    keep = device_ids(ids_)
    code = capi.Code(case.k, case.m)
    with Source(src, [(case.lin, recv)], case.id) as placed:
        code.decode_batch_mixed(src.base, case.lin.bs, case.lin.ss, dst.base, case.lout.bs, case.lout.ss, pats,
                                keep.data_ptr(), case.sz, case.ns, stream=stream())
        torch.cuda.synchronize()
        name = capi.last_kernel_name()
        dst.check(case.lout, want, (case.id, name))
        placed.unchanged()
    assert name == case.name


@pytest.mark.parametrize("case", REPAIR, ids=ids(REPAIR))
def test_repair(arenas, case):
    src, dst = arenas
    recv, want, pres, tgts, ids_ = case.build()
    keep = device_ids(ids_)
    code = capi.Code(case.k, case.m)
    with Source(src, [(case.lin, recv)], case.id) as placed:
        code.repair_batch(src.base, case.lin.bs, case.lin.ss, dst.base, case.lout.bs, case.lout.ss, pres, tgts,
                          keep.data_ptr(), case.sz, case.ns, stream=stream())
        torch.cuda.synchronize()
        name = capi.last_kernel_name()
        dst.check(case.lout, want, (case.id, name))
        placed.unchanged()
    assert name == case.name


# ---- scrub: verify, locate, correct -----------------------------------------------------------------

class Words(object):
    """n uint32 words on the device, pre-filled, between guard words."""

    def __init__(self, n):
        self.n = n
        self.t = torch.from_numpy(np.full(GW + n + GW, FILL, dtype=np.uint32).view(np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * GW

    def read(self, what):
        got = self.t.cpu().numpy().view(np.uint32)
        assert (got[:GW] == FILL).all() and (got[GW + self.n:] == FILL).all(), ("guard words", what)
        return got[GW:GW + self.n].copy()


def corrupted(clean, cor):
    blocks = clean.copy()
    for s, j, x, v in cor:
        blocks[s, j, x] ^= v
    return blocks


@pytest.mark.parametrize("case", VERIFY, ids=ids(VERIFY))
def test_verify(arenas, knobs, case):
    """Clean, then one byte flipped in a row past 2^31 and one in a row past
    2^32: the masks against test_gpu_verify.expected_bits."""
    src, _ = arenas
    case.set_knobs(knobs)
    code = capi.Code(case.k, case.m)
    P = verify.check_rows(case.k, case.m, tuple(case.nums))
    clean = case.clean()
    (sa, ja), (sb, jb) = case.far_errors()
    lay, W = case.lay, (case.c + 31) // 32
    for what, cor in (("clean", []), ("far", [(sa, ja, case.sz - 1, 0x01), (sb, jb, 1024, 0x80)])):
        with Source(src, [(lay, corrupted(clean, cor))], (case.id, what)) as placed:
            words = Words(case.ns * W)
            code.verify_batch(src.base, lay.bs, lay.ss, case.nums, case.sz, case.ns, words.ptr, stream=stream())
            torch.cuda.synchronize()
            name = capi.last_kernel_name()
            got = words.read((case.id, what)).reshape(case.ns, W)
            want = verify.pack(verify.expected_bits(P, case.k, case.ns, cor))
            assert (got == want).all(), (case.id, what, name, np.argwhere(got != want)[:4].tolist())
            assert bool(want.any()) == bool(cor)
            placed.unchanged()
        assert name == case.name, (case.id, what, name)


def locate_errors(case):
    """The two far single errors and a double error in the last stripe."""
    (sa, ja), (sb, jb) = case.far_errors()
    s = case.ns - 1
    return [(sa, ja, case.sz - 1, 0x01), (sb, jb, 1024, 0x80), (s, case.nb - 2, 17, 0x21), (s, case.nb - 1, 17, 0x42)]


@pytest.mark.parametrize("case", LOCATE, ids=ids(LOCATE))
def test_locate(arenas, knobs, case):
    src, _ = arenas
    case.set_knobs(knobs)
    code = capi.Code(case.k, case.m)
    P, Q = oracle_PQ(case.k, case.m, tuple(case.nums))
    clean = case.clean()
    lay = case.lay
    for what, cor in (("clean", []), ("far", locate_errors(case))):
        blocks = corrupted(clean, cor)
        want = verdicts(P, Q, blocks)
        if cor:
            (sa, ja), (sb, jb) = case.far_errors()
            assert want[sa] == ja and want[sb] == jb and want[case.ns - 1] >= case.nb, want.tolist()
            assert np.count_nonzero(want != CLEAN) == 3
        with Source(src, [(lay, blocks)], (case.id, what)) as placed:
            words = Words(case.ns)
            code.locate_batch(src.base, lay.bs, lay.ss, case.nums, case.sz, case.ns, words.ptr, stream=stream())
            torch.cuda.synchronize()
            name = capi.last_kernel_name()
            got = words.read((case.id, what))
            assert (got == want).all(), (case.id, what, name, [(int(i), hex(got[i]), hex(want[i]))
                                                                for i in np.nonzero(got != want)[0][:4]])
            placed.unchanged()
        assert name == case.name, (case.id, what, name)


@pytest.mark.parametrize("case", CORRECT, ids=ids(CORRECT))
def test_correct(arenas, knobs, case):
    """In place in the source arena: culprits in the far stripes (far_blocks:
    the far slots) and one near the base; the bytes of the whole arena other
    than the background are counted against the model's blocks; a second call
    finds every stripe CLEAN and writes nothing."""
    src, _ = arenas
    case.set_knobs(knobs)
    code = capi.Code(case.k, case.m)
    P, Q = oracle_PQ(case.k, case.m, tuple(case.nums))
    (sa, ja), (sb, jb) = case.far_errors()
    blocks = corrupted(case.clean(), [(sa, ja, case.sz - 1, 0x01), (sb, jb, 1024, 0x80), (0, 0, 5, 0x33)])
    want, after = corrected(P, Q, blocks)
    assert want[sa] == ja and want[sb] == jb and want[0] == 0 and np.count_nonzero(want != CLEAN) == 3
    assert (after == case.clean()).all()
    lay = case.lay
    src.place(lay, blocks)
    try:
        for what, expect in (("first", want), ("second", np.full(case.ns, CLEAN, dtype=np.uint32))):
            words = Words(case.ns)
            code.correct_batch(src.base, lay.bs, lay.ss, case.nums, case.sz, case.ns, words.ptr, stream=stream())
            torch.cuda.synchronize()
            name = capi.last_kernel_name()
            got = words.read((case.id, what))
            assert (got == expect).all(), (case.id, what, name, [(int(i), hex(got[i]), hex(expect[i]))
                                                                  for i in np.nonzero(got != expect)[0][:4]])
            judge(src.gather(lay), after, src.count_not(BACKGROUND), BACKGROUND, (case.id, what, name))
            assert name == case.name, (case.id, what, name)
    except BaseException:
        src.reset()
        raise
    src.clear(lay)


# ---- one block longer than 4 GiB ----------------------------------------------------------------------

def test_one_block_past_4gib(arenas, jit_off):
    """k = 1, m = 2, sz = 2^32 + 4097: the primary in the source arena, the
    parity in the destination arena, through the single-stripe call (the
    one-unit-per-lane form of matapply_reg).  The parity row of this code is
    [1], so the parity equals the primary over the whole length; the oracle
    confirms it on the bytes around 0, 2^31 and 2^32.  Then verify_batch with
    the parity as the one check.  Wider codes at this length need tens of GiB
    of blocks and are deliberately left out."""
    src, dst = arenas
    sz = BIG
    assert sz <= far_arena.SPAN
    lo_s, lo_d = far_arena.LEAD + src.odd, far_arena.LEAD + dst.odd
    prim, par = src.t[lo_s:lo_s + sz], dst.t[lo_d:lo_d + sz]
    # an odd period: the bytes 2^31 or 2^32 away are never the same bytes
    period = 2**26 + 1
    rnd = torch.from_numpy(np.random.default_rng(far_arena.SEED).integers(0, 256, size=period, dtype=np.uint8)).cuda()
    try:
        for a in range(0, sz, period):
            n = min(period, sz - a)
            prim[a:a + n] = rnd[:n]
        before = src.total()
        code = capi.Code(1, 2)
        code.encode_ptrs([src.base], [dst.base], [1], sz, stream=stream())
        torch.cuda.synchronize()
        assert capi.last_kernel_name() == "matapply_reg<1,1>"
        for a in range(0, sz, far_arena.CHUNK):
            b = a + far_arena.CHUNK
            assert torch.equal(par[a:b], prim[a:b]), ("parity differs in the chunk at", a)
        for a, b in ((0, 4096), (2**31 - 2048, 2**31 + 2048), (2**32 - 2048, sz)):
            want = oracle.encode(1, 2, prim[a:b].cpu().numpy()[None, :])
            assert (par[a:b].cpu().numpy() == want[0]).all(), (a, b)
        assert dst.count_not(GUARD) == src.count_not(GUARD, lo_s, lo_s + sz)
        judge_source(before, src.total(), "encode")

        bs = dst.base - src.base
        assert bs > 0
        for flip, want in ((0, 0), (1, 1)):
            if flip:
                par[2**32 + 4000] ^= 0x10
            words = Words(1)
            code.verify_batch(src.base, bs, 2 * bs, [0, 1], sz, 1, words.ptr, stream=stream())
            torch.cuda.synchronize()
            assert capi.last_kernel_name() == "matverify_reg<1,1>"
            assert words.read(("verify", flip)).tolist() == [want], flip
        judge_source(before, src.total(), "verify")
    finally:
        prim.fill_(BACKGROUND)
        par.fill_(GUARD)
        torch.cuda.synchronize()


# ---- the staged host path ---------------------------------------------------------------------------------

ROOM = 64


@pytest.mark.parametrize("case", [REG[0], REG[2]], ids=ids([REG[0], REG[2]]))
def test_staged_pageable_host(case):
    """The 3/10 far_stripes encode and decode from a pageable numpy arena of the
    same lead and span into a second one (np.empty: only the touched pages become
    resident).  The output arena is pre-filled with 0xA5 around every row and
    around every row's aliases; afterwards those zones must hold the oracle's
    rows in their true places and 0xA5 elsewhere, 64 bytes on each side
    included.  No page-locked arena: pinning 6.5 GiB touches every page."""
    blocks, want, index, _ = case.build()
    lin, lout = case.lin, case.lout
    size = far_arena.LEAD + far_arena.SPAN + far_arena.TAIL
    hsrc, hdst = np.empty(size, dtype=np.uint8), np.empty(size, dtype=np.uint8)
    sb, db = far_arena.LEAD + far_arena.SRC_ODD, far_arena.LEAD + far_arena.DST_ODD

    def zones(lay):
        return sorted({p - ROOM for _, _, o in lay.starts() for p in (o,) + far_arena.aliases(o)})

    for z in zones(lin):
        hsrc[sb + z:sb + z + lin.sz + 2 * ROOM] = BACKGROUND
    for s, j, o in lin.starts():
        hsrc[sb + o:sb + o + lin.sz] = blocks[s, j]
    for z in zones(lout):
        hdst[db + z:db + z + lout.sz + 2 * ROOM] = GUARD
    model = far_arena.Sparse(GUARD)
    model.place(lout, want)
    code = capi.Code(case.k, case.m)
    f = code.encode_batch if case.op == "enc" else code.decode_batch
    f(hsrc.ctypes.data + sb, lin.bs, lin.ss, hdst.ctypes.data + db, lout.bs, lout.ss, index, case.sz, case.ns, flags=0)
    got = np.stack([np.stack([hdst[db + lout.start(s, j):][:lout.sz] for j in range(lout.rows)])
                    for s in range(lout.ns)])
    judge(got, want, int(np.count_nonzero(want != GUARD)), GUARD, case.id)
    for z in zones(lout):
        n = lout.sz + 2 * ROOM
        assert (hdst[db + z:db + z + n] == model.read(z, n)).all(), (case.id, "a write around a row or at an alias", z)
    for s, j, o in lin.starts():
        assert (hsrc[sb + o:sb + o + lin.sz] == blocks[s, j]).all(), (case.id, "the source was written", s, j)


def test_device_checker_rejects_a_row_at_its_alias(arenas):
    """The checker itself on the device, fed by torch alone (no kernel is
    broken for it): the right rows pass; with one far row also present 2^32
    bytes early the count over the arena rejects them; with that row only
    there, the gathered rows do.  tests/test_far_layout.py holds the same rules
    on a model of the arena."""
    _, dst = arenas
    # one stripe past 2^32 whose aliases lie on no other row
    lay = Layout("far_stripes", 7, SZ, ns=1, first=2**32 + 2**20, strides=far_arena.far_stripes(7, SZ))
    want = far_arena.data(1, lay.ns, lay.rows, lay.sz)
    s, j = lay.far_rows()[1]
    o = lay.start(s, j)
    alias = far_arena.LEAD + dst.odd + o % 2**32
    assert o >= 2**32 and (dst.t[alias - 64:alias + lay.sz + 64] == GUARD).all()
    dst.place(lay, want)
    dst.check(lay, want, "right")
    row = torch.from_numpy(want[s, j]).cuda()
    dst.place(lay, want)
    dst.t[alias:alias + lay.sz] = row
    with pytest.raises(AssertionError, match="in the whole arena"):
        dst.check(lay, want, "as well")
    dst.place(lay, want)
    dst.row(lay, s, j).fill_(GUARD)
    dst.t[alias:alias + lay.sz] = row
    with pytest.raises(AssertionError, match="only untouched bytes"):
        dst.check(lay, want, "instead")
    dst.t[17] = 0
    with pytest.raises(AssertionError, match="in the whole arena"):
        dst.check(lay, np.full_like(want, GUARD), "one byte in the lead")
    assert dst.count_not(GUARD) == 0


def test_device_memory_stays_under_16_gib(arenas):
    """Runs last: the most this module held at once, arenas, per-call blocks
    and counting slices together."""
    peak = torch.cuda.max_memory_allocated() - HELD[0]
    print("far-offset module: peak device memory %.2f GiB" % (peak / 2**30))
    assert 2 * far_arena.SPAN < peak < 16 * 2**30
