"""GPU parity of the batched parity update (fec_update_batch; matupdate_reg<C, R>
in zfec_amd/csrc/kernels.hip).  Expected bytes never come from the library:
random stripes are encoded with the CPU oracle (zfec/fec.c:487-505), the changed
primaries replaced, and the stripes encoded again with the oracle; the rows
after the call must equal the second encode.  The row buffer carries 0xA5
guards before, between (padded layouts) and after the rows; inputs start at
byte offset 3 and rows at byte offset 5 (the helpers of test_gpu_mixed).

The kernel XORs into its output, so a block must end with the byte tail, not
with a last chunk shifted back over its neighbour.  What the sizes can show:
at 17 and 1023 the shifted chunk would sit in its neighbour's wave, where
every load precedes every store, so both lanes would store identical, correct
bytes; 1040 is 65 whole chunks and has no tail at all.  The overlapped form
goes wrong only where the tail chunk is lane 0 of a NEW wave (sz = 1024 w + t,
0 < t < 16): test_tail_chunk_in_its_own_wave has those sizes, under the
default grid, where the two waves race, and under ZFEC_HIP_GRID_CAP=1 and 2,
where the tail's wave runs a step after its neighbour has stored."""
import numpy as np
import pytest

import zfec_amd
from zfec_amd import capi
from oracle import oracle

import far_arena
from test_gpu_mixed import GUARD, IN_OFF, OUT_OFF, TAIL, Layout, stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NONE = capi.FEC_UPDATE_NONE


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if zfec_amd.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")


def encode_all(k, m, data):
    """All m blocks (ns, m, sz) of the stripes data (ns, k, sz), by the oracle."""
    ns, _, sz = data.shape
    flat = np.ascontiguousarray(data.transpose(1, 0, 2)).reshape(k, ns * sz)
    par = oracle.encode(k, m, flat).reshape(m - k, ns, sz).transpose(1, 0, 2)
    return np.concatenate([data, par], axis=1)


def random_changed(rng, k, ns, c, none=0.25):
    """(ns, c) primary numbers, about a quarter of the slots -1 (none)."""
    ch = rng.integers(0, k, size=(ns, c))
    ch[rng.random((ns, c)) < none] = -1
    return ch


class Update(object):
    """One call's buffers.  `changed` is (ns, c) int64, -1 for none; slot
    (s, c) carries a random delta, and in the old/new form random `old` bytes
    with new = old ^ delta.  A none slot's inputs hold random bytes that must
    not matter.  `words` (optional) replaces the uint32 words handed to the
    library (numbers the host cannot check); `changed` then says what they
    should amount to."""

    def __init__(self, k, m, nums, changed, sz, kind="padded", form="delta", szmax=None, seed=0, device_mem=True,
                 deltas=None, base=None):
        changed = np.asarray(changed, dtype=np.int64)
        self.k, self.m, self.nums, self.sz, self.form = k, m, list(nums), sz, form
        self.ns, self.c = changed.shape
        self.changed = changed
        ns, c = self.ns, self.c
        if base is None:
            base = stripes(k, m, ns, szmax or sz, seed)[1]
        self.before = np.ascontiguousarray(base[:, :, :sz])  # all m blocks (ns, m, sz)
        rng = np.random.default_rng([k, m, ns, sz, c, seed])
        self.deltas = rng.integers(0, 256, size=(ns, c, sz), dtype=np.uint8) if deltas is None else deltas
        junk = rng.integers(0, 256, size=(ns, c, sz), dtype=np.uint8)
        data = self.before[:, :k].copy()
        for s in range(ns):
            for i in range(c):
                if changed[s, i] >= 0:
                    data[s, changed[s, i]] ^= self.deltas[s, i]
        self.after = encode_all(k, m, data)
        self.want = self.after[:, self.nums]
        # inputs
        self.lin = Layout(kind, ns, c, sz)
        old = rng.integers(0, 256, size=(ns, c, sz), dtype=np.uint8)
        live = (changed >= 0)[:, :, None]
        if form == "delta":
            new = np.where(live, self.deltas, junk)
            old = None
        else:
            new = np.where(live, old ^ self.deltas, junk)
        self.newb = self.place_in(new, device_mem)
        self.oldb = self.place_in(old, device_mem) if old is not None else None
        # rows: guards everywhere but in the rows
        self.lout = Layout(kind, ns, len(self.nums), sz)
        rows = np.full(OUT_OFF + self.lout.nbytes + TAIL, GUARD, dtype=np.uint8)
        self.lout.view(rows[OUT_OFF:OUT_OFF + self.lout.nbytes])[:, :, :sz] = self.before[:, self.nums]
        self.rows0 = rows
        t = torch.from_numpy(rows.copy())
        self.rows = t.cuda() if device_mem else t.pin_memory()
        self.keep = None

    def place_in(self, blocks, device_mem):
        buf = np.zeros(IN_OFF + self.lin.nbytes + TAIL, dtype=np.uint8)
        self.lin.view(buf[IN_OFF:IN_OFF + self.lin.nbytes])[:, :, :self.sz] = blocks
        t = torch.from_numpy(buf)
        return t.cuda() if device_mem else t.pin_memory()

    def launch(self, code, where="host", stream=None, flags=capi.FEC_FLAG_ASYNC, words=None):
        w = self.changed & 0xFFFFFFFF if words is None else np.asarray(words, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.uint32)
        if where == "device":
            self.keep = torch.from_numpy(w.view(np.int32)).cuda()
            ptr = self.keep.data_ptr()
        else:
            self.keep = w
            ptr = w.ctypes.data
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        code.update_batch(self.oldb.data_ptr() + IN_OFF if self.oldb is not None else 0, self.newb.data_ptr() + IN_OFF,
                          self.lin.bs, self.lin.ss, self.rows.data_ptr() + OUT_OFF, self.lout.bs, self.lout.ss,
                          self.nums, ptr, self.c, self.sz, self.ns, stream=st, flags=flags)
        return capi.last_kernel_name()

    def result(self, what=""):
        """The rows (ns, r, sz), the guards checked; and the whole buffer."""
        torch.cuda.synchronize()
        host = self.rows.cpu().numpy()
        n = self.lout.nbytes
        assert (host[:OUT_OFF] == GUARD).all(), ("write before the rows", what)
        assert (host[OUT_OFF + n:] == GUARD).all(), ("write after the rows", what)
        body = self.lout.view(host[OUT_OFF:OUT_OFF + n])
        assert (body[:, :, self.sz:] == GUARD).all(), ("write past a row", what)
        return body[:, :, :self.sz], host

    def check(self, what=""):
        got, host = self.result(what)
        if not (got == self.want).all():
            bad = np.argwhere((got != self.want).any(axis=2))
            s, i = bad[0]
            x = int(np.argmax(got[s, i] != self.want[s, i]))
            raise AssertionError((what, "wrong (stripe, row)", bad[:6].tolist(), "first wrong byte", x))
        return host


def run(k, m, nums, changed, sz, kind="padded", form="delta", where="host", name=None, **kw):
    u = Update(k, m, nums, changed, sz, kind, form, **kw)
    got_name = u.launch(capi.Code(k, m), where)
    what = (k, m, len(nums), u.c, sz, kind, form, where, got_name)
    if name is not None:
        assert got_name == name, what
    return u.check(what)


# ---- 1. the sweep ----------------------------------------------------------------------------

SIZES = (1, 15, 16, 17, 1023, 1024, 1040, 4096)


@pytest.mark.parametrize("form", ["oldnew", "delta"])
@pytest.mark.parametrize("kind", ["packed", "padded", "bm"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_sweep(C, kind, form):
    """K=3/M=10, all 7 parity rows of 37 stripes, each stripe with its own
    changed numbers and some slots none: the byte tail alone (1, 15), exact
    chunks (16, 1024), a chunk and a tail (17), 63 chunks and a tail (1023), a
    second wave with one live lane (1040) and four waves per stripe."""
    k, m, ns = 3, 10, 37
    rng = np.random.default_rng(C)
    changed = random_changed(rng, k, ns, C)
    changed[0], changed[1] = -1, 0  # a stripe with no live slot, and one with the same block in every slot
    for sz in SIZES:
        run(k, m, range(k, m), changed, sz, kind, form, name="matupdate_reg<%d,7>" % C, szmax=max(SIZES))


TAIL_SIZES = (2056, 2049, 2063, 4100, 1025, 1030, 1039)  # three and five waves per stripe first: see below


@pytest.mark.parametrize("form", ["oldnew", "delta"])
@pytest.mark.parametrize("cap", [None, 2, 1])
def test_tail_chunk_in_its_own_wave(knobs, cap, form):
    """sz = 1024 w + t with 0 < t < 16: the byte tail is lane 0 of wave w, and the
    chunk before it lane 63 of wave w - 1.  A last chunk shifted back to end at
    sz would overlap that chunk from ANOTHER wave, and whichever wave comes
    second would read what the first stored and apply the delta again.  Under
    the default grid the two waves run side by side and the overlap may go
    unseen.  With ONE workgroup (4 waves) and three waves per stripe (2049,
    2056, 2063) the tail wave of stripes 2, 6, 10, ... is wave number 3 s + 2,
    a multiple of 4: the first unit of a wave's NEXT step, when its neighbour's
    store is a step old (five waves per stripe, 4100: stripes 0, 4, 8, ...).  A
    build with the overlapped chunk fails there at stripe 2, byte sz - 16.  With
    two workgroups the same holds for every eighth stripe as long as the
    workgroups keep pace; that build failed there too, at later stripes."""
    if cap is not None:
        knobs(ZFEC_HIP_GRID_CAP=cap)
    k, m, ns = 3, 10, 37
    changed = random_changed(np.random.default_rng(cap or 0), k, ns, 2, none=0.0)
    for sz in TAIL_SIZES:
        run(k, m, range(k, m), changed, sz, form=form, name="matupdate_reg<2,7>", szmax=max(TAIL_SIZES))


# ---- 2. every <C, R> and the row groups ------------------------------------------------------

@pytest.mark.parametrize("R", range(1, 9))
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_every_instantiation(C, R):
    """K = C primaries, R parity rows and C input slots: matupdate_reg<C, R>."""
    k, m, ns = C, C + R, 37
    changed = random_changed(np.random.default_rng(10 * C + R), k, ns, C)
    run(k, m, range(k, m), changed, 1040, form="oldnew" if R % 2 else "delta", name="matupdate_reg<%d,%d>" % (C, R))


@pytest.mark.parametrize("k,m,ns,C,last", [(4, 20, 37, 2, 8), (10, 16, 37, 3, 6), (20, 24, 37, 1, 4),
                                           (20, 60, 5, 4, 8), (128, 256, 3, 2, 8)])
def test_row_groups(k, m, ns, C, last):
    """More than 8 rows are row groups of 8 over one upload: 16 rows two
    launches, 40 rows five, 128 rows sixteen (four mask dwords per record)."""
    changed = random_changed(np.random.default_rng(k + m), k, ns, C)
    run(k, m, range(k, m), changed, 1040, name="matupdate_reg<%d,%d>" % (C, last))


def test_uneven_last_group():
    """K=4/M=15: 11 rows, a group of 8 and one of 3."""
    changed = random_changed(np.random.default_rng(15), 4, 37, 2)
    run(4, 15, range(4, 15), changed, 1040, name="matupdate_reg<2,3>")


# ---- 3. none and skipping ----------------------------------------------------------------------

def test_all_none_is_untouched():
    k, m, ns, sz = 3, 10, 37, 1040
    for where in ("host", "device"):
        u = Update(k, m, range(k, m), np.full((ns, 3), -1), sz, form="oldnew")
        u.launch(capi.Code(k, m), where)
        host = u.check(where)
        assert (host == u.rows0).all(), where


@pytest.mark.parametrize("bad", [3, 4, 255, 0x7FFFFFFF, 0xFFFFFFFE])
def test_device_side_bad_number_is_none(bad):
    """A device-side number that is not < k (k itself included) leaves its slot
    unapplied; the stripe's other slots are applied."""
    k, m, ns, sz = 3, 10, 37, 1040
    rng = np.random.default_rng(bad % 1000)
    changed = random_changed(rng, k, ns, 3, none=0.0)
    words = changed.copy()
    hit = rng.random((ns, 3)) < 0.4
    hit[2] = True           # every slot of one stripe
    hit[3] = [False, True, False]
    words[hit] = bad
    changed[hit] = -1       # what the call should amount to
    u = Update(k, m, range(k, m), changed, sz)
    u.launch(capi.Code(k, m), "device", words=words)
    host = u.check(bad)
    assert (u.lout.view(host[OUT_OFF:OUT_OFF + u.lout.nbytes])[2, :, :sz] == u.before[2, k:]).all()


# ---- 4. primary rows ---------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,C", [(3, 10, 1), (3, 10, 3), (10, 16, 2)])
def test_primary_rows(k, m, C):
    """The rows are a whole stored stripe in a shuffled order: the changed
    primary's row becomes the new block, every other primary row is unchanged
    (its coefficient is zero: neither read nor written), parity rows follow."""
    ns, sz = 37, 1040
    rng = np.random.default_rng(m)
    nums = rng.permutation(m).tolist()
    changed = random_changed(rng, k, ns, C)
    u = Update(k, m, nums, changed, sz)
    u.launch(capi.Code(k, m))
    got, _ = u.result()
    for s in range(ns):
        touched = set(int(j) for j in changed[s] if j >= 0)
        for i, b in enumerate(nums):
            if b < k and b not in touched:
                assert (got[s, i] == u.before[s, b]).all(), ("an unchanged primary row moved", s, b)
            elif b < k:
                assert (got[s, i] == u.after[s, b]).all(), ("the changed primary's row is not the new block", s, b)
    assert (got == u.want).all()


# ---- 5. the same block in two slots ---------------------------------------------------------------

def test_same_block_in_two_slots():
    k, m, ns, sz = 3, 10, 37, 1040
    rng = np.random.default_rng(5)
    j = rng.integers(0, k, size=ns)
    two = Update(k, m, range(k, m), np.stack([j, j], axis=1), sz)
    two.launch(capi.Code(k, m))
    a = two.check("two slots")
    one = Update(k, m, range(k, m), j[:, None], sz, deltas=two.deltas[:, :1] ^ two.deltas[:, 1:])
    one.launch(capi.Code(k, m))
    b = one.check("one slot with d1 ^ d2")
    assert (a == b).all()


# ---- 6. the walk -------------------------------------------------------------------------------

@pytest.mark.parametrize("sz", [1040, 4096, 3000])
def test_grid_stride(knobs, sz):
    """Two workgroups (8 waves) walk 37 stripes of 2, 4 or 3 waves each; with 3
    waves per stripe a step is 2 stripes and 2 waves (gs_w != 0), so the carry
    of the walk runs."""
    knobs(ZFEC_HIP_GRID_CAP=2)
    k, m, ns = 3, 10, 37
    changed = random_changed(np.random.default_rng(sz), k, ns, 2)
    run(k, m, range(k, m), changed, sz, form="oldnew", name="matupdate_reg<2,7>", szmax=4096)


@pytest.mark.parametrize("sz,ns", [(4096, 37), (20000, 5)])
def test_split_launches(knobs, sz, ns):
    """ZFEC_HIP_LAUNCH_UNITS=1024: 4 KiB stripes go in groups of 4 (the changed
    pointer advanced per group), 20000-byte blocks in byte ranges of 16 KiB --
    a read-modify-write cut into ranges must apply each byte exactly once."""
    knobs(ZFEC_HIP_LAUNCH_UNITS=1024)
    k, m = 3, 10
    changed = random_changed(np.random.default_rng(sz), k, ns, 3)
    for where in ("host", "device"):
        run(k, m, range(k, m), changed, sz, where=where, name="matupdate_reg<3,7>", seed=1)


# ---- 7. host- and device-side numbers --------------------------------------------------------------

def test_host_and_device_numbers_identical():
    k, m, ns, sz = 3, 10, 37, 1040
    changed = random_changed(np.random.default_rng(7), k, ns, 2)
    a = run(k, m, range(k, m), changed, sz, where="host", szmax=4096)
    b = run(k, m, range(k, m), changed, sz, where="device", szmax=4096)
    assert (a == b).all()


def test_id_width():
    """66,000 stripes of one chunk: more stripes (and waves) than 16 bits count."""
    k, m, ns, sz = 3, 10, 66000, 16
    changed = random_changed(np.random.default_rng(66), k, ns, 1)
    a = run(k, m, range(k, m), changed, sz, "packed", where="host")
    b = run(k, m, range(k, m), changed, sz, "packed", where="device")
    assert (a == b).all()


# ---- 8. composition ------------------------------------------------------------------------------

def test_two_updates_compose():
    """j1 then j2 equals the oracle's encode of the twice-changed stripe; the
    same delta applied twice restores the original rows bit for bit."""
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    rng = np.random.default_rng(8)
    first = Update(k, m, range(k, m), random_changed(rng, k, ns, 1, none=0.0), sz)
    first.launch(code)
    first.check("first")
    second = Update(k, m, range(k, m), random_changed(rng, k, ns, 1, none=0.0), sz, seed=1, base=first.after)
    second.rows = first.rows  # the rows the first call left
    second.launch(code)
    second.check("second on top of the first")
    # the same two deltas again: back to the start
    first.launch(code)
    second.launch(code)
    torch.cuda.synchronize()
    assert (first.rows.cpu().numpy() == first.rows0).all()


# ---- 9. with the scrub -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(3, 10), (10, 16)])
def test_scrub_is_clean_after_an_update(k, m):
    ns, sz, r = 37, 2048, m - k
    code = capi.Code(k, m)
    u = Update(k, m, range(k, m), random_changed(np.random.default_rng(k), k, ns, 2), sz, kind="packed")
    u.launch(code)
    got, _ = u.result()
    stored = torch.from_numpy(np.ascontiguousarray(np.concatenate([u.after[:, :k], got], axis=1))).cuda()
    words = -(-r // 32)
    mism = torch.full((ns * words,), -1, dtype=torch.int32, device="cuda")
    code.verify_batch(stored.data_ptr(), sz, m * sz, list(range(m)), sz, ns, mism.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not mism.cpu().numpy().any()
    # and the scrub does see a stale parity: the rows before the update
    stale = torch.from_numpy(np.ascontiguousarray(np.concatenate([u.after[:, :k], u.before[:, k:]], axis=1))).cuda()
    code.verify_batch(stale.data_ptr(), sz, m * sz, list(range(m)), sz, ns, mism.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dirty = mism.cpu().numpy().view(np.uint32).reshape(ns, words)[:, 0] != 0
    assert (dirty == (u.changed >= 0).any(axis=1)).all()


# ---- 10. page-locked host buffers --------------------------------------------------------------------

@pytest.mark.parametrize("form", ["oldnew", "delta"])
def test_page_locked_host_memory(form):
    """Inputs and rows in page-locked host memory are read and updated in place."""
    k, m, ns, sz = 3, 10, 37, 1040
    u = Update(k, m, range(k, m), random_changed(np.random.default_rng(10), k, ns, 2), sz, form=form, device_mem=False)
    assert u.launch(capi.Code(k, m), flags=0) == "matupdate_reg<2,7>"
    u.check(form)


# ---- 11. two streams -----------------------------------------------------------------------------------

def test_two_streams():
    """Asynchronous calls back to back on two streams, each with its own
    records, more of them than the staging ring has slots."""
    k, ns, sz = 3, 37, 1040
    rng = np.random.default_rng(11)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cases = []
    for i in range(6):
        m = 6 + i  # another code, so other records, per call
        cases.append((capi.Code(k, m), Update(k, m, range(k, m), random_changed(rng, k, ns, 2), sz, seed=i)))
    torch.cuda.synchronize()
    for i, (code, u) in enumerate(cases):
        name = u.launch(code, "host" if i % 3 else "device", stream=streams[i % 2].cuda_stream)
        assert name == "matupdate_reg<2,%d>" % (3 + i)
    for i, (_, u) in enumerate(cases):
        u.check(i)


# ---- 12. graph capture -----------------------------------------------------------------------------------

def test_declines_under_graph_capture():
    k, m, ns, sz = 3, 10, 37, 1040
    code = capi.Code(k, m)
    changed = random_changed(np.random.default_rng(12), k, ns, 2)
    u = Update(k, m, range(k, m), changed, sz)
    x = torch.zeros(16, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            x.add_(1)
            with pytest.raises(capi.FecError, match="captured into a graph"):
                u.launch(code)
    torch.cuda.synchronize()
    assert (u.rows.cpu().numpy() == u.rows0).all()  # nothing was enqueued
    u.launch(code)  # a normal call afterwards works
    u.check("after the capture")


# ---- 13. offsets past 2^32 -------------------------------------------------------------------------------

def test_far_stripes():
    """Stripes just under 64 MiB apart in both arenas of far_arena.py: row 0 of
    stripe 32 straddles byte 2^31 and row 0 of stripe 64 byte 2^32 from the
    base, so s * stripe_stride needs all 64 bits, for the inputs and the rows."""
    k, m, sz, ns, C = 3, 10, 4097, far_arena.NS, 2
    r = m - k
    rng = np.random.default_rng(far_arena.SEED)
    base = stripes(k, m, ns, sz, seed=far_arena.SEED)[1]
    changed = random_changed(rng, k, ns, C)
    changed[32], changed[64], changed[69] = [0, 2], [1, 1], [-1, 2]
    u = Update(k, m, range(k, m), changed, sz, base=base, form="oldnew")
    src = far_arena.Arena(torch, far_arena.BACKGROUND, far_arena.SRC_ODD)
    dst = far_arena.Arena(torch, far_arena.GUARD, far_arena.DST_ODD)
    lin = far_arena.Layout("far_stripes", 2 * C, sz)  # old slots, then new slots, one stripe stride
    lout = far_arena.Layout("far_stripes", r, sz)
    assert lout.straddlers(2**31) and lout.straddlers(2**32) and lin.straddlers(2**32)
    body = u.lin.view(u.newb.cpu().numpy()[IN_OFF:IN_OFF + u.lin.nbytes])[:, :, :sz]
    obody = u.lin.view(u.oldb.cpu().numpy()[IN_OFF:IN_OFF + u.lin.nbytes])[:, :, :sz]
    try:
        src.place(lin, np.concatenate([obody, body], axis=1))
        dst.place(lout, u.before[:, k:])
        before = src.total()
        words = torch.from_numpy(np.ascontiguousarray(changed & 0xFFFFFFFF, dtype=np.uint32).view(np.int32)).cuda()
        capi.Code(k, m).update_batch(src.base, src.base + C * lin.bs, lin.bs, lin.ss, dst.base, lout.bs, lout.ss,
                                     list(range(k, m)), words.data_ptr(), C, sz, ns,
                                     stream=torch.cuda.current_stream().cuda_stream)
        assert capi.last_kernel_name() == "matupdate_reg<2,7>"
        dst.check(lout, u.want, "far_stripes")
        far_arena.judge_source(before, src.total(), "far_stripes")
    finally:
        src.t = dst.t = None
        torch.cuda.empty_cache()


# ---- 14. Encoder.update_batch ------------------------------------------------------------------------------

def test_python_api():
    k, m, ns, sz = 3, 10, 37, 1040
    enc = zfec_amd.Encoder(k, m)
    rng = np.random.default_rng(14)
    data = rng.integers(0, 256, size=(ns, k, sz), dtype=np.uint8)
    before = encode_all(k, m, data)

    def parity():
        return torch.from_numpy(np.ascontiguousarray(before[:, k:])).cuda()

    # one changed block per stripe: 1-D changed, [ns, sz] inputs, old and new
    j = rng.integers(0, k, size=ns)
    j[5] = -1
    newblk = rng.integers(0, 256, size=(ns, sz), dtype=np.uint8)
    oldblk = np.where((j >= 0)[:, None], data[np.arange(ns), np.maximum(j, 0)], 0).astype(np.uint8)
    data1 = data.copy()
    for s in range(ns):
        if j[s] >= 0:
            data1[s, j[s]] = newblk[s]
    want1 = encode_all(k, m, data1)[:, k:]
    new_t, old_t = torch.from_numpy(newblk).cuda(), torch.from_numpy(oldblk).cuda()
    forms = {"list": j.tolist(), "numpy": j, "host tensor": torch.from_numpy(j), "device tensor": torch.from_numpy(j).cuda(),
             "int32 numpy": j.astype(np.int32)}
    for what, form in forms.items():
        par = parity()
        out = enc.update_batch(par, form, new_t, old=old_t)
        assert out is par and capi.last_kernel_name() == "matupdate_reg<1,7>", what
        assert (out.cpu().numpy() == want1).all(), what
    # deltas (old=None), 2-D changed with two slots, [ns, c, sz] inputs
    ch2 = random_changed(rng, k, ns, 2)
    d2 = rng.integers(0, 256, size=(ns, 2, sz), dtype=np.uint8)
    data2 = data.copy()
    for s in range(ns):
        for c in range(2):
            if ch2[s, c] >= 0:
                data2[s, ch2[s, c]] ^= d2[s, c]
    all2 = encode_all(k, m, data2)
    for what, form in (("lists", ch2.tolist()), ("numpy", ch2), ("device tensor", torch.from_numpy(ch2).cuda())):
        out = enc.update_batch(parity(), form, torch.from_numpy(d2).cuda())
        assert capi.last_kernel_name() == "matupdate_reg<2,7>", what
        assert (out.cpu().numpy() == all2[:, k:]).all(), what
    # explicit blocknums: a parity node's two blocks, and a whole stripe with the primaries
    nums = [9, 4]
    out = enc.update_batch(torch.from_numpy(np.ascontiguousarray(before[:, nums])).cuda(), ch2, torch.from_numpy(d2).cuda(),
                           blocknums=nums)
    assert capi.last_kernel_name() == "matupdate_reg<2,2>" and (out.cpu().numpy() == all2[:, nums]).all()
    every = rng.permutation(m).tolist()
    out = enc.update_batch(torch.from_numpy(np.ascontiguousarray(before[:, every])).cuda(), ch2,
                           torch.from_numpy(d2).cuda(), blocknums=every)
    assert (out.cpu().numpy() == all2[:, every]).all()
    # block-major parity and inputs whose strides differ (old is made to match new)
    par = torch.from_numpy(np.ascontiguousarray(before[:, k:].transpose(1, 0, 2))).cuda().transpose(0, 1)
    wide = torch.zeros((ns, 2 * sz), dtype=torch.uint8, device="cuda")
    wide[:, :sz] = old_t
    out = enc.update_batch(par, j, new_t, old=wide[:, :sz])
    assert out.stride(0) < out.stride(1) and (out.cpu().numpy() == want1).all()
    # a host-side number the library would refuse, and a device-side one it takes for none
    with pytest.raises(zfec_amd.Error, match="but one was 3"):
        enc.update_batch(parity(), [3] * ns, new_t, old=old_t)
    out = enc.update_batch(parity(), torch.full((ns,), 3, dtype=torch.int64).cuda(), new_t, old=old_t)
    assert (out.cpu().numpy() == before[:, k:]).all()
    # nor does a 64-bit device-side number wrap into a primary: 2^32 + j is a none, not j
    for big in (2**32, 2**32 + 1, -2**32 + 2, -2):
        out = enc.update_batch(parity(), torch.full((ns,), big, dtype=torch.int64).cuda(), new_t, old=old_t)
        assert (out.cpu().numpy() == before[:, k:]).all(), big
