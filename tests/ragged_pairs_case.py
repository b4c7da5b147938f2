"""Shared by test_ragged_pairs_surface.py (CPU), test_gpu_ragged_locate2.py and
test_gpu_ragged_correct2.py: the CPU model of one ragged pair call
(fec_locate2_batch_ragged / fec_correct2_batch_ragged) over a
ragged_scrub_case.ScrubCase, the corruption lists the tests use, and the
harness that makes one call on the GPU.

The model is per stripe and comes from the CPU oracle alone: a stripe that
holds a corruption gets pair_ref.corrected2 (whose verdicts are
pair_ref.verdicts2's) on case.stripe_blocks(s), the (1, nb, sz) array the arena
holds; every other stripe is (CLEAN, NONE), which ScrubCase itself has checked
(no syndrome in the uncorrupted stripes).  No library call feeds it.  The
expected arena is built as test_gpu_ragged_correct.expected_arena builds it:
the arena on entry, gaps, lead and tail included, with the blocks of every
stripe whose verdict is a slot or a pair replaced -- here by the model's own
blocks after the correction."""
import itertools

import numpy as np

import locate_ref
import pair_ref
import ragged_scrub_case as sc

rc = sc.rc
NONE = pair_ref.NONE
CLEAN, MANY, UNKNOWN, UNFIT = sc.CLEAN, sc.MANY, sc.UNKNOWN, sc.UNFIT
GUARD_WORD, LEAD_W, TAIL_W = 0xDEADBEEF, 3, 5
NUMS8 = sc.NUMS + [3]  # K=3/M=10, c = 5: triples are refused


class Model(object):
    """planes: uint32 (2, ns), the two verdict words of every stripe.
    after: stripe -> its (nb, sz) blocks after fec_correct2_batch_ragged, for
    the stripes that hold a corruption.  unfit: stripes a test hands to the
    library with a descriptor that does not fit (device-side descriptors):
    (UNFIT, NONE), nothing healed."""

    def __init__(self, case, unfit=()):
        self.case = case
        P, Q = locate_ref.oracle_PQ(case.k, case.m, tuple(case.nums))
        self.planes = np.full((2, case.ns), NONE, dtype=np.uint32)
        self.planes[0] = CLEAN
        self.after = {}
        for s in sorted(set(s for s, _, _, _ in case.corrupt)):
            one = case.stripe_blocks(s)
            if s in unfit:
                continue
            v, after = pair_ref.corrected2(case.k, case.m, case.nums, P, Q, one)
            self.planes[:, s] = v[:, 0]
            self.after[s] = after[0]
        for s in unfit:
            self.planes[:, s] = (UNFIT, NONE)

    def healed(self):
        """The stripes whose verdict is a slot or a pair."""
        return [s for s in range(self.case.ns) if self.planes[0, s] < self.case.nb]

    def pair_of(self, s):
        a, b = int(self.planes[0, s]), int(self.planes[1, s])
        return (a, b) if b != NONE else None

    def expected_arena(self, tail=sc.TAIL, heal=True):
        case = self.case
        n = sc.IN_OFF + case.src_bytes
        want = np.concatenate([case.src[:n], np.full(tail, sc.BACKGROUND, dtype=np.uint8)])
        if heal:
            for s in self.healed():
                sz = case.sizes[s]
                for j in range(case.nb):
                    o = sc.IN_OFF + case.soff[s] + j * (case.sbs or sz)
                    want[o:o + sz] = self.after[s][j]
        return want


# ---- corruption lists ----------------------------------------------------------------------------------

PLACEMENTS = ("same byte", "one unit", "first and last", "overlapped chunk", "whole blocks")


def place_pair(s, a, b, sz, kind, n):
    """The (stripe, slot, byte, xor) entries of one pair stripe.  kind names a
    placement of PLACEMENTS; where the stripe is too short for it the bytes
    coincide, which is the first placement."""
    x, y = 1 + (37 * n) % 255, 1 + (91 * n + 7) % 255
    if kind == "same byte":
        pos = sc.positions(sz)
        p = pos[n % len(pos)]
        return [(s, a, p, x), (s, b, p, y)]
    if kind == "one unit":  # different bytes of the stripe's last 1 KiB unit
        u0 = (sz - 1) // 1024 * 1024
        return [(s, a, u0, x), (s, b, sz - 1, y)]
    if kind == "first and last":
        return [(s, a, 0, x), (s, b, sz - 1, y)]
    if kind == "overlapped chunk":  # [sz - 16, sz) where sz % 16 != 0: its first byte is also the chunk before's
        return [(s, a, max(0, sz - 16), x), (s, b, sz - 1 - (n % min(sz, 3)), y)]
    assert kind == "whole blocks"
    rng = np.random.default_rng(1000 + n)
    va, vb = rng.integers(1, 256, size=(2, sz))
    return [(s, a, p, int(va[p])) for p in range(sz)] + [(s, b, p, int(vb[p])) for p in range(sz)]


def mixed_corrupt(sizes, nb, seed=0, every=9, whole_up_to=1100):
    """Of the nonempty stripes, in order: one in `every` stays clean, one in
    `every` gets a single flipped byte, the others two corrupt slots, the pair
    cycling through all nb (nb - 1) / 2 pairs (from pair `seed` on) and the
    placement through PLACEMENTS; whole blocks are overwritten only in stripes
    of at most whole_up_to bytes (the next placement elsewhere), and a 70001-byte
    stripe is always a pair stripe and takes "first and last".  Returns (corrupt, pairs: stripe -> ((a, b),
    placement), singles: stripe -> slot)."""
    allp = list(itertools.combinations(range(nb), 2))
    cor, pairs, singles = [], {}, {}
    n = q = 0
    for s, sz in enumerate(sizes):
        if not sz:
            continue
        n += 1
        if n % every == 1 and sz != 70001:
            continue
        if n % every == 2 and sz != 70001:
            singles[s] = (n // every + seed) % nb
            pos = sc.positions(sz)
            cor.append((s, singles[s], pos[n % len(pos)], 1 + (53 * n) % 255))
            continue
        a, b = allp[(q + seed) % len(allp)]
        kind = PLACEMENTS[q % len(PLACEMENTS)]
        if kind == "whole blocks" and sz > whole_up_to:
            kind = PLACEMENTS[(q + 1) % len(PLACEMENTS)]
        if sz == 70001:
            kind = "first and last"
        if q % 2:  # either order of the two slots in the stripe's bytes
            a, b = b, a
        cor += place_pair(s, a, b, sz, kind, q)
        pairs[s] = ((min(a, b), max(a, b)), kind)
        q += 1
    return cor, pairs, singles


# ---- one call on the GPU ---------------------------------------------------------------------------------

def words(vals, desc):
    """nstripes 8-byte words in host (numpy) or device (torch) memory: (keep-alive, address)."""
    import torch

    a = np.array([int(v) % 2**64 for v in vals], dtype=np.uint64)
    if desc == "host":
        return a, a.ctypes.data
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t, t.data_ptr()


def call(case, heal, desc="host", res="dev", soff=None, sizes=None, tail=sc.TAIL, pinned=False):
    """One fec_locate2_batch_ragged (heal: fec_correct2_batch_ragged) over a
    fresh copy of the case's arena, which ends `tail` bytes past the extent the
    call declares, with the 2 * ns verdict words between guard words in device
    ("dev"), page-locked ("pinned") or plain host ("host") memory.  Returns
    (planes (2, ns), the last kernel's name, the arena afterwards, the tensor
    that holds it)."""
    import torch
    from zfec_amd import capi

    ns = case.ns
    host = np.concatenate([case.src[:sc.IN_OFF + case.src_bytes], np.full(tail, sc.BACKGROUND, dtype=np.uint8)])
    arena = torch.from_numpy(host.copy()).pin_memory() if pinned else torch.from_numpy(host).cuda()
    fill = np.full(LEAD_W + 2 * ns + TAIL_W, GUARD_WORD, dtype=np.uint32)
    if res == "dev":
        out = torch.from_numpy(fill.view(np.int32)).cuda()
        ptr = out.data_ptr() + 4 * LEAD_W
    elif res == "pinned":
        out = torch.from_numpy(fill.view(np.int32)).pin_memory()
        ptr = out.data_ptr() + 4 * LEAD_W
    else:
        out = fill
        ptr = out.ctypes.data + 4 * LEAD_W
    keep = [words(case.sizes if sizes is None else sizes, desc), words(case.soff if soff is None else soff, desc)]
    code = capi.Code(case.k, case.m)
    fn = code.correct2_batch_ragged if heal else code.locate2_batch_ragged
    fn(arena.data_ptr() + sc.IN_OFF, case.src_bytes, case.sbs, keep[1][1], keep[0][1], case.nums, ns, ptr,
       stream=torch.cuda.current_stream().cuda_stream)
    name = capi.last_kernel_name()
    torch.cuda.synchronize()
    if res == "dev":
        out = out.cpu().numpy().view(np.uint32)
    elif res == "pinned":
        out = out.numpy().view(np.uint32)
    assert (out[:LEAD_W] == GUARD_WORD).all() and (out[LEAD_W + 2 * ns:] == GUARD_WORD).all(), "guard words written"
    return out[LEAD_W:LEAD_W + 2 * ns].reshape(2, ns).copy(), name, arena.cpu().numpy(), arena


def judge(model, planes, after, what, heal, tail=sc.TAIL):
    """Both planes against the model, and the whole arena afterwards against
    the expected one (a location must leave it as on entry)."""
    bad = np.argwhere(planes != model.planes)
    assert not bad.size, (what, "wrong verdict words (plane, stripe, got, want)",
                          [(int(p), int(s), hex(planes[p, s]), hex(model.planes[p, s])) for p, s in bad[:8]])
    want = model.expected_arena(tail, heal)
    diff = np.flatnonzero(after != want)
    assert not diff.size, (what, "arena differs at", diff[:8].tolist(), "stripe offsets", model.case.soff[:8])


def no_bit_left(model, arena):
    """fec_verify_batch_ragged over the arena after a correction (still on the
    device) sets no bit for any stripe with a slot or pair verdict."""
    import torch
    from zfec_amd import capi

    case = model.case
    out = torch.full((case.ns, case.words), -1, dtype=torch.int32, device="cuda")
    keep = [words(case.sizes, "host"), words(case.soff, "host")]
    capi.Code(case.k, case.m).verify_batch_ragged(arena.data_ptr() + sc.IN_OFF, case.src_bytes, case.sbs, keep[1][1],
                                                  keep[0][1], case.nums, case.ns, out.data_ptr(),
                                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bits = out.cpu().numpy()
    healed = model.healed()
    assert healed and not bits[healed].any(), "a healed stripe is still inconsistent"


# ---- the main case: K=3/M=10, 7 slots (21 pairs), the edge sizes twice over ----------------------------

PERM = [int(x) for x in np.random.default_rng(11).permutation(len(rc.EDGE_SIZES))]
ORDERS = {"listed": rc.EDGE_SIZES, "reversed": rc.EDGE_SIZES[::-1], "permuted": [rc.EDGE_SIZES[i] for i in PERM]}
_main = {}


def main_case(order, layout="packed"):
    """(case, clean case, model, pairs, singles): the order's sizes twice in a
    row, so that all 21 pairs fit into one call beside clean, single-slot and
    zero-size stripes.  Computed once and shared, unchanged, by the tests."""
    key = (order, layout)
    if key not in _main:
        sizes = list(ORDERS[order]) * 2
        i = sorted(ORDERS).index(order)
        cor, pairs, singles = mixed_corrupt(sizes, len(sc.NUMS), seed=5 * i)
        place = [int(x) for x in np.random.default_rng(20 + i).permutation(len(sizes))]
        case = sc.ScrubCase(3, 10, sc.NUMS, sizes, cor, layout=layout, place=place, seed=60 + i)
        clean = sc.ScrubCase(3, 10, sc.NUMS, sizes, (), layout=layout, place=place, seed=60 + i)
        _main[key] = (case, clean, Model(case), pairs, singles)
    return _main[key]
