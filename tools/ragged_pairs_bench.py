#!/usr/bin/env python3
"""The ragged pair location and correction (fec_locate2_batch_ragged /
fec_correct2_batch_ragged) against existing calls on the same buffers in the
same process: K=3/M=10 with 7 blocks held (c = 4, 21 pairs), device-resident,
--rounds alternating rounds of single launches between two events (a
correction heals what it finds, so the corruption is applied again, untimed,
before every launch of a dirty state), medians and the range of single-round
ratios.  Every launch touches many times the 256 MiB Infinity Cache.

1  mixed sizes, clean: --nstripes stripes of fixed-seed block sizes uniform in
   [1, 4096], packed objects, descriptors in device memory
     loc   fec_locate_batch_ragged      loc2  fec_locate2_batch_ragged
     cor   fec_correct_batch_ragged     cor2  fec_correct2_batch_ragged
   (the uniform pair, tools/locate2_bench.py, shows locate2 / locate = 1.00)

2  mixed sizes, 1 % of the stripes with two whole blocks overwritten; for the
   location and for the correction
     a  the ragged call on the packed objects
     b  the same stripes padded to 4096: one fec_locate2_batch /
        fec_correct2_batch over the padded rows
     c  calls by distinct size: one uniform call per distinct size over objects
        already gathered by size (the gather itself is not charged)

3  equal sizes: --nstripes stripes of 4096-byte blocks, clean and 1 % dirty
     u   fec_locate2_batch / fec_correct2_batch (the yardstick)
     u2  the same call again (the A/A spread of the yardstick in this run)
     rd  the ragged call, descriptors in device memory
     rh  the ragged call, descriptors in host memory (staged per call)

Before anything is timed the verdicts are the known corruption, and after every
healing launch of the first round the overwritten blocks are what they were.
Writes profiles/ragged_pairs_bench.json.

    python tools/ragged_pairs_bench.py [--nstripes 1000000] [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import zfec_amd  # noqa: E402
from zfec_amd import capi  # noqa: E402
from ragged_bench import dev_words, summary  # noqa: E402

K, M, SZ = 3, 10, 4096
NB = 7
NUMS = list(range(NB))
CLEAN, NONE = zfec_amd.LOCATE_CLEAN, zfec_amd.LOCATE_NONE


def packed_arena(code, st, sizes):
    """Consistent packed objects of the given block sizes: (arena, offsets)."""
    ns = len(sizes)
    start = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    g = torch.Generator(device="cuda").manual_seed(6)
    data = torch.randint(0, 256, (K * total,), dtype=torch.uint8, device="cuda", generator=g)
    arena = torch.empty(NB * total, dtype=torch.uint8, device="cuda")
    dsz, din, dout = dev_words(sizes), dev_words(K * start), dev_words(NB * start)
    code.encode_batch_ragged(data.data_ptr(), data.numel(), 0, din.data_ptr(), arena.data_ptr(), arena.numel(), 0,
                             dout.data_ptr(), dsz.data_ptr(), NUMS, ns, stream=st.cuda_stream)
    torch.cuda.synchronize()
    return arena, NB * start


def equal_arena(code, st, ns):
    g = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randint(0, 256, (ns, K, SZ), dtype=torch.uint8, device="cuda", generator=g)
    blocks = torch.empty((ns, NB, SZ), dtype=torch.uint8, device="cuda")
    code.encode_batch(data.data_ptr(), SZ, K * SZ, blocks.data_ptr(), SZ, NB * SZ, NUMS, SZ, ns, stream=st.cuda_stream)
    torch.cuda.synchronize()
    return blocks


class Spoiler(object):
    """Two whole blocks of `frac` of the stripes of a flat arena overwritten (xor
    with bytes in 1..255, so every byte changes), again and again with the same
    bytes.  sizes, offs: per stripe, numpy; stripe s's slot j is at offs[s] + j * sizes[s]."""

    def __init__(self, arena, sizes, offs, frac, seed):
        ns = len(sizes)
        n = max(1, int(ns * frac))
        rng = np.random.default_rng(seed)
        self.rows = np.sort(rng.permutation(ns)[:n])
        a = rng.integers(0, NB, size=n)
        b = (a + rng.integers(1, NB, size=n)) % NB
        self.slots = np.stack([np.minimum(a, b), np.maximum(a, b)])  # (2, n), a < b
        sz = np.asarray(sizes, dtype=np.int64)[self.rows]
        starts = np.concatenate([np.asarray(offs, dtype=np.int64)[self.rows] + self.slots[t] * sz for t in range(2)])
        lens = torch.as_tensor(np.concatenate([sz, sz])).cuda()
        first = torch.cumsum(lens, 0) - lens
        total = int(lens.sum())
        self.idx = torch.repeat_interleave(torch.as_tensor(starts).cuda() - first, lens) + \
            torch.arange(total, device="cuda")
        self.arena = arena
        self.orig = arena[self.idx]
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.noise = torch.randint(1, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
        self.n = n

    def want(self, ns):
        """The [2, ns] verdicts of the arena as spoil() leaves it."""
        w = torch.empty((2, ns), dtype=torch.int32)
        w[0] = CLEAN
        w[1] = NONE
        w[:, torch.as_tensor(self.rows)] = torch.as_tensor(self.slots, dtype=torch.int32)
        return w.cuda()

    def spoil(self):
        self.arena[self.idx] = self.orig ^ self.noise

    def healed(self):
        return torch.equal(self.arena[self.idx], self.orig)


def timed_singles(arms, nrounds, before, after_first=None):
    """arms: name -> launch function(stream handle).  One launch per arm and
    round between two events, `before()` run untimed ahead of it; the first
    round is a warm-up, after each launch of which after_first(name) runs."""
    st = torch.cuda.current_stream()
    rounds = {a: [] for a in arms}
    for rnd in range(nrounds + 1):
        for a, fn in arms.items():
            before(a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            fn(st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            if rnd:
                rounds[a].append(e0.elapsed_time(e1))
            elif after_first:
                after_first(a)
    return rounds


def ragged(code, heal, arena, off_ptr, size_ptr, ns, res, pairs=True):
    name = ("correct" if heal else "locate") + ("2" if pairs else "") + "_batch_ragged"
    fn = getattr(code, name)
    return lambda sh: fn(arena.data_ptr(), arena.numel(), 0, off_ptr, size_ptr, NUMS, ns, res.data_ptr(), stream=sh)


def uniform(code, heal, blocks, sz, ns, res):
    fn = code.correct2_batch if heal else code.locate2_batch
    return lambda sh: fn(blocks.data_ptr(), sz, NB * sz, NUMS, sz, ns, res.data_ptr(), stream=sh)


def pair_count(res):
    return int((res.view(2, -1)[1] != NONE).sum())


# ---- 1: mixed sizes, clean -----------------------------------------------------------------------------------

def mixed_clean(args, code, arena, dsz, doff, ns):
    r1 = torch.empty(ns, dtype=torch.int32, device="cuda")
    r2 = torch.empty(2 * ns, dtype=torch.int32, device="cuda")
    arms = {"loc": ragged(code, False, arena, doff.data_ptr(), dsz.data_ptr(), ns, r1, pairs=False),
            "loc2": ragged(code, False, arena, doff.data_ptr(), dsz.data_ptr(), ns, r2),
            "cor": ragged(code, True, arena, doff.data_ptr(), dsz.data_ptr(), ns, r1, pairs=False),
            "cor2": ragged(code, True, arena, doff.data_ptr(), dsz.data_ptr(), ns, r2)}
    kernels = {}
    for a, fn in arms.items():
        (r1 if a in ("loc", "cor") else r2).fill_(0x55)
        fn(torch.cuda.current_stream().cuda_stream)
        kernels[a] = capi.last_kernel_name()
        torch.cuda.synchronize()
    assert bool((r1 == CLEAN).all()) and bool((r2[:ns] == CLEAN).all()) and bool((r2[ns:] == NONE).all()), \
        "a consistent arena was judged dirty"
    rounds = timed_singles(arms, args.rounds, lambda a: None)
    out = summary(rounds, "loc")
    out["kernels"] = kernels
    q = [x / y for x, y in zip(rounds["cor2"], rounds["cor"])]
    out["cor2_over_cor"] = {"median": round(float(np.median(q)), 4), "min": round(min(q), 4), "max": round(max(q), 4)}
    return out


# ---- 2: mixed sizes, 1 % dirty ---------------------------------------------------------------------------------

def mixed_dirty(args, st, code, sizes, arena, offs, dsz, doff, padded):
    ns = len(sizes)
    order = np.sort(sizes)
    sorted_arena, soffs = packed_arena(code, st, order)
    vals, counts = np.unique(order, return_counts=True)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    buckets = [(int(v), int(n), int(soffs[i]), int(i)) for v, n, i in zip(vals, counts, first)]
    ra, rb, rc_ = (torch.empty(2 * ns, dtype=torch.int32, device="cuda") for _ in range(3))
    sp = {"a": Spoiler(arena, sizes, offs, 0.01, 21),
          "b": Spoiler(padded.view(-1), np.full(ns, SZ, dtype=np.int64), np.arange(ns, dtype=np.int64) * (NB * SZ),
                       0.01, 21),
          "c": Spoiler(sorted_arena, order, soffs, 0.01, 21)}
    res = {}
    for heal in (False, True):
        def c(sh, heal=heal):
            fn = code.correct2_batch if heal else code.locate2_batch
            for v, n, o, i in buckets:
                fn(sorted_arena.data_ptr() + o, v, NB * v, NUMS, v, n, rc_.data_ptr() + 8 * i, stream=sh)

        arms = {"a": ragged(code, heal, arena, doff.data_ptr(), dsz.data_ptr(), ns, ra),
                "b": uniform(code, heal, padded, SZ, ns, rb),
                "c": c}
        # the verdicts are the known corruption (c: as many pairs, its words lie per call)
        for a, r in (("a", ra), ("b", rb), ("c", rc_)):
            sp[a].spoil()
            r.fill_(0x55)
            arms[a](st.cuda_stream)
            torch.cuda.synchronize()
            if a != "c":
                assert torch.equal(r.view(2, ns), sp[a].want(ns)), "%s: the verdicts are not the known corruption" % a
            if heal:
                assert sp[a].healed(), "%s did not restore the overwritten blocks" % a
        rc_.fill_(0x55)
        sp["c"].spoil()
        c(st.cuda_stream)
        torch.cuda.synchronize()
        got = sum(int((rc_[2 * i + n:2 * i + 2 * n] != NONE).sum()) for v, n, o, i in buckets)
        assert got == sp["c"].n, "c: %d pairs named, %d stripes overwritten" % (got, sp["c"].n)

        def check(a, heal=heal):
            assert not heal or sp[a].healed(), "%s did not restore the overwritten blocks" % a

        rounds = timed_singles(arms, args.rounds, lambda a: sp[a].spoil(), check)
        res["correct2" if heal else "locate2"] = summary(rounds, "a")
        torch.cuda.synchronize()
    for s in sp.values():  # leave the arenas clean
        s.arena[s.idx] = s.orig
    res["shape"] = {"stripes": ns, "distinct_sizes": len(buckets), "overwritten_stripes": sp["a"].n,
                    "block_bytes": NB * int(sizes.sum()), "padded_block_bytes": NB * ns * SZ}
    return res


# ---- 3: equal sizes ---------------------------------------------------------------------------------------------

def equal_sizes(args, st, code, blocks):
    ns = blocks.shape[0]
    arena = blocks.view(-1)
    sizes = np.full(ns, SZ, dtype=np.int64)
    offs = np.arange(ns, dtype=np.int64) * (NB * SZ)
    dsz, doff = dev_words(sizes), dev_words(offs)
    ru, rr = (torch.empty(2 * ns, dtype=torch.int32, device="cuda") for _ in range(2))
    sp = Spoiler(arena, sizes, offs, 0.01, 22)
    res = {"bytes_scrubbed_per_launch": ns * NB * SZ}
    for state, dirty in (("clean", False), ("one_percent", True)):
        for heal in (False, True):
            arms = {"u": uniform(code, heal, blocks, SZ, ns, ru),
                    "rd": ragged(code, heal, arena, doff.data_ptr(), dsz.data_ptr(), ns, rr),
                    "rh": ragged(code, heal, arena, offs.ctypes.data, sizes.ctypes.data, ns, rr),
                    "u2": uniform(code, heal, blocks, SZ, ns, ru)}
            want = sp.want(ns) if dirty else None
            for a in ("u", "rd", "rh"):
                if dirty:
                    sp.spoil()
                r = ru if a == "u" else rr
                r.fill_(0x55)
                arms[a](st.cuda_stream)
                torch.cuda.synchronize()
                if dirty:
                    assert torch.equal(r.view(2, ns), want), "%s: the verdicts are not the known corruption" % a
                    assert not heal or sp.healed(), "%s did not restore the overwritten blocks" % a
                else:
                    assert pair_count(r) == 0 and bool((r[:ns] == CLEAN).all()), "a consistent arena was judged dirty"
            rounds = timed_singles(arms, args.rounds, (lambda a: sp.spoil()) if dirty else (lambda a: None))
            res.setdefault(state, {})["correct2" if heal else "locate2"] = summary(rounds, "u")
            torch.cuda.synchronize()
        if dirty:
            arena[sp.idx] = sp.orig
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_pairs_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_pairs_bench.py measures on a GPU"
    code = capi.Code(K, M)
    st = torch.cuda.current_stream()
    ns = args.nstripes
    out = {"workload": "K=3/M=10, 7 blocks held (c = 4), device-resident; medians of %d alternating rounds of single "
                       "launches between two events, one warm-up round; in the dirty states two whole blocks of 1 %% "
                       "of the stripes are overwritten again, untimed, before every launch" % args.rounds,
           "device": torch.cuda.get_device_name(0)}
    sizes = np.random.default_rng(7).integers(1, SZ + 1, size=ns, dtype=np.int64)
    arena, offs = packed_arena(code, st, sizes)
    dsz, doff = dev_words(sizes), dev_words(offs)
    out["mixed_uniform_1_4096"] = {"clean": mixed_clean(args, code, arena, dsz, doff, ns)}
    print("mixed clean done", file=sys.stderr, flush=True)
    padded = equal_arena(code, st, ns)
    out["mixed_uniform_1_4096"]["one_percent"] = mixed_dirty(args, st, code, sizes, arena, offs, dsz, doff, padded)
    print("mixed dirty done", file=sys.stderr, flush=True)
    del arena
    torch.cuda.empty_cache()
    out["equal_sizes_4096"] = equal_sizes(args, st, code, padded)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
