#!/usr/bin/env python3
"""The ragged repair and the ragged in-place correction
(fec_repair_batch_ragged / fec_correct_batch_ragged) against the uniform calls:
K=3/M=10, device-resident, all arms in one process, --rounds alternating
rounds, medians and the range of single-round ratios.

Repair arms are timed like tools/ragged_bench.py (launches back to back
between two events behind a spin kernel).  A correction heals what it finds,
so its arms are timed one launch at a time between two events, the corruption
applied again (untimed) before every launch; every launch touches many times
the 256 MiB Infinity Cache.

1  equal sizes: --nstripes stripes of 4096-byte blocks on the same buffers
   repair: one lost block per stripe, all 120 present-patterns at random
     u   fec_repair_batch (the yardstick), ids in device memory
     u2  the same call again (the A/A spread of the yardstick in this run)
     rd  the ragged call, descriptors and ids in device memory (ragged_scan runs)
     rh  the ragged call, descriptors and ids in host memory (staged per call)
   correct: all 10 blocks held (7 checks); clean data, 1 % of the stripes with
   one corrupt byte, every stripe with one
     u / u2 / rd / rh as above, fec_correct_batch against the ragged call
   --caps runs rd again under those ZFEC_HIP_GRID_CAP values: fewer workgroups
   give each wave a longer range of units (--sweep: the caps that give 6, 12,
   24 and 48 units per wave).

2  mixed sizes: --nstripes stripes of fixed-seed sizes uniform in [1, 4096],
   for the repair and for the correction of clean data
     a  the ragged call (device arrays) on the packed objects
     b  pad every object to 4096: one uniform call over the padded rows
     c  bucket by size: one uniform call per distinct size over objects already
        gathered by size (the gather itself is not charged)

The ragged results are compared with the uniform call's before anything is
timed.  Writes profiles/ragged_repair_bench.json.

    python tools/ragged_repair_bench.py [--nstripes 1000000] [--rounds 9] [--launches 5] [--sweep] [--out FILE]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from zfec_amd import capi  # noqa: E402
from ragged_bench import dev_words, run_rounds, set_cap, summary, with_caps  # noqa: E402

K, M, SZ = 3, 10, 4096
NB = M
NUMS = list(range(M))
PRESENT = [list(p) for p in itertools.combinations(range(M), K)]          # all 120
TARGETS = [[min(b for b in range(M) if b not in p)] for p in PRESENT]     # one lost block each


def dev_ids(ids):
    return torch.as_tensor(np.asarray(ids, dtype=np.int32)).cuda()


# ---- repair -------------------------------------------------------------------------------------------

def repair_uniform(code, src, dst, sz, ns, ids_ptr):
    return lambda sh: code.repair_batch(src, sz, K * sz, dst, sz, sz, PRESENT, TARGETS, ids_ptr, sz, ns, stream=sh)


def repair_ragged(code, src, dst, p, ids_ptr, ns):
    return lambda sh: code.repair_batch_ragged(src.data_ptr(), src.numel(), 0, p["in"], dst.data_ptr(), dst.numel(), 0,
                                               p["out"], p["sizes"], PRESENT, TARGETS, ids_ptr, ns, stream=sh)


def repair_equal(args, st, code):
    ns = args.nstripes
    g = torch.Generator(device="cuda").manual_seed(5)
    recv = torch.randint(0, 256, (ns * K * SZ,), dtype=torch.uint8, device="cuda", generator=g)
    want = torch.empty(ns * SZ, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(want)
    ids = np.random.default_rng(7).integers(0, len(PRESENT), size=ns).astype(np.uint32)
    dids = dev_ids(ids.view(np.int32))
    sizes = np.full(ns, SZ, dtype=np.int64)
    start = np.arange(ns, dtype=np.int64) * SZ
    h = {"sizes": sizes, "in": K * start, "out": start}
    d = {k: dev_words(v) for k, v in h.items()}
    hp = {k: v.ctypes.data for k, v in h.items()}
    dp = {k: v.data_ptr() for k, v in d.items()}
    u = repair_uniform(code, recv.data_ptr(), want.data_ptr(), SZ, ns, dids.data_ptr())
    u(st.cuda_stream)
    for p, ip in ((dp, dids.data_ptr()), (hp, ids.ctypes.data)):
        out.fill_(0xA5)
        repair_ragged(code, recv, out, p, ip, ns)(st.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(out, want), "ragged repair differs from fec_repair_batch"
    kern = capi.last_kernel_name()
    arms = with_caps({"u": repair_uniform(code, recv.data_ptr(), out.data_ptr(), SZ, ns, dids.data_ptr()),
                      "rd": repair_ragged(code, recv, out, dp, dids.data_ptr(), ns),
                      "rh": repair_ragged(code, recv, out, hp, ids.ctypes.data, ns),
                      "u2": repair_uniform(code, recv.data_ptr(), out.data_ptr(), SZ, ns, dids.data_ptr())},
                     ("rd",), args.caps)
    rounds, host = run_rounds(arms, args.rounds, args.launches, st, "equal repair")
    return dict(summary(rounds, "u"), host_call_us=host, kernel=kern, bytes_per_launch=ns * (K + 1) * SZ)


def repair_mixed(args, st, code, sizes):
    ns = len(sizes)
    ids = np.random.default_rng(8).integers(0, len(PRESENT), size=ns).astype(np.uint32)
    g = torch.Generator(device="cuda").manual_seed(6)
    total = int(sizes.sum())
    start = np.cumsum(sizes) - sizes
    # a: packed objects
    src = torch.randint(0, 256, (K * total,), dtype=torch.uint8, device="cuda", generator=g)
    out_a = torch.empty(total, dtype=torch.uint8, device="cuda")
    pa = {k: dev_words(v) for k, v in {"sizes": sizes, "in": K * start, "out": start}.items()}
    dids = dev_ids(ids.view(np.int32))
    a = repair_ragged(code, src, out_a, {k: v.data_ptr() for k, v in pa.items()}, dids.data_ptr(), ns)
    # b: every object padded to SZ
    padded = torch.randint(0, 256, (ns * K * SZ,), dtype=torch.uint8, device="cuda", generator=g)
    out_b = torch.empty(ns * SZ, dtype=torch.uint8, device="cuda")
    b = repair_uniform(code, padded.data_ptr(), out_b.data_ptr(), SZ, ns, dids.data_ptr())
    # c: the objects gathered by size (the same bytes, sorted; the gather is not charged)
    order = np.argsort(sizes, kind="stable")
    ssz = sizes[order]
    sstart = np.cumsum(ssz) - ssz
    sids = dev_ids(ids[order].view(np.int32))
    out_c = torch.empty(total, dtype=torch.uint8, device="cuda")
    vals, counts = np.unique(ssz, return_counts=True)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    buckets = [(int(v), int(n), int(sstart[i]), int(i)) for v, n, i in zip(vals, counts, first)]

    def c(sh):
        for v, n, o, i in buckets:
            code.repair_batch(src.data_ptr() + K * o, v, K * v, out_c.data_ptr() + o, v, v, PRESENT, TARGETS,
                              sids.data_ptr() + 4 * i, v, n, stream=sh)

    for f in (a, b, c):
        f(st.cuda_stream)
    torch.cuda.synchronize()
    rounds, host = run_rounds(with_caps({"a": a, "b": b, "c": c}, ("a",), args.caps), args.rounds, args.launches, st,
                              "mixed repair")
    return dict(summary(rounds, "a"), host_call_us=host,
                shape={"stripes": ns, "distinct_sizes": len(buckets), "block_bytes": (K + 1) * total,
                       "padded_block_bytes": (K + 1) * ns * SZ})


# ---- correction -------------------------------------------------------------------------------------------

def corrupt(blocks, frac, seed):
    """XOR one byte of one slot in `frac` of the stripes; a healing call, or calling it again, undoes it."""
    if not frac:
        return
    ns = blocks.shape[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.arange(ns, device="cuda") if frac >= 1 else \
        torch.randperm(ns, device="cuda", generator=g)[:max(1, int(ns * frac))]
    slot = torch.randint(0, NB, (idx.numel(),), device="cuda", generator=g)
    pos = torch.randint(0, SZ, (idx.numel(),), device="cuda", generator=g)
    blocks[idx, slot, pos] ^= 0x5A


def timed_singles(arms, nrounds, before, tag):
    """arms: name -> (launch function(stream handle), grid cap).  One launch per
    arm and round between two events, `before()` run untimed ahead of it."""
    st = torch.cuda.current_stream()
    rounds = {a: [] for a in arms}
    for rnd in range(nrounds + 1):  # the first round is a warm-up
        for a, (fn, cap) in arms.items():
            before()
            set_cap(cap)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            fn(st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            set_cap(None)
            if rnd:
                rounds[a].append(e0.elapsed_time(e1))
    return rounds


def correct_uniform(code, blocks, sz, ns, res):
    return lambda sh: code.correct_batch(blocks.data_ptr(), sz, NB * sz, NUMS, sz, ns, res.data_ptr(), stream=sh)


def correct_ragged(code, arena, off_ptr, size_ptr, ns, res):
    return lambda sh: code.correct_batch_ragged(arena.data_ptr(), arena.numel(), 0, off_ptr, size_ptr, NUMS, ns,
                                                res.data_ptr(), stream=sh)


def correct_equal(args, st, code):
    ns = args.nstripes
    g = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randint(0, 256, (ns, K, SZ), dtype=torch.uint8, device="cuda", generator=g)
    blocks = torch.empty((ns, NB, SZ), dtype=torch.uint8, device="cuda")
    code.encode_batch(data.data_ptr(), SZ, K * SZ, blocks.data_ptr(), SZ, NB * SZ, NUMS, SZ, ns, stream=st.cuda_stream)
    torch.cuda.synchronize()
    del data
    arena = blocks.view(-1)
    sizes = np.full(ns, SZ, dtype=np.int64)
    offs = np.arange(ns, dtype=np.int64) * (NB * SZ)
    dsz, doff = dev_words(sizes), dev_words(offs)
    ru, rr = torch.empty(ns, dtype=torch.int32, device="cuda"), torch.empty(ns, dtype=torch.int32, device="cuda")
    # the ragged call against the uniform one on the same corruption: verdicts, and the arena healed
    probe = blocks[:: max(1, ns // 4096)].clone()
    for po, ps in ((doff.data_ptr(), dsz.data_ptr()), (offs.ctypes.data, sizes.ctypes.data)):
        corrupt(blocks, 0.01, 8)
        correct_uniform(code, blocks, SZ, ns, ru)(st.cuda_stream)
        corrupt(blocks, 0.01, 8)
        rr.fill_(0x55)
        correct_ragged(code, arena, po, ps, ns, rr)(st.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(ru, rr), "ragged correction's verdicts differ from fec_correct_batch's"
        assert int((ru >= 0).sum()) == max(1, int(ns * 0.01)), "unexpected number of corrected stripes"
        assert torch.equal(blocks[:: max(1, ns // 4096)], probe), "the ragged correction did not heal the arena"
    kern = capi.last_kernel_name()
    res = {"kernel": kern, "bytes_scrubbed_per_launch": ns * NB * SZ}
    for name, frac in (("clean", 0.0), ("one_percent", 0.01), ("every_stripe", 1.0)):
        arms = with_caps({"u": correct_uniform(code, blocks, SZ, ns, ru),
                          "rd": correct_ragged(code, arena, doff.data_ptr(), dsz.data_ptr(), ns, rr),
                          "rh": correct_ragged(code, arena, offs.ctypes.data, sizes.ctypes.data, ns, rr),
                          "u2": correct_uniform(code, blocks, SZ, ns, ru)}, ("rd",), args.caps)
        rounds = timed_singles(arms, args.rounds, lambda: corrupt(blocks, frac, 9), "equal correct " + name)
        res[name] = summary(rounds, "u")
        torch.cuda.synchronize()
        assert torch.equal(blocks[:: max(1, ns // 4096)], probe), "a timed correction left the arena corrupt"
    return res, blocks


def correct_mixed(args, st, code, sizes, padded):
    from ragged_scrub_bench import packed_arena

    ns = len(sizes)
    arena, offs = packed_arena(code, st, sizes)
    dsz, doff = dev_words(sizes), dev_words(offs)
    order = np.sort(sizes)
    sorted_arena, soffs = packed_arena(code, st, order)
    vals, counts = np.unique(order, return_counts=True)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    buckets = [(int(v), int(n), int(soffs[i]), int(i)) for v, n, i in zip(vals, counts, first)]
    ra, rb, rc_ = (torch.empty(ns, dtype=torch.int32, device="cuda") for _ in range(3))
    a = correct_ragged(code, arena, doff.data_ptr(), dsz.data_ptr(), ns, ra)
    b = correct_uniform(code, padded, SZ, ns, rb)

    def c(sh):
        for v, n, o, i in buckets:
            code.correct_batch(sorted_arena.data_ptr() + o, v, NB * v, NUMS, v, n, rc_.data_ptr() + 4 * i, stream=sh)

    for f, r in ((a, ra), (b, rb), (c, rc_)):
        r.fill_(0x55)
        f(st.cuda_stream)
        torch.cuda.synchronize()
        assert bool((r == -1).all()), "a consistent arena was judged dirty"
    rounds, host = run_rounds(with_caps({"a": a, "b": b, "c": c}, ("a",), args.caps), args.rounds, args.launches, st,
                              "mixed correct")
    return dict(summary(rounds, "a"), host_call_us=host,
                shape={"stripes": ns, "distinct_sizes": len(buckets), "block_bytes": NB * int(sizes.sum()),
                       "padded_block_bytes": NB * ns * SZ})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--caps", type=lambda v: [int(x) for x in v.split(",") if x], default=[],
                    help="also run the ragged device-array arms under these ZFEC_HIP_GRID_CAP values")
    ap.add_argument("--sweep", action="store_true",
                    help="--caps that give the equal-size arms 6, 12, 24 and 48 units per wave")
    ap.add_argument("--skip-mixed", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_repair_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_repair_bench.py measures on a GPU"
    if args.sweep:  # 4 units per stripe, 4 waves per workgroup
        units = args.nstripes * (SZ // 1024)
        args.caps = sorted({-(-units // (4 * upw)) for upw in (6, 12, 24, 48)} | set(args.caps), reverse=True)
    code = capi.Code(K, M)
    st = torch.cuda.current_stream()
    out = {"workload": "K=3/M=10, device-resident; repair: one lost block per stripe, all 120 present-patterns at "
                       "random, medians of %d alternating rounds of %d launches back to back; correction: all 10 "
                       "blocks held (7 checks), medians of %d alternating rounds of single launches, the corruption "
                       "applied again before each" % (args.rounds, args.launches, args.rounds),
           "device": torch.cuda.get_device_name(0), "grid_caps": args.caps,
           "units_per_wave_of_caps": {str(c): round(args.nstripes * (SZ // 1024) / (4.0 * c), 2) for c in args.caps}}
    out["equal_sizes_4096"] = {"repair": repair_equal(args, st, code)}
    torch.cuda.empty_cache()
    out["equal_sizes_4096"]["correct"], padded = correct_equal(args, st, code)
    if not args.skip_mixed:
        sizes = np.random.default_rng(7).integers(1, 4097, size=args.nstripes, dtype=np.int64)
        caps, args.caps = args.caps, []
        out["mixed_uniform_1_4096"] = {"correct_clean": correct_mixed(args, st, code, sizes, padded)}
        del padded
        torch.cuda.empty_cache()
        out["mixed_uniform_1_4096"]["repair"] = repair_mixed(args, st, code, sizes)
        args.caps = caps
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
