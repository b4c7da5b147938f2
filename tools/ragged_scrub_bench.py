#!/usr/bin/env python3
"""The ragged scrub (fec_verify_batch_ragged / fec_locate_batch_ragged) against
the uniform calls: K=3/M=10 with all 10 blocks held (7 checks), device-resident,
timed like tools/ragged_bench.py (launches back to back between two events
behind a spin kernel, every launch touching many times the 256 MiB Infinity
Cache), all arms in one process, --rounds alternating rounds, medians and the
range of single-round ratios.

1  equal sizes: --nstripes stripes of 4096-byte blocks on the same buffer, for
   verify and for locate
     u   fec_verify_batch / fec_locate_batch (the yardstick)
     u2  the same call again (the A/A spread of the yardstick in this run)
     rd  the ragged call, descriptor arrays in device memory (ragged_scan runs)
     rh  the ragged call, descriptor arrays in host memory (staged per call)
   --caps runs rd again under those ZFEC_HIP_GRID_CAP values: fewer workgroups
   give each wave a longer range of units (the units-per-wave rule was measured
   for the encode only).

2  mixed sizes: --nstripes stripes of fixed-seed sizes uniform in [1, 4096],
   for verify and for locate
     a  the ragged call (device arrays) on the packed objects
     b  pad every object to 4096: one uniform call over the padded rows
     c  bucket by size: one uniform call per distinct size over objects already
        gathered by size (the gather itself is not charged)

3  locate against verify, ragged calls, equal sizes: clean data, 1 % of the
   stripes with one corrupt byte, every stripe with one.

Every buffer holds consistent stripes (the library's own encode), so the clean
arms take the clean path; the ragged results are compared with the uniform
call's before anything is timed.  Writes profiles/ragged_scrub_bench.json.

    python tools/ragged_scrub_bench.py [--nstripes 1000000] [--rounds 9] [--launches 5] [--caps 256,2048] [--out FILE]
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

from zfec_amd import capi  # noqa: E402
from ragged_bench import dev_words, run_rounds, summary, with_caps  # noqa: E402

K, M, SZ = 3, 10, 4096
NB, C = M, M - K
NUMS = list(range(M))
OPS = ("verify", "locate")


def result_words(ns):
    return torch.empty(ns, dtype=torch.int32, device="cuda")


def uniform(code, op, ptr, sz, ns, res):
    fn = code.verify_batch if op == "verify" else code.locate_batch
    return lambda sh: fn(ptr, sz, NB * sz, NUMS, sz, ns, res.data_ptr(), stream=sh)


def ragged(code, op, arena, off_ptr, size_ptr, ns, res):
    fn = code.verify_batch_ragged if op == "verify" else code.locate_batch_ragged
    return lambda sh: fn(arena.data_ptr(), arena.numel(), 0, off_ptr, size_ptr, NUMS, ns, res.data_ptr(), stream=sh)


def corrupt(blocks, frac, seed):
    """XOR one byte of one slot in `frac` of the stripes; calling it again undoes it."""
    ns = blocks.shape[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.arange(ns, device="cuda") if frac >= 1 else \
        torch.randperm(ns, device="cuda", generator=g)[:max(1, int(ns * frac))]
    slot = torch.randint(0, NB, (idx.numel(),), device="cuda", generator=g)
    pos = torch.randint(0, SZ, (idx.numel(),), device="cuda", generator=g)
    blocks[idx, slot, pos] ^= 0x5A


def equal_sizes(args, st, code):
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
    ru, rr = result_words(ns), result_words(ns)
    res = {}
    # the ragged results against the uniform call's, with 1 % of the stripes corrupt
    corrupt(blocks, 0.01, 8)
    for op in OPS:
        uniform(code, op, blocks.data_ptr(), SZ, ns, ru)(st.cuda_stream)
        for po, ps in ((doff.data_ptr(), dsz.data_ptr()), (offs.ctypes.data, sizes.ctypes.data)):
            rr.fill_(0x55)
            ragged(code, op, arena, po, ps, ns, rr)(st.cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(ru, rr), "ragged %s differs from the uniform call" % op
        clean = 0 if op == "verify" else -1
        assert int((ru != clean).sum()) == max(1, int(ns * 0.01)), "unexpected number of dirty stripes"
    corrupt(blocks, 0.01, 8)
    for op in OPS:
        arms = with_caps({"u": uniform(code, op, blocks.data_ptr(), SZ, ns, ru),
                          "rd": ragged(code, op, arena, doff.data_ptr(), dsz.data_ptr(), ns, rr),
                          "rh": ragged(code, op, arena, offs.ctypes.data, sizes.ctypes.data, ns, rr),
                          "u2": uniform(code, op, blocks.data_ptr(), SZ, ns, ru)}, ("rd",), args.caps)
        rounds, host = run_rounds(arms, args.rounds, args.launches, st, "equal " + op)
        ragged(code, op, arena, doff.data_ptr(), dsz.data_ptr(), ns, rr)(st.cuda_stream)
        res[op] = dict(summary(rounds, "u"), host_call_us=host, kernel=capi.last_kernel_name())
    # locate against verify on the ragged calls
    lv = {}
    for name, frac in (("clean", 0.0), ("one_percent", 0.01), ("every_stripe", 1.0)):
        if frac:
            corrupt(blocks, frac, 9)
        arms = {op: (ragged(code, op, arena, doff.data_ptr(), dsz.data_ptr(), ns, rr), None) for op in OPS}
        rounds, _ = run_rounds(arms, args.rounds, args.launches, st, "locate/verify " + name)
        lv[name] = summary(rounds, "verify")
        if frac:
            corrupt(blocks, frac, 9)
    res["locate_against_verify"] = lv
    res["bytes_per_launch"] = ns * NB * SZ
    return res, blocks


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


def mixed_sizes(args, st, code, sizes, padded):
    ns = len(sizes)
    arena, offs = packed_arena(code, st, sizes)
    dsz, doff = dev_words(sizes), dev_words(offs)
    # c: the same sizes sorted, so objects of one size are contiguous
    order = np.sort(sizes)
    sorted_arena, soffs = packed_arena(code, st, order)
    vals, counts = np.unique(order, return_counts=True)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    buckets = [(int(v), int(n), int(soffs[i]), int(i)) for v, n, i in zip(vals, counts, first)]
    ra, rb, rc_ = result_words(ns), result_words(ns), result_words(ns)
    res = {}
    for op in OPS:
        a = ragged(code, op, arena, doff.data_ptr(), dsz.data_ptr(), ns, ra)
        b = uniform(code, op, padded.data_ptr(), SZ, ns, rb)
        fn = code.verify_batch if op == "verify" else code.locate_batch

        def c(sh, fn=fn):
            for v, n, o, i in buckets:
                fn(sorted_arena.data_ptr() + o, v, NB * v, NUMS, v, n, rc_.data_ptr() + 4 * i, stream=sh)

        clean = 0 if op == "verify" else -1
        for f, r in ((a, ra), (b, rb), (c, rc_)):
            r.fill_(0x55)
            f(st.cuda_stream)
            torch.cuda.synchronize()
            assert bool((r == clean).all()), "a consistent arena was judged dirty (%s)" % op
        rounds, host = run_rounds(with_caps({"a": a, "b": b, "c": c}, ("a",), args.caps), args.rounds, args.launches,
                                  st, "mixed " + op)
        res[op] = dict(summary(rounds, "a"), host_call_us=host)
    res["shape"] = {"stripes": ns, "distinct_sizes": len(buckets), "block_bytes": NB * int(sizes.sum()),
                    "padded_block_bytes": NB * ns * SZ}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--caps", type=lambda v: [int(x) for x in v.split(",") if x], default=[],
                    help="also run the ragged device-array arm under these ZFEC_HIP_GRID_CAP values")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_scrub_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_scrub_bench.py measures on a GPU"
    code = capi.Code(K, M)
    st = torch.cuda.current_stream()
    out = {"workload": "K=3/M=10, all 10 blocks held (7 checks), verify and locate, device-resident; medians of %d "
                       "alternating rounds of %d launches back to back, cold caches" % (args.rounds, args.launches),
           "device": torch.cuda.get_device_name(0)}
    out["equal_sizes_4096"], padded = equal_sizes(args, st, code)
    rng = np.random.default_rng(7)
    out["mixed_uniform_1_4096"] = mixed_sizes(args, st, code, rng.integers(1, 4097, size=args.nstripes, dtype=np.int64),
                                              padded)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
