#!/usr/bin/env python3
"""Batched error location (fec_locate_batch) next to fec_verify_batch on the
same buffers in the same process.  Device-resident, timed like
tools/verify_bench.py: launches back to back between two events (a spin kernel
holds the stream while they are queued), rotating over two disjoint buffer
sets, each larger than the 256 MiB Infinity Cache.

K=3/M=10, --nstripes x 4 KiB (10^6) stripes with all ten blocks held (basis
0..2, 7 checks), in three states of the data:
  clean      no stripe corrupt
  1pct       1 % of the stripes with one flipped byte in one block
  all        every stripe with one whole block overwritten
Each state times verify_batch, locate_batch, verify_batch and locate_batch
again (two rounds, so drift shows), and reports locate / verify from the
faster round of each.  `leave_one_out` times today's way of locating on the
1pct data: nb verify_batch calls, each over nb - 1 of the blocks.  (A strided
layout can leave out only the first or the last slot without a gather, so the
calls alternate between slots 1..nb-1 and 0..nb-2; the gathers a caller would
need for the slots in between are not counted.)  One K=10/M=16 leg on 64 x
4 MiB covers the scratch path (rows_locate), clean and with 10 % of the stripes
corrupt.

After timing, every verdict is checked against the known corruption.
Writes profiles/locate_bench.json.

    python tools/locate_bench.py [--nstripes 1000000] [--launches 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (back_to_back, HBM peak)
from zfec_amd import capi  # noqa: E402
from verify_bench import NSETS, make_sets  # noqa: E402

CLEAN = -1


def flip_bytes(blocks, frac, g):
    """One flipped byte in one block of a fraction of the stripes; returns the
    expected int32 verdicts and a function that flips the bytes back."""
    ns, m, sz = blocks.shape
    n = max(1, int(ns * frac))
    rows = torch.randperm(ns, device="cuda", generator=g)[:n]
    slot = torch.randint(0, m, (n,), device="cuda", generator=g)
    pos = torch.randint(0, sz, (n,), device="cuda", generator=g)
    blocks[rows, slot, pos] ^= 0x5A
    want = torch.full((ns,), CLEAN, dtype=torch.int32, device="cuda")
    want[rows] = slot.to(torch.int32)

    def undo():
        blocks[rows, slot, pos] ^= 0x5A
    return want, undo


def overwrite_blocks(blocks, g):
    """One whole block of every stripe overwritten with random bytes (xor with
    1..255, so every byte changes); returns the expected int32 verdicts."""
    ns, m, sz = blocks.shape
    slot = torch.randint(0, m, (ns,), device="cuda", generator=g)
    step = 1 << 16
    for s0 in range(0, ns, step):
        n = min(step, ns - s0)
        rows = torch.arange(s0, s0 + n, device="cuda")
        blocks[rows, slot[s0:s0 + n]] ^= torch.randint(1, 256, (n, sz), dtype=torch.uint8, device="cuda", generator=g)
    return slot.to(torch.int32)


def run_code(k, m, sz, ns, launches, st, g, states, leave_one_out):
    code = capi.Code(k, m)
    c = m - k
    words = (c + 31) // 32
    nums = list(range(m))
    sets = make_sets(code, k, m, sz, ns, st, g)
    masks = [torch.full((ns, words), -1, dtype=torch.int32, device="cuda") for _ in range(NSETS)]
    outs = [torch.full((ns,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(NSETS)]
    moved = ns * m * sz  # bytes a call reads

    def ver(i, first=0, nb=m):
        ptr = sets[i].data_ptr() + first * sz

        def f(sh):
            code.verify_batch(ptr, sz, m * sz, nums[first:first + nb], sz, ns, masks[i].data_ptr(), stream=sh)
        return f

    def loc(i):
        def f(sh):
            code.locate_batch(sets[i].data_ptr(), sz, m * sz, nums, sz, ns, outs[i].data_ptr(), stream=sh)
        return f

    def timed(leg, fns, nbytes):
        ms, host_us = bench.back_to_back(fns, launches, st, "locate " + leg)
        kern = capi.last_kernel_name()
        torch.cuda.synchronize()
        gbps = nbytes / (ms * 1e-3) / 1e9
        return {"kernel": kern, "ms": round(ms, 4), "GBps": round(gbps, 1),
                "hbm_frac": round(gbps / bench.HBM_PEAK_GBPS, 4), "host_call_us": round(host_us, 2)}

    res = {}
    for state, frac in states:
        if state == "clean":
            want = [torch.full((ns,), CLEAN, dtype=torch.int32, device="cuda")] * NSETS
        elif state == "all":
            want = [overwrite_blocks(sets[i], g) for i in range(NSETS)]
        else:
            flipped = [flip_bytes(sets[i], frac, g) for i in range(NSETS)]
            want = [w for w, _ in flipped]
        legs = {}
        for rnd in (1, 2):
            legs["verify_%d" % rnd] = timed("%s verify %d" % (state, rnd), [ver(i) for i in range(NSETS)], moved)
            legs["locate_%d" % rnd] = timed("%s locate %d" % (state, rnd), [loc(i) for i in range(NSETS)], moved)
        for i in range(NSETS):
            assert torch.equal(outs[i], want[i]), "%s: the verdicts are not the known corruption" % state
            assert torch.equal(masks[i].ne(0).any(dim=1), want[i] != CLEAN), "%s: verify disagrees" % state
        v = min(legs["verify_1"]["ms"], legs["verify_2"]["ms"])
        ell = min(legs["locate_1"]["ms"], legs["locate_2"]["ms"])
        res[state] = {"legs": legs, "corrupt_stripes": int((want[0] != CLEAN).sum()),
                      "locate_over_verify": round(ell / v, 4)}
        if leave_one_out and state == "1pct":
            # nb calls per locate: the calls of one set back to back, first slot or last slot left out
            fns = [ver(i, first=h % 2, nb=m - 1) for i in range(NSETS) for h in range(m)]
            one = timed("leave one out", fns, ns * (m - 1) * sz)
            one["calls_per_locate"] = m
            one["ms_per_locate"] = round(one["ms"] * m, 4)
            res["leave_one_out_1pct"] = one
            res["leave_one_out_over_locate"] = round(one["ms"] * m / ell, 2)
        if state not in ("clean", "all"):
            for _, undo in flipped:
                undo()  # the next state starts from clean data
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "locate_bench.py measures on a GPU"
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(11)
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "%d launches back to back over %d buffer sets, cold caches; verify and locate alternate twice "
                     "per data state, the ratio takes the faster round of each" % (args.launches, NSETS),
           "configs": {}}
    shapes = [("k3_m10_%dx4KiB" % args.nstripes, 3, 10, 4096, args.nstripes,
               [("clean", 0), ("1pct", 0.01), ("all", 1)], True),
              ("k10_m16_64x4MiB", 10, 16, 4 << 20, 64, [("clean", 0), ("10pct", 0.1)], False)]
    for name, k, m, sz, ns, states, loo in shapes:
        out["configs"][name] = run_code(k, m, sz, ns, args.launches, st, g, states, loo)
        torch.cuda.empty_cache()
        print(name, "done", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
