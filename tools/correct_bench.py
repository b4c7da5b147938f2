#!/usr/bin/env python3
"""Batched in-place correction (fec_correct_batch) next to its two baselines on
the same buffer in the same process, device-resident:

  locate   fec_locate_batch alone: names the corrupt block, heals nothing
  recipe   the three-call recipe of INTEGRATION.md section 5 -- locate_batch,
           repair patterns built from the verdicts with tensor operations,
           repair_batch, copy back -- restricted to the stripes locate named
           (what a caller who scrubs mostly clean data would write; on the
           `all` data that is every stripe, the recipe as printed there)
  correct  fec_correct_batch: one call

K=3/M=10, --nstripes x 4 KiB (10^6) stripes with all ten blocks held (basis
0..2, 7 checks, block numbers 0..9 as tools/locate_bench.py), in three states:
  clean    no stripe corrupt                          (locate, correct)
  1pct     1 % of the stripes with one block overwritten
  all      one block of every stripe overwritten      (locate, recipe, correct)

Every call is timed on its own between two events.  The buffer (41 GB at the
default size) is 160 times the 256 MiB Infinity Cache, so every call starts
cold: what the previous call left in the caches is the last 0.6 % of what it
read.  The legs of a state alternate round by round (so drift hits them
alike) after two untimed rounds; a call that heals is followed, untimed, by
the same corruption again, so every timed call sees the same data.  Reported
per leg: the median, the minimum and the maximum over the rounds; per ratio:
the ratio of the medians and the smallest and largest ratio of one round.

After the rounds of a state the healed buffer is checked: the verdicts are the
known corruption, every rewritten block equals what was there before it was
overwritten, and a further locate_batch answers CLEAN for every stripe.
Writes profiles/correct_bench.json.

    python tools/correct_bench.py [--nstripes 1000000] [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zfec_amd  # noqa: E402
from zfec_amd import capi  # noqa: E402

CLEAN = zfec_amd.LOCATE_CLEAN
WARM = 2
STEP = 1 << 16  # stripes per indexed read-modify-write: bounds the temporaries


def clean_stripes(k, m, sz, ns, g):
    a = torch.empty((ns, m, sz), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 30) // (k * sz))
    for s0 in range(0, ns, step):
        n = min(step, ns - s0)
        a[s0:s0 + n, :k] = torch.randint(0, 256, (n, k, sz), dtype=torch.uint8, device="cuda", generator=g)
    capi.Code(k, m).encode_batch(a.data_ptr(), sz, m * sz, a.data_ptr() + k * sz, sz, m * sz, list(range(k, m)), sz,
                                 ns, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return a


class Spoiler(object):
    """One whole block of `frac` of the stripes overwritten (xor with bytes in
    1..255, so every byte changes), again and again with the same bytes."""

    def __init__(self, blocks, frac, g):
        ns, m, sz = blocks.shape
        n = max(1, int(ns * frac))
        self.blocks = blocks
        self.rows = torch.sort(torch.randperm(ns, device="cuda", generator=g)[:n]).values
        self.slot = torch.randint(0, m, (n,), device="cuda", generator=g)
        self.noise = torch.randint(1, 256, (n, sz), dtype=torch.uint8, device="cuda", generator=g)
        self.orig = torch.empty((n, sz), dtype=torch.uint8, device="cuda")
        for i in range(0, n, STEP):
            self.orig[i:i + STEP] = blocks[self.rows[i:i + STEP], self.slot[i:i + STEP]]
        self.want = torch.full((ns,), CLEAN, dtype=torch.int32, device="cuda")
        self.want[self.rows] = self.slot.to(torch.int32)

    def spoil(self):
        for i in range(0, len(self.rows), STEP):
            r, s = self.rows[i:i + STEP], self.slot[i:i + STEP]
            self.blocks[r, s] = self.orig[i:i + STEP] ^ self.noise[i:i + STEP]

    def healed(self):
        for i in range(0, len(self.rows), STEP):
            if not torch.equal(self.blocks[self.rows[i:i + STEP], self.slot[i:i + STEP]], self.orig[i:i + STEP]):
                return False
        return True


def recipe(dec, blocks, nums, nums_t):
    """INTEGRATION.md section 5, over the stripes locate_batch named."""
    k = dec.k
    v = dec.locate_batch(blocks, nums).long()
    hit = (v >= 0).nonzero().flatten()
    if len(hit):
        vh = v[hit]
        idx = torch.arange(k, device=blocks.device).expand(len(hit), k)
        idx = idx + (idx >= vh[:, None])  # the first k slots that are not the culprit
        held = blocks[hit[:, None], idx]
        rebuilt = dec.repair_batch(held, nums_t[idx], nums_t[vh][:, None])
        blocks[hit, vh] = rebuilt[:, 0]
    return v.to(torch.int32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "rounds": len(ms)}


def ratio(num, den):
    per_round = [a / b for a, b in zip(num, den)]
    return {"of_medians": round(statistics.median(num) / statistics.median(den), 4),
            "min_round": round(min(per_round), 4), "max_round": round(max(per_round), 4)}


def run_state(dec, blocks, nums, nums_t, frac, rounds, g):
    dirty = frac > 0
    sp = Spoiler(blocks, frac, g) if dirty else None
    want = sp.want if dirty else torch.full((blocks.shape[0],), CLEAN, dtype=torch.int32, device="cuda")
    legs = [("locate", lambda: dec.locate_batch(blocks, nums), False),
            ("correct", lambda: dec.correct_batch(blocks, nums), True)]
    if dirty:
        legs.insert(1, ("recipe", lambda: recipe(dec, blocks, nums, nums_t), True))
        sp.spoil()
    ms = {name: [] for name, _, _ in legs}
    kernels = {}
    for rnd in range(WARM + rounds):
        for name, fn, heals in legs:
            t, v = timed(fn)
            kernels[name] = capi.last_kernel_name()
            assert torch.equal(v, want), "%s: the verdicts are not the known corruption" % name
            if dirty and heals:
                assert rnd or sp.healed(), "%s did not restore the overwritten blocks" % name
                sp.spoil()
            if rnd >= WARM:
                ms[name].append(t)
    if dirty:  # the last word: one more correction, checked in full
        dec.correct_batch(blocks, nums)
        assert sp.healed(), "correct_batch did not restore the overwritten blocks"
    assert (dec.locate_batch(blocks, nums) == CLEAN).all(), "the buffer is not clean after the state"
    res = {"corrupt_stripes": int((want != CLEAN).sum()), "kernels": kernels,
           "legs": {name: summary(v) for name, v in ms.items()},
           "correct_over_locate": ratio(ms["correct"], ms["locate"])}
    if dirty:
        res["recipe_over_correct"] = ratio(ms["recipe"], ms["correct"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "correct_bench.py measures on a GPU"
    k, m, sz, ns = 3, 10, 4096, args.nstripes
    g = torch.Generator(device="cuda").manual_seed(13)
    dec = zfec_amd.Decoder(k, m)
    nums = list(range(m))
    nums_t = torch.tensor(nums, device="cuda")
    blocks = clean_stripes(k, m, sz, ns, g)
    out = {"device": torch.cuda.get_device_name(0),
           "shape": "K=%d/M=%d, %d stripes of %d bytes, all %d blocks held" % (k, m, ns, sz, m),
           "timing": "every call between two events on a buffer of %.1f GB (cold caches); the legs of a state "
                     "alternate for %d rounds after %d untimed ones; a healing call is followed, untimed, by the same "
                     "corruption again" % (blocks.numel() / 1e9, args.rounds, WARM),
           "states": {}}
    for state, frac in (("clean", 0.0), ("1pct", 0.01), ("all", 1.0)):
        out["states"][state] = run_state(dec, blocks, nums, nums_t, frac, args.rounds, g)
        torch.cuda.empty_cache()
        print(state, "done", file=sys.stderr, flush=True)
    c = out["states"]["clean"]["legs"]
    out["clean_verdict_walk_ms"] = round(c["correct"]["median_ms"] - c["locate"]["median_ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
