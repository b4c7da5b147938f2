#!/usr/bin/env python3
"""Pair location and correction (fec_locate2_batch, fec_correct2_batch) next to
their baselines on the same buffer in the same process, device-resident:

  locate    fec_locate_batch: answers MANY for a stripe with two bad blocks
  locate2   fec_locate2_batch: names the pair
  verify45  what a caller must do without it to name a pair: locate_batch, the
            MANY stripes gathered, then for each of the C(10,2) = 45 pairs the
            eight other slots gathered and fec_verify_batch on them; the pair
            whose leave-two-out scrub shows no bit is the culprit
  correct   fec_correct_batch: heals single blocks, leaves MANY stripes alone
  correct2  fec_correct2_batch: heals the pairs too

K=3/M=10, --nstripes x 4 KiB (10^6) stripes with all ten blocks held (c = 7),
in three states:
  clean   no stripe corrupt                            (no verify45)
  1pct    1 % of the stripes with two blocks overwritten
  all     two blocks of every stripe overwritten
and one wide shape, K=10/M=16, 1024 stripes of 64 KiB, all 16 blocks held, in
the same three states without verify45.

Every call is timed on its own between two events.  The legs of a state
alternate round by round (so drift hits them alike) after two untimed rounds; a
call that heals is followed, untimed, by the same corruption again, so every
timed call sees the same data.  Reported per leg: the median, the minimum and
the maximum over the rounds; per ratio: the ratio of the medians and the
smallest and largest ratio of one round.

What the clean state may cost over locate / correct is accounted for from two
measurements taken here: the time to store one verdict plane (a fill of
nstripes words) and the gap one more launch adds to a stream (a chain of
one-element kernels).  locate2 adds one plane and two launches over an empty
list (pairs_locate, pairs_finish), correct2 a third (pairs_correct).

After the rounds of a state the verdicts are the known corruption and, for the
healing legs, every overwritten block equals what was there before.  Writes
profiles/locate2_bench.json.

    python tools/locate2_bench.py [--nstripes 1000000] [--rounds 9] [--out FILE]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import zfec_amd  # noqa: E402
from zfec_amd import capi  # noqa: E402
from correct_bench import STEP, WARM, clean_stripes, ratio, summary, timed  # noqa: E402

CLEAN, MANY, NONE = zfec_amd.LOCATE_CLEAN, zfec_amd.LOCATE_MANY, zfec_amd.LOCATE_NONE


class Spoiler2(object):
    """Two whole blocks of `frac` of the stripes overwritten (xor with bytes in
    1..255, so every byte changes), again and again with the same bytes."""

    def __init__(self, blocks, frac, g):
        ns, nb, sz = blocks.shape
        n = max(1, int(ns * frac))
        self.blocks = blocks
        self.rows = torch.sort(torch.randperm(ns, device="cuda", generator=g)[:n]).values
        a = torch.randint(0, nb, (n,), device="cuda", generator=g)
        b = (a + torch.randint(1, nb, (n,), device="cuda", generator=g)) % nb
        self.slots = torch.stack([torch.minimum(a, b), torch.maximum(a, b)])  # (2, n), a < b
        self.noise = torch.randint(1, 256, (2, n, sz), dtype=torch.uint8, device="cuda", generator=g)
        self.orig = torch.empty((2, n, sz), dtype=torch.uint8, device="cuda")
        for t in range(2):
            for i in range(0, n, STEP):
                self.orig[t, i:i + STEP] = blocks[self.rows[i:i + STEP], self.slots[t, i:i + STEP]]
        self.want2 = torch.empty((2, ns), dtype=torch.int32, device="cuda")
        self.want2[0] = CLEAN
        self.want2[1] = NONE
        self.want2[:, self.rows] = self.slots.to(torch.int32)
        self.want1 = torch.full((ns,), CLEAN, dtype=torch.int32, device="cuda")
        self.want1[self.rows] = MANY

    def spoil(self):
        for t in range(2):
            for i in range(0, len(self.rows), STEP):
                r, s = self.rows[i:i + STEP], self.slots[t, i:i + STEP]
                self.blocks[r, s] = self.orig[t, i:i + STEP] ^ self.noise[t, i:i + STEP]

    def healed(self):
        for t in range(2):
            for i in range(0, len(self.rows), STEP):
                if not torch.equal(self.blocks[self.rows[i:i + STEP], self.slots[t, i:i + STEP]],
                                   self.orig[t, i:i + STEP]):
                    return False
        return True


def verify45(dec, blocks, nums):
    """Names the pairs with today's calls; returns the [2, ns] verdicts
    locate2_batch would give (for stripes with at most two bad blocks)."""
    nb = len(nums)
    v = dec.locate_batch(blocks, nums)
    out = torch.stack([v, torch.full_like(v, NONE)])
    many = (v == MANY).nonzero().flatten()
    if len(many) == 0:
        return out
    held = blocks[many]
    found = torch.zeros(len(many), dtype=torch.bool, device=blocks.device)
    for a, b in itertools.combinations(range(nb), 2):
        keep = [j for j in range(nb) if j not in (a, b)]
        sub = held[:, keep]
        ok = ~dec.verify_batch(sub, [nums[j] for j in keep]).any(dim=1) & ~found
        out[0, many[ok]] = a
        out[1, many[ok]] = b
        found |= ok
    return out


def overheads(ns):
    """(ms to store one verdict plane, ms one more launch adds to a stream)."""
    plane = torch.empty(ns, dtype=torch.int32, device="cuda")
    one = torch.zeros(1, device="cuda")
    fills, gaps = [], []
    for rnd in range(WARM + 9):
        t, _ = timed(lambda: plane.fill_(NONE))
        n = 200

        def chain():
            for _ in range(n):
                one.add_(1)
        g, _ = timed(chain)
        if rnd >= WARM:
            fills.append(t)
            gaps.append(g / n)
    return statistics.median(fills), statistics.median(gaps)


def run_state(dec, blocks, nums, frac, rounds, g, baseline):
    dirty = frac > 0
    ns = blocks.shape[0]
    sp = Spoiler2(blocks, frac, g) if dirty else None
    if dirty:
        want1, want2 = sp.want1, sp.want2
        sp.spoil()
    else:
        want1 = torch.full((ns,), CLEAN, dtype=torch.int32, device="cuda")
        want2 = torch.stack([want1, torch.full_like(want1, NONE)])
    legs = [("locate", lambda: dec.locate_batch(blocks, nums), want1, False),
            ("locate2", lambda: dec.locate2_batch(blocks, nums), want2, False)]
    if dirty and baseline:
        legs.append(("verify45", lambda: verify45(dec, blocks, nums), want2, False))
    legs += [("correct", lambda: dec.correct_batch(blocks, nums), want1, False),
             ("correct2", lambda: dec.correct2_batch(blocks, nums), want2, True)]
    ms = {leg[0]: [] for leg in legs}
    kernels = {}
    for rnd in range(WARM + rounds):
        for name, fn, want, heals in legs:
            t, v = timed(fn)
            kernels[name] = capi.last_kernel_name()
            assert torch.equal(v, want), "%s: the verdicts are not the known corruption" % name
            if dirty and heals:
                assert rnd or sp.healed(), "%s did not restore the overwritten blocks" % name
                sp.spoil()
            if rnd >= WARM:
                ms[name].append(t)
    if dirty:  # leave the buffer clean for the next state, checked in full
        dec.correct2_batch(blocks, nums)
        assert sp.healed(), "correct2_batch did not restore the overwritten blocks"
    assert (dec.locate_batch(blocks, nums) == CLEAN).all(), "the buffer is not clean after the state"
    res = {"corrupt_stripes": int((want1 != CLEAN).sum()), "kernels": kernels,
           "legs": {name: summary(v) for name, v in ms.items()},
           "locate2_over_locate": ratio(ms["locate2"], ms["locate"]),
           "correct2_over_correct": ratio(ms["correct2"], ms["correct"])}
    if "verify45" in ms:
        res["verify45_over_locate2"] = ratio(ms["verify45"], ms["locate2"])
    return res


def run_shape(k, m, sz, ns, rounds, g, baseline):
    dec = zfec_amd.Decoder(k, m)
    nums = list(range(m))
    blocks = clean_stripes(k, m, sz, ns, g)
    out = {"shape": "K=%d/M=%d, %d stripes of %d bytes, all %d blocks held (%.1f GB)"
                    % (k, m, ns, sz, m, blocks.numel() / 1e9), "states": {}}
    for state, frac in (("clean", 0.0), ("1pct", 0.01), ("all", 1.0)):
        out["states"][state] = run_state(dec, blocks, nums, frac, rounds, g, baseline)
        torch.cuda.empty_cache()
        print(k, m, state, "done", file=sys.stderr, flush=True)
    fill_ms, gap_ms = overheads(ns)
    c = out["states"]["clean"]["legs"]
    out["clean_accounting"] = {
        "plane_store_ms": round(fill_ms, 4), "launch_gap_ms": round(gap_ms, 4),
        "locate2_excess_ms": round(c["locate2"]["median_ms"] - c["locate"]["median_ms"], 4),
        "locate2_accounted_ms": round(fill_ms + 2 * gap_ms, 4),
        "correct2_excess_ms": round(c["correct2"]["median_ms"] - c["correct"]["median_ms"], 4),
        "correct2_accounted_ms": round(fill_ms + 3 * gap_ms, 4)}
    del blocks
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--wide-nstripes", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate2_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "locate2_bench.py measures on a GPU"
    g = torch.Generator(device="cuda").manual_seed(17)
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "every call between two events; the legs of a state alternate for %d rounds after %d untimed "
                     "ones; a healing call is followed, untimed, by the same corruption again" % (args.rounds, WARM),
           "headline": run_shape(3, 10, 4096, args.nstripes, args.rounds, g, True),
           "wide": run_shape(10, 16, 65536, args.wide_nstripes, args.rounds, g, False)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
