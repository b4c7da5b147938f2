#!/usr/bin/env python3
"""Batched parity verification (fec_verify_batch) against what a caller did
before it: encode the parity again into scratch and compare.  Device-resident,
timed like bench.py's cold legs: launches back to back between two events (a
spin kernel holds the stream while they are queued), rotating over two disjoint
buffer sets, each larger than the 256 MiB Infinity Cache.

Legs, for K=3/M=10 with all ten blocks present and the basis 0..2, at both
--nstripes x 4 KiB (10^6) and 256 x 1 MiB:
  a  fec_encode_batch of the 7 parity rows into scratch (the existing kernel,
     the yardstick: the same bytes moved, 7 of the 10 units as writes)
  b  (a) plus a torch compare with the stored parity: what a caller does today
  c  fec_verify_batch on clean data
  d  fec_verify_batch with 1 % of the stripes corrupted in one byte
and for K=10/M=16 on 64 x 4 MiB (the scratch path):
  e  fec_verify_batch, next to its own encode + compare

After timing, every leg's result is checked against the known corruption.
Writes profiles/verify_bench.json.

    python tools/verify_bench.py [--nstripes 1000000] [--launches 10] [--out FILE]
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

NSETS = 2
SLICE = 1 << 16  # stripes per torch compare: bounds the compare's temporary


def make_sets(code, k, m, sz, ns, st, g):
    """NSETS copies of ns clean stripes [ns, m, sz] at different addresses."""
    a = torch.empty((ns, m, sz), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 30) // (k * sz))
    for s0 in range(0, ns, step):
        n = min(step, ns - s0)
        a[s0:s0 + n, :k] = torch.randint(0, 256, (n, k, sz), dtype=torch.uint8, device="cuda", generator=g)
    code.encode_batch(a.data_ptr(), sz, m * sz, a.data_ptr() + k * sz, sz, m * sz, list(range(k, m)), sz, ns,
                      stream=st.cuda_stream)
    torch.cuda.synchronize()
    return [a] + [a.clone() for _ in range(NSETS - 1)]


def compare(scratch, blocks, k, out):
    """out[s, i] = parity row i of stripe s differs, in slices of stripes."""
    ns = blocks.shape[0]
    for s0 in range(0, ns, SLICE):
        torch.any(scratch[s0:s0 + SLICE] != blocks[s0:s0 + SLICE, k:], dim=2, out=out[s0:s0 + SLICE])


def unpack(mask, c):
    shifts = torch.arange(32, dtype=torch.int32, device=mask.device)
    bits = (mask.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(mask.shape[0], -1)[:, :c].ne(0)


def corrupt(blocks, k, frac, g):
    """Flip one byte in one block of a fraction of the stripes; returns the
    expected [ns, c] bool: a check block sets its own bit, a basis block all."""
    ns, m, sz = blocks.shape
    c = m - k
    n = max(1, int(ns * frac))
    rows = torch.randperm(ns, device="cuda", generator=g)[:n]
    slot = torch.randint(0, m, (n,), device="cuda", generator=g)
    pos = torch.randint(0, sz, (n,), device="cuda", generator=g)
    blocks[rows, slot, pos] ^= 0x5A
    want = torch.zeros((ns, c), dtype=torch.bool, device="cuda")
    want[rows] = torch.where((slot < k)[:, None], torch.ones(1, dtype=torch.bool, device="cuda"),
                             (slot - k)[:, None] == torch.arange(c, device="cuda")[None, :])
    return want


def run_code(k, m, sz, ns, launches, st, g, legs):
    code = capi.Code(k, m)
    c = m - k
    words = (c + 31) // 32
    nums = list(range(m))
    sets = make_sets(code, k, m, sz, ns, st, g)
    # one scratch for both sets: it is larger than the Infinity Cache itself, so
    # a launch finds none of the previous launch's lines in it
    scratch = torch.empty((ns, c, sz), dtype=torch.uint8, device="cuda")
    masks = [torch.full((ns, words), -1, dtype=torch.int32, device="cuda") for _ in range(NSETS)]
    diff = torch.zeros((ns, c), dtype=torch.bool, device="cuda")
    units = ns * m * sz  # bytes a leg moves: k + c rows read, or k read and c written

    def enc(i):
        def f(sh):
            code.encode_batch(sets[i].data_ptr(), sz, m * sz, scratch.data_ptr(), sz, c * sz, nums[k:], sz, ns,
                              stream=sh)
        return f

    def enc_cmp(i):
        e = enc(i)

        def f(sh):
            e(sh)
            compare(scratch, sets[i], k, diff)
        return f

    def ver(i):
        def f(sh):
            code.verify_batch(sets[i].data_ptr(), sz, m * sz, nums, sz, ns, masks[i].data_ptr(), stream=sh)
        return f

    def timed(leg, fns, moved):
        ms, host_us = bench.back_to_back(fns, launches, st, "verify " + leg)
        kern = capi.last_kernel_name()
        torch.cuda.synchronize()
        gbps = moved / (ms * 1e-3) / 1e9
        return {"kernel": kern, "ms": round(ms, 4), "GBps": round(gbps, 1),
                "hbm_frac": round(gbps / bench.HBM_PEAK_GBPS, 4), "host_call_us": round(host_us, 2)}

    res = {}
    if "a" in legs:
        res["a_encode_into_scratch"] = timed("a", [enc(i) for i in range(NSETS)], units)
        assert torch.equal(scratch[:SLICE], sets[0][:SLICE, k:]), "leg a: the parity is not the stored parity"
    if "b" in legs:
        # the compare reads the 7 scratch rows and the 7 stored rows again
        res["b_encode_then_torch_compare"] = timed("b", [enc_cmp(i) for i in range(NSETS)], units + 2 * ns * c * sz)
        assert not diff.any(), "leg b: clean data compared unequal"
    if "c" in legs:
        res["c_verify_clean"] = timed("c", [ver(i) for i in range(NSETS)], units)
        for mk in masks:
            assert not mk.any(), "leg c: clean data has mismatch bits"
    if "d" in legs:
        want = [corrupt(sets[i], k, 0.01, g) for i in range(NSETS)]
        res["d_verify_1pct_corrupt"] = timed("d", [ver(i) for i in range(NSETS)], units)
        for i in range(NSETS):
            assert torch.equal(unpack(masks[i], c), want[i]), "leg d: the masks are not the known corruption"
        res["d_verify_1pct_corrupt"]["corrupt_stripes"] = int(want[0].any(dim=1).sum())
    if "e" in legs:
        res["e_encode_then_torch_compare"] = timed("e0", [enc_cmp(i) for i in range(NSETS)],
                                                   units + 2 * ns * c * sz)
        assert not diff.any(), "leg e: clean data compared unequal"
        res["e_verify_clean"] = timed("e", [ver(i) for i in range(NSETS)], units)
        for mk in masks:
            assert not mk.any(), "leg e: clean data has mismatch bits"
        want = corrupt(sets[0], k, 0.1, g)
        ver(0)(st.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(unpack(masks[0], c), want), "leg e: the masks are not the known corruption"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "verify_bench.py measures on a GPU"
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(9)
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "%d launches back to back over %d buffer sets, cold caches" % (args.launches, NSETS),
           "configs": {}}
    shapes = [("k3_m10_%dx4KiB" % args.nstripes, 3, 10, 4096, args.nstripes, "abcd"),
              ("k3_m10_256x1MiB", 3, 10, 1 << 20, 256, "abcd"),
              ("k10_m16_64x4MiB", 10, 16, 4 << 20, 64, "e")]
    for name, k, m, sz, ns, legs in shapes:
        res = run_code(k, m, sz, ns, args.launches, st, g, legs)
        torch.cuda.empty_cache()
        print(name, "done", file=sys.stderr, flush=True)
        base =res.get("a_encode_into_scratch", res.get("e_encode_then_torch_compare"))["ms"]
        out["configs"][name] = {"legs": res, "ratio_to_first_leg": {n: round(v["ms"] / base, 4)
                                                                    for n, v in res.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
