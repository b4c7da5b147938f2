#!/usr/bin/env python3
"""Ragged batches (fec_encode_batch_ragged / fec_decode_batch_ragged) against
the uniform batched calls: K=3/M=10, encode of blocks 3..9 and the decode of
slots [0, 5, 9], device-resident, timed like bench.py's cold legs (launches
back to back between two events behind a spin kernel; every launch touches
many times the 256 MiB Infinity Cache), all arms in one process, --rounds
alternating rounds, medians and the range of single-round ratios.

1  equal sizes: --nstripes stripes of 4096-byte blocks on the same buffers
     u   fec_encode_batch / fec_decode_batch, packed object-major (the yardstick)
     u2  the same call again (the A/A spread of the yardstick in this run)
     rd  the ragged call, descriptor arrays in device memory (ragged_scan runs)
     rh  the ragged call, descriptor arrays in host memory (staged per call)
   The ragged call moves the same block bytes plus 32 bytes per stripe: a ratio
   beyond the A/A spread is the walk's cost.

2  mixed sizes, encode, against what a caller could do without the call:
   "uniform": --nstripes stripes of fixed-seed sizes uniform in [1, 4096];
   "tahoe": --files files of seven 43 691-byte blocks and one tail uniform in
   [1, 43 691] (128 KiB segments at k = 3)
     a  the ragged call (device arrays) on the packed objects
     b  pad every object to the longest: one uniform call over padded rows
     c  bucket by size: one uniform call per distinct size over objects already
        gathered by size (the gather itself is not charged)
     d  one call per object: timed on the first --sample objects, scaled up

--caps runs every ragged arm again under those ZFEC_HIP_GRID_CAP values: fewer
workgroups give each wave a longer contiguous range of units.

Every ragged output is compared with the uniform call's before it is timed.
Writes profiles/ragged_bench.json.

    python tools/ragged_bench.py [--nstripes 1000000] [--rounds 9] [--launches 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (back_to_back)
from zfec_amd import capi  # noqa: E402

K, M, SZ = 3, 10, 4096
R = M - K
ENC = list(range(K, M))
DEC = [0, 5, 9]
TAHOE = 43691


def summary(rounds, base):
    """rounds: arm -> [ms per round]; medians, and per arm the median and the
    range of the single-round ratios to `base`."""
    out = {"median_ms": {a: round(statistics.median(v), 4) for a, v in rounds.items()}, "ratio_to_" + base: {}}
    for a, v in rounds.items():
        q = [x / y for x, y in zip(v, rounds[base])]
        out["ratio_to_" + base][a] = {"median": round(statistics.median(q), 4), "min": round(min(q), 4),
                                      "max": round(max(q), 4)}
    out["rounds_ms"] = {a: [round(x, 4) for x in v] for a, v in rounds.items()}
    return out


def set_cap(cap):
    """ZFEC_HIP_GRID_CAP for the launches that follow (None: the library's own caps)."""
    if cap is None:
        os.environ.pop("ZFEC_HIP_GRID_CAP", None)
    else:
        os.environ["ZFEC_HIP_GRID_CAP"] = str(cap)
    capi.reload_config()


def with_caps(arms, ragged, caps):
    """arms (name -> function) as name -> (function, cap), the `ragged` ones
    again under every grid cap of --caps."""
    out = {}
    for a, fn in arms.items():
        out[a] = (fn, None)
        if a in ragged:
            for cap in caps:
                out["%s_cap%d" % (a, cap)] = (fn, cap)
    return out


def run_rounds(arms, nrounds, launches, st, tag):
    """arms: name -> (launch function(stream handle), grid cap), alternating
    within each round.  Returns the rounds' ms per launch and each arm's host
    cost per call: the mean of three calls on the idle stream (in the
    back-to-back run a ragged call may wait for one of its four staging
    slots, which only bounds the queue's depth)."""
    rounds = {a: [] for a in arms}
    host = {}
    for _ in range(nrounds):
        for a, (fn, cap) in arms.items():
            set_cap(cap)
            ms, _ = bench.back_to_back([fn], launches, st, "%s %s" % (tag, a))
            rounds[a].append(ms)
            set_cap(None)
    for a, (fn, cap) in arms.items():
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        for _ in range(3):
            fn(st.cuda_stream)
        host[a] = round((time.perf_counter() - h0) / 3 * 1e6, 1)
    torch.cuda.synchronize()
    return rounds, host


def dev_words(vals):
    return torch.as_tensor(np.asarray(vals, dtype=np.int64)).cuda()


def equal_sizes(args, st, code):
    ns = args.nstripes
    g = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randint(0, 256, (ns, K, SZ), dtype=torch.uint8, device="cuda", generator=g)
    par = torch.empty((ns, R, SZ), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(par)
    sizes = np.full(ns, SZ, dtype=np.int64)
    start = np.arange(ns, dtype=np.int64) * SZ
    h = {"sizes": sizes, "in": K * start, "enc": R * start, "dec": 2 * start}
    d = {k: dev_words(v) for k, v in h.items()}
    hp = {k: v.ctypes.data for k, v in h.items()}
    dp = {k: v.data_ptr() for k, v in d.items()}

    def uni_enc(o):
        return lambda sh: code.encode_batch(data.data_ptr(), SZ, K * SZ, o.data_ptr(), SZ, R * SZ, ENC, SZ, ns,
                                            stream=sh)

    def rag_enc(p, o):
        return lambda sh: code.encode_batch_ragged(data.data_ptr(), data.numel(), 0, p["in"], o.data_ptr(),
                                                   o.numel(), 0, p["enc"], p["sizes"], ENC, ns, stream=sh)

    uni_enc(par)(st.cuda_stream)
    for p in (dp, hp):
        out.fill_(0xA5)
        rag_enc(p, out)(st.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(out, par), "ragged encode differs from fec_encode_batch"
    kern = capi.last_kernel_name()
    arms = with_caps({"u": uni_enc(out), "rd": rag_enc(dp, out), "rh": rag_enc(hp, out), "u2": uni_enc(out)},
                     ("rd", "rh"), args.caps)
    rounds, host = run_rounds(arms, args.rounds, args.launches, st, "equal encode")
    res = {"encode": dict(summary(rounds, "u"), host_call_us=host, kernel=kern)}

    recv = torch.stack([data[:, 0], par[:, 5 - K], par[:, 9 - K]], dim=1).contiguous()
    want = data[:, 1:].contiguous()
    dout = torch.empty((ns, 2, SZ), dtype=torch.uint8, device="cuda")

    def uni_dec(sh):
        code.decode_batch(recv.data_ptr(), SZ, K * SZ, dout.data_ptr(), SZ, 2 * SZ, DEC, SZ, ns, stream=sh)

    def rag_dec(p):
        return lambda sh: code.decode_batch_ragged(recv.data_ptr(), recv.numel(), 0, p["in"], dout.data_ptr(),
                                                   dout.numel(), 0, p["dec"], p["sizes"], DEC, ns, stream=sh)

    for p in (dp, hp):
        dout.fill_(0xA5)
        rag_dec(p)(st.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(dout, want), "ragged decode did not recover the data"
    kern = capi.last_kernel_name()
    arms = with_caps({"u": uni_dec, "rd": rag_dec(dp), "rh": rag_dec(hp), "u2": uni_dec}, ("rd", "rh"), args.caps)
    rounds, host = run_rounds(arms, args.rounds, args.launches, st, "equal decode")
    res["decode"] = dict(summary(rounds, "u"), host_call_us=host, kernel=kern)
    res["bytes_per_launch"] = {"encode": ns * M * SZ, "decode": ns * (K + 2) * SZ}
    return res


def mixed_sizes(args, st, code, name, sizes):
    """Encode of packed objects of the given block sizes; arms a-d."""
    ns = len(sizes)
    start = np.cumsum(sizes) - sizes
    total, longest = int(sizes.sum()), int(sizes.max())
    g = torch.Generator(device="cuda").manual_seed(6)
    data = torch.randint(0, 256, (K * total,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.full((R * total,), 0xA5, dtype=torch.uint8, device="cuda")
    dsz, din, dout = dev_words(sizes), dev_words(K * start), dev_words(R * start)

    def a(sh):
        code.encode_batch_ragged(data.data_ptr(), data.numel(), 0, din.data_ptr(), out.data_ptr(), out.numel(), 0,
                                 dout.data_ptr(), dsz.data_ptr(), ENC, ns, stream=sh)

    # b: every object padded to the longest ([ns][K][longest] in, [ns][R][longest] out)
    pin = torch.zeros((ns, K, longest), dtype=torch.uint8, device="cuda")
    pout = torch.empty((ns, R, longest), dtype=torch.uint8, device="cuda")

    def b(sh):
        code.encode_batch(pin.data_ptr(), longest, K * longest, pout.data_ptr(), longest, R * longest, ENC, longest,
                          ns, stream=sh)

    # c: objects of one size are contiguous already when the sizes are sorted; the
    # packed arena of the sorted sizes has the same bytes in total, so the same
    # arena serves (which object a byte belongs to does not change its cost)
    order = np.sort(sizes)
    vals, counts = np.unique(order, return_counts=True)
    cstart = np.cumsum(order) - order
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    buckets = [(int(v), int(n), int(cstart[i])) for v, n, i in zip(vals, counts, first)]

    def c(sh):
        for v, n, o in buckets:
            code.encode_batch(data.data_ptr() + K * o, v, K * v, out.data_ptr() + R * o, v, R * v, ENC, v, n,
                              stream=sh)

    # d: one call per object, the first --sample of them
    sample = min(args.sample, ns)
    objs = [(int(sizes[s]), int(start[s])) for s in range(sample)]

    def d(sh):
        for v, o in objs:
            code.encode_batch(data.data_ptr() + K * o, v, K * v, out.data_ptr() + R * o, v, R * v, ENC, v, 1,
                              stream=sh)

    # the ragged output against per-object calls on the sampled objects
    a(st.cuda_stream)
    torch.cuda.synchronize()
    got = out[:R * int(start[sample - 1] + sizes[sample - 1])].clone()
    out.fill_(0xA5)
    d(st.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(got, out[:got.numel()]), "%s: ragged encode differs from per-object calls" % name
    rounds, host = run_rounds(with_caps({"a": a, "b": b, "c": c}, ("a",), args.caps), args.rounds, args.launches, st,
                              name)
    res = summary(rounds, "a")
    # d is launch-bound: one round of back-to-back passes over the sample, scaled to all objects
    ms, host_us = bench.back_to_back([d], 3, st, name + " d")
    res["d_per_object"] = {"sample": sample, "ms_sample": round(ms, 4), "ms_scaled": round(ms * ns / sample, 2),
                           "host_us_per_call": round(host_us / sample, 2)}
    res["host_call_us"] = host
    res["shape"] = {"stripes": ns, "distinct_sizes": len(buckets), "longest": longest, "block_bytes": M * total,
                    "padded_block_bytes": M * ns * longest}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--caps", type=lambda v: [int(x) for x in v.split(",") if x], default=[],
                    help="also run every ragged arm under these ZFEC_HIP_GRID_CAP values (the units-per-wave A/B)")
    ap.add_argument("--only", choices=["equal", "mixed"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_bench.py measures on a GPU"
    code = capi.Code(K, M)
    st = torch.cuda.current_stream()
    out = {"workload": "K=3/M=10, encode of blocks 3..9 and decode of slots [0, 5, 9], device-resident; medians of %d "
                       "alternating rounds of %d launches back to back, cold caches" % (args.rounds, args.launches),
           "device": torch.cuda.get_device_name(0)}
    if args.only != "mixed":
        out["equal_sizes_4096"] = equal_sizes(args, st, code)
        torch.cuda.empty_cache()
    if args.only != "equal":
        rng = np.random.default_rng(7)
        out["mixed_uniform_1_4096"] = mixed_sizes(args, st, code, "uniform",
                                                  rng.integers(1, 4097, size=args.nstripes, dtype=np.int64))
        torch.cuda.empty_cache()
        tails = rng.integers(1, TAHOE + 1, size=args.files, dtype=np.int64)
        tahoe = np.concatenate([np.full((args.files, 7), TAHOE, dtype=np.int64), tails[:, None]], axis=1).reshape(-1)
        out["mixed_tahoe_segments"] = mixed_sizes(args, st, code, "tahoe", tahoe)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
