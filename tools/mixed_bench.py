#!/usr/bin/env python3
"""Batched decode with a pattern per stripe (fec_decode_batch_mixed) against
the shared-pattern call: K=3/M=10, 4 KiB blocks, --nstripes objects (10^6),
device-resident, every leg writing all 3 primaries of every stripe, timed like
bench.py's cold legs: launches back to back between two events (a spin kernel
holds the stream while they are queued), rotating over two disjoint buffer
sets, each many times the 256 MiB Infinity Cache.

Legs:
  a  fec_decode_batch, FEC_FLAG_ALL_PRIMARIES, the one pattern [7, 8, 9]
     (matapply_rows<3,3>: the existing kernel, the yardstick)
  b  fec_decode_batch_mixed, the same one pattern
  c  fec_decode_batch_mixed, all 120 three-subsets of 10 assigned at random
  d  fec_decode_batch_mixed, the same 120 patterns in sorted runs
  e  what the library offered for (d) before: 120 jobs through
     fec_run_batch_jobs, one per run

The 120 patterns keep fec_decode's slot rule (primary i at slot i), which (e)
needs; ids live on the device.  Every leg's output is compared with the
original data after the timed launches.  Writes profiles/mixed_decode_bench.json.

    python tools/mixed_bench.py [--nstripes 1000000] [--launches 10] [--out FILE]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (back_to_back, HBM peak)
from zfec_amd import capi  # noqa: E402

K, M, SZ = 3, 10, 4096
NSETS = 2


def place(sub):
    """The subset in slot order with primary i at slot i."""
    slots = [None] * K
    sec = iter([n for n in sub if n >= K])
    for n in sub:
        if n < K:
            slots[n] = n
    return [s if s is not None else next(sec) for s in slots]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_decode_bench.json"))
    args = ap.parse_args()
    ns = args.nstripes
    assert torch.cuda.is_available(), "mixed_bench.py measures on a GPU"
    code = capi.Code(K, M)
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(3)
    # every block of every stripe: [ns, M, SZ]
    allb = torch.empty((ns, M, SZ), dtype=torch.uint8, device="cuda")
    allb[:, :K] = torch.randint(0, 256, (ns, K, SZ), dtype=torch.uint8, device="cuda", generator=g)
    code.encode_batch(allb.data_ptr(), SZ, M * SZ, allb.data_ptr() + K * SZ, SZ, M * SZ, list(range(K, M)), SZ, ns,
                      stream=st.cuda_stream)
    torch.cuda.synchronize()
    data = allb[:, :K]
    pats = [place(c) for c in itertools.combinations(range(M), K)]
    pats_t = torch.tensor(pats, device="cuda")
    rows = torch.arange(ns, device="cuda")[:, None]

    def gather(ids):
        return allb[rows, pats_t[ids.long()]].contiguous()  # [ns, K, SZ]

    def timed(leg, fns, outs):
        ms, _ = bench.back_to_back(fns, args.launches, st, "mixed " + leg)
        kern = capi.last_kernel_name()
        torch.cuda.synchronize()
        # host cost of a call: the mean of three on the idle stream, after the
        # timed run (in the back-to-back run itself a mixed call may wait for
        # one of its four staging slots, which only bounds the queue's depth)
        h0 = time.perf_counter()
        for i in range(3):
            fns[i % len(fns)](st.cuda_stream)
        host_us = (time.perf_counter() - h0) / 3 * 1e6
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, data), "leg %s: the output is not the data" % leg
            o.fill_(0xA5)
        gbps = 2 * ns * K * SZ / (ms * 1e-3) / 1e9
        return {"kernel": kern, "ms": round(ms, 4), "GBps_in_plus_out": round(gbps, 1),
                "hbm_frac": round(gbps / bench.HBM_PEAK_GBPS, 4), "host_call_us": round(host_us, 2)}

    res = {}
    outs = [torch.full((ns, K, SZ), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
    args5 = (SZ, K * SZ)

    def mixed_fn(recv, out, plist, ids):
        def f(sh):
            code.decode_batch_mixed(recv.data_ptr(), *args5, out.data_ptr(), *args5, plist, ids.data_ptr(), SZ, ns,
                                    stream=sh)
        return f

    # a, b: one pattern
    one = [7, 8, 9]
    recv = [allb[:, 7:10].contiguous() for _ in range(NSETS)]
    zeros = torch.zeros(ns, dtype=torch.int32, device="cuda")

    def shared_fn(i):
        def f(sh):
            code.decode_batch(recv[i].data_ptr(), *args5, outs[i].data_ptr(), *args5, one, SZ, ns, stream=sh,
                              flags=capi.FEC_FLAG_ASYNC | capi.FEC_FLAG_ALL_PRIMARIES)
        return f

    res["a_shared_one_pattern"] = timed("a", [shared_fn(i) for i in range(NSETS)], outs)
    res["b_mixed_one_pattern"] = timed("b", [mixed_fn(recv[i], outs[i], [one], zeros) for i in range(NSETS)], outs)
    del recv
    torch.cuda.empty_cache()

    # c: 120 patterns at random (set i: its own assignment)
    ids_c = [torch.randint(0, len(pats), (ns,), dtype=torch.int32, device="cuda", generator=g) for _ in range(NSETS)]
    recv = [gather(ids_c[i]) for i in range(NSETS)]
    pnp = np.asarray(pats, dtype=np.uint32)
    res["c_mixed_120_random"] = timed("c", [mixed_fn(recv[i], outs[i], pnp, ids_c[i]) for i in range(NSETS)], outs)
    del recv
    torch.cuda.empty_cache()

    # d, e: the same assignments in sorted runs
    ids_d = [torch.sort(ids_c[i]).values.contiguous() for i in range(NSETS)]
    recv = [gather(ids_d[i]) for i in range(NSETS)]
    # the data of stripe s is data[s] in every leg: only the received blocks follow the ids
    res["d_mixed_120_sorted"] = timed("d", [mixed_fn(recv[i], outs[i], pnp, ids_d[i]) for i in range(NSETS)], outs)
    jobs = []
    for i in range(NSETS):
        counts = torch.bincount(ids_d[i].long(), minlength=len(pats)).cpu().tolist()
        js, s0 = [], 0
        for p, n in enumerate(counts):
            if n:
                js.append(capi.decode_job(code, recv[i].data_ptr() + s0 * K * SZ, *args5,
                                          outs[i].data_ptr() + s0 * K * SZ, *args5, pats[p], SZ, n,
                                          flags=capi.FEC_FLAG_ALL_PRIMARIES))
            s0 += n
        jobs.append(capi.BatchJobs(js))
    res["e_120_batch_jobs_sorted"] = timed("e", [lambda sh, j=j: j.run(stream=sh) for j in jobs], outs)
    res["e_120_batch_jobs_sorted"]["jobs"] = jobs[0].n

    a = res["a_shared_one_pattern"]["ms"]
    out = {"workload": "K=3/M=10, %d stripes of 4 KiB blocks, device-resident, all 3 primaries written; %d launches "
                       "back to back over %d buffer sets" % (ns, args.launches, NSETS),
           "device": torch.cuda.get_device_name(0), "legs": res,
           "ratio_to_a": {k: round(v["ms"] / a, 4) for k, v in res.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
