#!/usr/bin/env python3
"""Batched repair (fec_repair_batch) against the batched decode with a pattern
per stripe: K=3/M=10, 4 KiB blocks, --nstripes objects (10^6), device-resident,
pattern ids on the device, timed like bench.py's cold legs: launches back to
back between two events after 200 ms of untimed ones (a spin kernel holds the
stream while they are queued), rotating over two disjoint buffer sets, each
many times the 256 MiB Infinity Cache.

Every stripe holds a random one of the 120 three-subsets of 10.  Legs:
  a  fec_decode_batch_mixed on those blocks (matapply_mixed<3>: the yardstick;
     reads 3 and writes 3 units per stripe)
  b  fec_repair_batch, t = 1: one random lost block per stripe, primaries and
     parity mixed (reads 3, writes 1)
  c  fec_repair_batch, t = 2, the second target NONE for half the stripes
     (reads 3, writes 1.5 on average)
  d  fec_repair_batch, t = 7: all seven absent blocks (reads 3, writes 7)
  e  what a caller did for (b) before: (a), then fec_encode_batch of all 7
     parity rows (reads 3 + 3, writes 3 + 7)

Every leg's output is compared with the stripes' own blocks after the timed
launches, and the rows of NONE targets with the fill they started with.
A unit is one 4 KiB block of one stripe; hbm_frac is the units a leg moves
over bench.py's HBM peak.  Writes profiles/repair_bench.json.

    python tools/repair_bench.py [--nstripes 1000000] [--launches 10] [--out FILE]
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
FILL = 0xA5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_bench.json"))
    args = ap.parse_args()
    ns = args.nstripes
    assert torch.cuda.is_available(), "repair_bench.py measures on a GPU"
    code = capi.Code(K, M)
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(5)
    # every block of every stripe: [ns, M, SZ]
    allb = torch.empty((ns, M, SZ), dtype=torch.uint8, device="cuda")
    allb[:, :K] = torch.randint(0, 256, (ns, K, SZ), dtype=torch.uint8, device="cuda", generator=g)
    code.encode_batch(allb.data_ptr(), SZ, M * SZ, allb.data_ptr() + K * SZ, SZ, M * SZ, list(range(K, M)), SZ, ns,
                      stream=st.cuda_stream)
    torch.cuda.synchronize()
    subs = [list(c) for c in itertools.combinations(range(M), K)]
    gone = [[b for b in range(M) if b not in s] for s in subs]  # each subset's 7 absent blocks
    nsub, ngone = len(subs), M - K
    subs_t = torch.tensor(subs, device="cuda")
    rows = torch.arange(ns, device="cuda")

    def rnd(hi):
        return [torch.randint(0, hi, (ns,), dtype=torch.int32, device="cuda", generator=g) for _ in range(NSETS)]

    sid = rnd(nsub)  # set i: its own assignment of subsets to stripes
    recv = [allb[rows[:, None], subs_t[sid[i].long()]].contiguous() for i in range(NSETS)]  # [ns, K, SZ]

    def timed(leg, fns, checks, units):
        """checks[i](): leg's outputs of set i against the stripes' blocks; units: per stripe."""
        ms, _ = bench.back_to_back(fns, args.launches, st, "repair " + leg)
        kern = capi.last_kernel_name()
        torch.cuda.synchronize()
        # host cost of a call: the mean of three on the idle stream, after the
        # timed run (in the back-to-back run itself a call may wait for one of
        # its four staging slots, which only bounds the queue's depth)
        h0 = time.perf_counter()
        for i in range(3):
            fns[i % len(fns)](st.cuda_stream)
        host_us = (time.perf_counter() - h0) / 3 * 1e6
        torch.cuda.synchronize()
        for c in checks:
            c()
        gbps = units * ns * SZ / (ms * 1e-3) / 1e9
        return {"kernel": kern, "ms": round(ms, 4), "units_per_stripe": round(units, 4), "GBps_moved": round(gbps, 1),
                "hbm_frac": round(gbps / bench.HBM_PEAK_GBPS, 4), "host_call_us": round(host_us, 2)}

    def check_rows(leg, out, tg):
        """out [ns, t, SZ] against targets tg [ns, t] (-1: NONE, the row keeps FILL)."""
        def f():
            for i in range(tg.shape[1]):
                live = tg[:, i] >= 0
                got = out[:, i]
                assert torch.equal(got[live], allb[rows[live], tg[:, i][live].long()]), \
                    "leg %s: row %d is not the target block" % (leg, i)
                assert bool((got[~live] == FILL).all()), "leg %s: a NONE row %d was written" % (leg, i)
        return f

    def repair_fn(i, out, pres, tgts, ids):
        t = tgts.shape[1]

        def f(sh):
            code.repair_batch(recv[i].data_ptr(), SZ, K * SZ, out.data_ptr(), SZ, t * SZ, pres, tgts, ids.data_ptr(), SZ,
                              ns, stream=sh)
        return f

    res = {}
    subs_np = np.asarray(subs, dtype=np.int64)
    gone_np = np.asarray(gone, dtype=np.int64)
    gone_t = torch.tensor(gone, device="cuda")

    # a: the yardstick
    prim = [torch.full((ns, K, SZ), FILL, dtype=torch.uint8, device="cuda") for _ in range(NSETS)]

    def mixed_fn(i):
        def f(sh):
            code.decode_batch_mixed(recv[i].data_ptr(), SZ, K * SZ, prim[i].data_ptr(), SZ, K * SZ, subs_np,
                                    sid[i].data_ptr(), SZ, ns, stream=sh)
        return f

    def check_prim(leg, i):
        def f():
            assert torch.equal(prim[i], allb[:, :K]), "leg %s: the output is not the data" % leg
        return f

    res["a_decode_mixed"] = timed("a", [mixed_fn(i) for i in range(NSETS)],
                                  [check_prim("a", i) for i in range(NSETS)], 2 * K)

    # b: t = 1, pattern id = subset * 7 + which absent block
    lost = rnd(ngone)
    pres_b = np.repeat(subs_np, ngone, axis=0)
    tgts_b = gone_np.reshape(-1, 1)
    ids_b = [(sid[i] * ngone + lost[i]).contiguous() for i in range(NSETS)]
    tg_b = [gone_t[sid[i].long(), lost[i].long()][:, None] for i in range(NSETS)]
    outs = [torch.full((ns, 1, SZ), FILL, dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
    res["b_repair_t1"] = timed("b", [repair_fn(i, outs[i], pres_b, tgts_b, ids_b[i]) for i in range(NSETS)],
                               [check_rows("b", outs[i], tg_b[i]) for i in range(NSETS)], K + 1)
    del outs

    # c: t = 2, pattern id = (subset * 7 + first) * 8 + second, second == 7: NONE
    half = rnd(2)
    second = [torch.where(half[i] == 0, torch.full_like(lost[i], ngone), x) for i, x in enumerate(rnd(ngone))]
    pres_c = np.repeat(subs_np, ngone * (ngone + 1), axis=0)
    sec_np = np.concatenate([gone_np, np.full((nsub, 1), -1)], axis=1)  # [nsub, 8]
    tgts_c = np.stack([np.repeat(gone_np.reshape(-1), ngone + 1),
                       np.repeat(sec_np, ngone, axis=0).reshape(-1)], axis=1)
    ids_c = [((sid[i] * ngone + lost[i]) * (ngone + 1) + second[i]).contiguous() for i in range(NSETS)]
    tg_c = [torch.from_numpy(tgts_c).cuda()[ids_c[i].long()] for i in range(NSETS)]
    live_c = float(sum((t >= 0).sum().item() for t in tg_c)) / (NSETS * ns)
    outs = [torch.full((ns, 2, SZ), FILL, dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
    res["c_repair_t2_half_none"] = timed("c", [repair_fn(i, outs[i], pres_c, tgts_c, ids_c[i]) for i in range(NSETS)],
                                         [check_rows("c", outs[i], tg_c[i]) for i in range(NSETS)], K + live_c)
    res["c_repair_t2_half_none"]["patterns"] = int(pres_c.shape[0])
    del outs, tg_c

    # d: t = 7, every absent block
    outs = [torch.full((ns, ngone, SZ), FILL, dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
    tg_d = [gone_t[sid[i].long()] for i in range(NSETS)]
    res["d_repair_t7"] = timed("d", [repair_fn(i, outs[i], subs_np, gone_np, sid[i]) for i in range(NSETS)],
                               [check_rows("d", outs[i], tg_d[i]) for i in range(NSETS)], K + ngone)
    del tg_d

    # e: decode, then encode all 7 parity rows (the caller then picks the one it lost)
    par = outs

    def long_fn(i):
        def f(sh):
            mixed_fn(i)(sh)
            code.encode_batch(prim[i].data_ptr(), SZ, K * SZ, par[i].data_ptr(), SZ, ngone * SZ,
                              list(range(K, M)), SZ, ns, stream=sh)
        return f

    def check_long(i):
        def f():
            assert torch.equal(prim[i], allb[:, :K]) and torch.equal(par[i], allb[:, K:]), "leg e: wrong output"
        return f

    for p in prim + par:
        p.fill_(FILL)
    res["e_decode_then_encode7"] = timed("e", [long_fn(i) for i in range(NSETS)],
                                         [check_long(i) for i in range(NSETS)], 2 * K + K + ngone)

    a, b = res["a_decode_mixed"]["ms"], res["b_repair_t1"]["ms"]
    out = {"workload": "K=3/M=10, %d stripes of 4 KiB blocks, device-resident, each holding a random 3-subset, ids on "
                       "the device; %d launches back to back over %d buffer sets" % (ns, args.launches, NSETS),
           "device": torch.cuda.get_device_name(0), "legs": res,
           "b_over_a": round(b / a, 4), "e_over_b": round(res["e_decode_then_encode7"]["ms"] / b, 4),
           "not_measured": "blocks under 1 KiB; K = 1, 2, 4; ids in host memory at this size; the k > 4 path"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
