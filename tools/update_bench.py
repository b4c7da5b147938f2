#!/usr/bin/env python3
"""The batched parity update (fec_update_batch, matupdate_reg<C,R>) with one
changed block per stripe, against its own traffic ceiling, against the sibling
kernel of fec_repair_batch and against today's alternative, fec_encode_batch of
the whole stripe.  Device-resident, all arms of a shape in one process on the
same buffers, --rounds alternating rounds, medians and the range of
single-round ratios.  Every arm is timed like bench.py's cold legs: launches
back to back between two events behind a spin kernel, after 200 ms of untimed
ones; every launch moves many times the 256 MiB Infinity Cache.

Shapes: 10^6 K=3/M=10 stripes of 4 KiB; 1024 stripes of 1 MiB of K=10/M=16,
K=20/M=24 and K=20/M=60 (40 parity rows: five row groups, each re-reading the
input).  All parity rows R = M - K are stored, packed [stripe][row][sz].

Arms:
  ud   fec_update_batch, delta form (oldb = NULL), numbers on the device
  ud2  the same call again (the A/A spread of this run)
  uo   fec_update_batch, old/new form
  rp   fec_repair_batch with pattern ids on the device, present = the k
       primaries, one target set of the same R parity rows (at most 32: the
       call's limit), into a buffer of its own
  en   fec_encode_batch of all R parity rows from the k primaries

A unit is one block of one stripe.  Each arm's bytes are the units it moves,
re-reads by row groups included (update: G*C or 2*G*C input units + R row units
read, R written, G = ceil(R / 8); repair with k <= 4: G*k + R; encode and the
wide repair: k + R), and its ceiling is bench.rw_ceiling of those bytes.
Before anything is timed the updated rows are compared with fec_encode_batch of
the changed stripes (the library against itself at the timed sizes; the tests
compare with the oracle).  Writes profiles/update_bench.json.

    python tools/update_bench.py [--rounds 9] [--launches 3] [--shapes 0,1,2,3] [--out FILE]
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

import bench  # noqa: E402  (rw_ceiling)
from zfec_amd import capi  # noqa: E402
from ragged_bench import run_rounds, summary  # noqa: E402

SHAPES = [(3, 10, 4096, 1000000), (10, 16, 1 << 20, 1024), (20, 24, 1 << 20, 1024), (20, 60, 1 << 20, 1024)]
REPAIR_MAX = 32


def rand_bytes(shape, g):
    """Random bytes without an int64 temporary: int32 words viewed as bytes."""
    n = int(np.prod(shape))
    assert n % 4 == 0
    return torch.randint(-2**31, 2**31 - 1, (n // 4,), dtype=torch.int32, device="cuda", generator=g).view(
        torch.uint8).view(shape)


def one_shape(args, st, k, m, sz, ns):
    r = m - k
    groups = -(-r // 8)
    code = capi.Code(k, m)
    g = torch.Generator(device="cuda").manual_seed(k * 100 + m)
    data = rand_bytes((ns, k, sz), g)
    par = torch.empty((ns, r, sz), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(par)
    nums = list(range(k, m))
    sh = st.cuda_stream

    def encode(src, dst):
        return lambda s: code.encode_batch(src.data_ptr(), sz, k * sz, dst.data_ptr(), sz, r * sz, nums, sz, ns,
                                           stream=s)

    encode(data, par)(sh)
    j = torch.randint(0, k, (ns,), dtype=torch.int32, device="cuda", generator=g)
    rows = torch.arange(ns, device="cuda")
    old = data[rows, j.long()].contiguous()  # [ns, sz]
    delta = rand_bytes((ns, sz), g)
    new = old ^ delta

    def update(o):
        return lambda s: code.update_batch(o.data_ptr() if o is not None else 0,
                                           (new if o is not None else delta).data_ptr(), sz, sz, par.data_ptr(), sz,
                                           r * sz, nums, j.data_ptr(), 1, sz, ns, stream=s)

    # correctness first: both forms against the library's encode of the changed stripes
    data[rows, j.long()] = new
    encode(data, out)(sh)
    update(None)(sh)
    kern = capi.last_kernel_name()
    torch.cuda.synchronize()
    assert torch.equal(par, out), "the delta-form update differs from fec_encode_batch of the changed stripes"
    update(None)(sh)   # back to the old parity
    update(old)(sh)    # and forward again, old/new form
    torch.cuda.synchronize()
    assert torch.equal(par, out), "the old/new-form update differs from fec_encode_batch of the changed stripes"

    rs = min(r, REPAIR_MAX)
    ids = torch.zeros(ns, dtype=torch.int32, device="cuda")
    present, targets = [list(range(k))], [list(range(k, k + rs))]

    def repair(s):
        code.repair_batch(data.data_ptr(), sz, k * sz, out.data_ptr(), sz, r * sz, present, targets, ids.data_ptr(), sz,
                          ns, stream=s)

    repair(sh)
    rp_kern = capi.last_kernel_name()
    encode(data, out)(sh)
    en_kern = capi.last_kernel_name()
    torch.cuda.synchronize()

    arms = {"ud": (update(None), None), "uo": (update(old), None), "rp": (repair, None), "en": (encode(data, out), None),
            "ud2": (update(None), None)}
    rounds, host = run_rounds(arms, args.rounds, args.launches, st, "update %d/%d" % (k, m))
    res = summary(rounds, "ud")
    unit = sz * ns
    rp_groups = -(-rs // 8) if k <= 4 else 1
    traffic = {"ud": (groups * 1 + r, r), "ud2": (groups * 1 + r, r), "uo": (groups * 2 + r, r),
               "rp": (rp_groups * k, rs), "en": (k, r)}
    res["units_read_written"] = {a: list(t) for a, t in traffic.items()}
    res["ceiling"] = {}
    for a, (rd, wr) in traffic.items():
        ms = res["median_ms"][a]
        gbps = (rd + wr) * unit / (ms * 1e-3) / 1e9
        c = bench.rw_ceiling(rd * unit, wr * unit, gbps)
        res["ceiling"][a] = {"GBps_moved": round(gbps, 1), "ceiling_GBps": c["GBps"],
                             "achieved_frac_of_ceiling": c["achieved_frac_of_ceiling"]}
    res["kernels"] = {"update": kern, "repair": rp_kern, "encode": en_kern}
    res["repair_targets"] = rs
    res["host_call_us"] = host
    res["shape"] = {"k": k, "m": m, "sz": sz, "nstripes": ns, "rows": r, "row_groups": groups}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--shapes", type=lambda v: [int(x) for x in v.split(",") if x], default=list(range(len(SHAPES))))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "update_bench.py measures on a GPU"
    st = torch.cuda.current_stream()
    out = {"workload": "one changed block per stripe (a random primary, numbers on the device), all R = M - K parity "
                       "rows stored packed; medians of %d alternating rounds of %d launches back to back, cold caches; "
                       "ratios are single-round ratios to the delta-form update (ud)" % (args.rounds, args.launches),
           "device": torch.cuda.get_device_name(0), "shapes": {},
           "not_measured": "more than one changed block per stripe; block-major and padded layouts; host-side numbers "
                           "at 10^6 stripes; page-locked host buffers"}
    for i in args.shapes:
        k, m, sz, ns = SHAPES[i]
        out["shapes"]["K%d_M%d_%dx%d" % (k, m, ns, sz)] = one_shape(args, st, k, m, sz, ns)
        torch.cuda.empty_cache()
        print("done", SHAPES[i], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
