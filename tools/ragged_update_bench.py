#!/usr/bin/env python3
"""The ragged parity update (fec_update_batch_ragged) against the uniform call
(fec_update_batch): device-resident, all arms of a shape in one process on the
same buffers, --rounds alternating rounds of --launches launches back to back,
medians and the range of single-round ratios (tools/ragged_bench.py's method).
One changed block per stripe in delta form, plus the old/new form once.  An
update XORs into its rows, so repeated launches need no reset: the bytes
differ, the traffic does not.

a  mixed sizes: --nstripes K=3/M=10 stripes, 7 parity rows, block sizes of a
   fixed seed uniform in [1, 4096]
     a  the ragged call (device arrays) on the packed objects
     b  pad every delta and every row to 4096: one uniform call
     c  one uniform call per distinct size over objects already gathered by
        size (the gather itself is not charged)
b  equal sizes: --nstripes stripes of 4096-byte blocks on the same buffers
     u / u2  fec_update_batch, and the same call again (the A/A spread)
     rd / rh the ragged call, descriptors and numbers in device / host memory
     uo / ro both calls in the old/new form
   --caps runs rd again under those ZFEC_HIP_GRID_CAP values (--sweep: the caps
   that give 2, 4, 8 and 16 units per wave).
c  one wide shape: --wide K=20/M=24 stripes, 4 parity rows, sizes uniform in
   [1, 2^20]: the ragged call against the uniform call padded to the longest.

The ragged result is compared with the uniform call's on a sample before
anything is timed.  Writes profiles/ragged_update_bench.json.

    python tools/ragged_update_bench.py [--nstripes 1000000] [--wide 1024] [--rounds 9] [--launches 5] [--sweep]
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

SZ = 4096


def rand(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def numbers(k, ns, seed):
    """One changed primary per stripe: uint32 words on the host and on the device."""
    ch = np.random.default_rng(seed).integers(0, k, size=ns).astype(np.uint32)
    return ch, torch.as_tensor(ch.view(np.int32)).cuda()


def uniform(code, nums, old, new, rows, sz, ns, ch_ptr):
    r = len(nums)
    return lambda sh: code.update_batch(old, new, sz, sz, rows, sz, r * sz, nums, ch_ptr, 1, sz, ns, stream=sh)


def ragged(code, nums, old, new, rows, p, ch_ptr, ns):
    return lambda sh: code.update_batch_ragged(old.data_ptr() if old is not None else 0, new.data_ptr(), new.numel(), 0,
                                               p["in"], rows.data_ptr(), rows.numel(), 0, p["rows"], p["sizes"], nums,
                                               ch_ptr, 1, ns, stream=sh)


def same_as_uniform(code, k, nums, st):
    """Both forms on 4096 stripes of 4 KiB, host and device arrays: the ragged rows are the uniform call's."""
    ns, r = 4096, len(nums)
    ch, dch = numbers(k, ns, 3)
    new, old, rows0 = rand(ns * SZ, 1), rand(ns * SZ, 2), rand(ns * r * SZ, 4)
    start = np.arange(ns, dtype=np.int64) * SZ
    h = {"sizes": np.full(ns, SZ, dtype=np.int64), "in": start, "rows": r * start}
    d = {key: dev_words(v) for key, v in h.items()}
    for o in (None, old):
        want = rows0.clone()
        uniform(code, nums, o.data_ptr() if o is not None else 0, new.data_ptr(), want.data_ptr(), SZ, ns,
                dch.data_ptr())(st.cuda_stream)
        for p, cp in (({key: v.data_ptr() for key, v in d.items()}, dch.data_ptr()),
                      ({key: v.ctypes.data for key, v in h.items()}, ch.ctypes.data)):
            got = rows0.clone()
            ragged(code, nums, o, new, got, p, cp, ns)(st.cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(got, want), "the ragged update differs from fec_update_batch"
    return capi.last_kernel_name()


def equal_sizes(args, st, code, k, nums):
    ns, r = args.nstripes, len(nums)
    ch, dch = numbers(k, ns, 7)
    new, old, rows = rand(ns * SZ, 5), rand(ns * SZ, 6), rand(ns * r * SZ, 8)
    start = np.arange(ns, dtype=np.int64) * SZ
    h = {"sizes": np.full(ns, SZ, dtype=np.int64), "in": start, "rows": r * start}
    d = {key: dev_words(v) for key, v in h.items()}
    hp, dp = {key: v.ctypes.data for key, v in h.items()}, {key: v.data_ptr() for key, v in d.items()}
    arms = {"u": uniform(code, nums, 0, new.data_ptr(), rows.data_ptr(), SZ, ns, dch.data_ptr()),
            "rd": ragged(code, nums, None, new, rows, dp, dch.data_ptr(), ns),
            "rh": ragged(code, nums, None, new, rows, hp, ch.ctypes.data, ns),
            "u2": uniform(code, nums, 0, new.data_ptr(), rows.data_ptr(), SZ, ns, dch.data_ptr()),
            "uo": uniform(code, nums, old.data_ptr(), new.data_ptr(), rows.data_ptr(), SZ, ns, dch.data_ptr()),
            "ro": ragged(code, nums, old, new, rows, dp, dch.data_ptr(), ns)}
    rounds, host = run_rounds(with_caps(arms, ("rd",), args.caps), args.rounds, args.launches, st, "equal sizes")
    res = dict(summary(rounds, "u"), host_call_us=host, bytes_per_launch=ns * (1 + 2 * r) * SZ,
               bytes_per_launch_oldnew=ns * (2 + 2 * r) * SZ)
    med = res["median_ms"]
    res["oldnew_ragged_over_uniform"] = round(med["ro"] / med["uo"], 4)
    return res


def mixed_sizes(args, st, code, k, nums, sizes, seed):
    """a: ragged on packed objects; b: padded to the longest; c (optional): a call per distinct size."""
    ns, r = len(sizes), len(nums)
    total, longest = int(sizes.sum()), int(sizes.max())
    start = np.cumsum(sizes) - sizes
    ch, dch = numbers(k, ns, seed)
    new_a, rows_a = rand(total, seed + 1), rand(r * total, seed + 2)
    pa = {key: dev_words(v) for key, v in {"sizes": sizes, "in": start, "rows": r * start}.items()}
    arms = {"a": ragged(code, nums, None, new_a, rows_a, {key: v.data_ptr() for key, v in pa.items()}, dch.data_ptr(),
                        ns)}
    new_b, rows_b = rand(ns * longest, seed + 3), rand(ns * r * longest, seed + 4)
    arms["b"] = uniform(code, nums, 0, new_b.data_ptr(), rows_b.data_ptr(), longest, ns, dch.data_ptr())
    shape = {"stripes": ns, "bytes_moved": (1 + 2 * r) * total, "padded_bytes_moved": (1 + 2 * r) * ns * longest}
    if args.by_size and len(np.unique(sizes)) <= 8192:
        order = np.argsort(sizes, kind="stable")
        ssz = sizes[order]
        sstart = np.cumsum(ssz) - ssz
        sch = torch.as_tensor(ch[order].view(np.int32)).cuda()
        new_c, rows_c = rand(total, seed + 5), rand(r * total, seed + 6)
        vals, counts = np.unique(ssz, return_counts=True)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        buckets = [(int(v), int(n), int(sstart[i]), int(i)) for v, n, i in zip(vals, counts, first)]
        shape["distinct_sizes"] = len(buckets)

        def c(sh):
            for v, n, o, i in buckets:
                code.update_batch(0, new_c.data_ptr() + o, v, v, rows_c.data_ptr() + r * o, v, r * v, nums,
                                  sch.data_ptr() + 4 * i, 1, v, n, stream=sh)

        arms["c"] = c
    for f in arms.values():
        f(st.cuda_stream)
    torch.cuda.synchronize()
    rounds, host = run_rounds(with_caps(arms, ("a",), args.caps), args.rounds, args.launches, st, "mixed sizes")
    return dict(summary(rounds, "a"), host_call_us=host, shape=shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstripes", type=int, default=1000000)
    ap.add_argument("--wide", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--caps", type=lambda v: [int(x) for x in v.split(",") if x], default=[],
                    help="also run the ragged device-array arms under these ZFEC_HIP_GRID_CAP values")
    ap.add_argument("--sweep", action="store_true",
                    help="--caps that give the equal-size arm 2, 4, 8 and 16 units per wave")
    ap.add_argument("--no-by-size", dest="by_size", action="store_false")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_update_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ragged_update_bench.py measures on a GPU"
    if args.sweep:  # 4 units per stripe, 4 waves per workgroup
        units = args.nstripes * (SZ // 1024)
        args.caps = sorted({-(-units // (4 * upw)) for upw in (2, 4, 8, 16)} | set(args.caps), reverse=True)
    st = torch.cuda.current_stream()
    out = {"workload": "device-resident parity update, one changed block per stripe; medians of %d alternating "
                       "rounds of %d launches back to back, ranges of single-round ratios"
                       % (args.rounds, args.launches),
           "device": torch.cuda.get_device_name(0), "grid_caps": args.caps,
           "units_per_wave_of_caps": {str(c): round(args.nstripes * (SZ // 1024) / (4.0 * c), 2) for c in args.caps}}
    k, m = 3, 10
    code, nums = capi.Code(k, m), list(range(k, m))
    out["kernel"] = same_as_uniform(code, k, nums, st)
    sizes = np.random.default_rng(7).integers(1, SZ + 1, size=args.nstripes, dtype=np.int64)
    caps, args.caps = args.caps, []
    out["a_mixed_3_10_uniform_1_4096"] = mixed_sizes(args, st, code, k, nums, sizes, 20)
    torch.cuda.empty_cache()
    args.caps = caps
    out["b_equal_3_10_4096"] = equal_sizes(args, st, code, k, nums)
    torch.cuda.empty_cache()
    args.caps = []
    k, m = 20, 24
    code, nums = capi.Code(k, m), list(range(k, m))
    out["kernel_wide"] = same_as_uniform(code, k, nums, st)
    wide = np.random.default_rng(9).integers(1, 2**20 + 1, size=args.wide, dtype=np.int64)
    args.by_size = False  # the wide shape: ragged against padded only
    out["c_wide_20_24_uniform_1_1MiB"] = mixed_sizes(args, st, code, k, nums, wide, 40)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
