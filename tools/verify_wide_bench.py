#!/usr/bin/env python3
"""The fused wide-code verify (matverify_bsr) against the two-step path
(expected rows into scratch, then rows_differ), on fec_verify_batch itself.
Method of tools/verify_bench.py: device-resident, cold -- launches back to back
between two events, rotating over buffer sets that together exceed twice the
256 MiB Infinity Cache -- and every leg's masks checked after timing.

The baseline is the parent commit's fec_verify_batch.  This tree runs the
parent's path unchanged under ZFEC_HIP_VERIFY_FUSED_MIN=4294967295, so:
  1. --parent-lib (the parent's libzfec_hip.so, built side by side:
     `git worktree add ../parent HEAD~1 && make -C ../parent`, copied to
     abuild/parent/) is timed against this tree with the knob off on the
     K=10/M=16 64 x 4 MiB leg, in alternating process rounds;
  2. every leg is then timed in one process, alternating per round between the
     default path (fused) and the knob (two-step), which removes the
     process-to-process noise.
Legs: K=10/M=16 on 64 x 4 MiB and K=20/M=60 (40 checks) on 64 x 1 MiB, clean
and with 1 % of the stripes corrupted in one byte; K=10/M=16 at 4 KiB blocks
with 16, 64, 256 and 1024 units (the threshold; fused forced with the knob at
1).  Medians of --rounds rounds and the range of single-round ratios.
Writes profiles/verify_wide_bench.json.

    python tools/verify_wide_bench.py [--rounds 9] [--launches 10] [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOB = "ZFEC_HIP_VERIFY_FUSED_MIN"
OFF = "4294967295"
COLD_BYTES = 3 << 28  # 768 MiB of blocks in rotation per leg (at least two sets)

LARGE = [("k10_m16_64x4MiB", 10, 16, 4 << 20, 64), ("k20_m60_64x1MiB", 20, 60, 1 << 20, 64)]
SMALL_UNITS = (16, 64, 256, 1024)  # K=10/M=16, 4 KiB blocks: two units per stripe


def setup(k, m, sz, ns, frac, g):
    """Buffer sets of ns stripes [ns, m, sz] (COLD_BYTES in all, at least two),
    a fraction of each set's stripes corrupted; returns (sets, masks, want)."""
    import torch
    from zfec_amd import capi
    code = capi.Code(k, m)
    nsets = max(2, -(-COLD_BYTES // (ns * m * sz)))
    a = torch.empty((ns, m, sz), dtype=torch.uint8, device="cuda")
    a[:, :k] = torch.randint(0, 256, (ns, k, sz), dtype=torch.uint8, device="cuda", generator=g)
    code.encode_batch(a.data_ptr(), sz, m * sz, a.data_ptr() + k * sz, sz, m * sz, list(range(k, m)), sz, ns,
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pool = torch.empty((nsets, ns, m, sz), dtype=torch.uint8, device="cuda")
    pool[:] = a
    del a
    c = m - k
    want = []
    for i in range(nsets):
        w = torch.zeros((ns, c), dtype=torch.bool, device="cuda")
        if frac:
            n = max(1, int(ns * frac))
            rows = torch.randperm(ns, device="cuda", generator=g)[:n]
            slot = torch.randint(0, m, (n,), device="cuda", generator=g)
            pos = torch.randint(0, sz, (n,), device="cuda", generator=g)
            pool[i][rows, slot, pos] ^= 0x5A
            w[rows] = torch.where((slot < k)[:, None], torch.ones(1, dtype=torch.bool, device="cuda"),
                                  (slot - k)[:, None] == torch.arange(c, device="cuda")[None, :])
        want.append(w)
    words = (c + 31) // 32
    masks = torch.full((nsets, ns, words), -1, dtype=torch.int32, device="cuda")
    return code, pool, masks, want


def unpack(mask, c):
    import torch
    shifts = torch.arange(32, dtype=torch.int32, device=mask.device)
    bits = (mask.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(mask.shape[0], -1)[:, :c].ne(0)


def time_leg(name, k, m, sz, ns, frac, variants, rounds, launches, g):
    """variants: name -> knob value (None: unset).  Alternates the variants
    within each round; returns per-variant lists of ms and the kernels seen."""
    import torch
    import bench
    from zfec_amd import capi
    st = torch.cuda.current_stream()
    code, pool, masks, want = setup(k, m, sz, ns, frac, g)
    nums = list(range(m))
    c = m - k

    def ver(i):
        def f(sh):
            code.verify_batch(pool[i].data_ptr(), sz, m * sz, nums, sz, ns, masks[i].data_ptr(), stream=sh)
        return f

    fns = [ver(i) for i in range(pool.shape[0])]
    n = max(launches, min(len(fns), 256))
    ms = {v: [] for v in variants}
    kern = {}
    for _ in range(rounds):
        for v, val in variants.items():
            if val is None:
                os.environ.pop(KNOB, None)
            else:
                os.environ[KNOB] = val
            capi.reload_config()
            t, _ = bench.back_to_back(fns, n, st, "%s %s" % (name, v))
            kern[v] = capi.last_kernel_name()
            ms[v].append(t)
            masks.fill_(-1)
            for i in (0, len(fns) - 1):  # checked after timing, outside the events
                fns[i](st.cuda_stream)
                torch.cuda.synchronize()
                assert torch.equal(unpack(masks[i], c), want[i]), (name, v, "masks are not the known corruption")
    os.environ.pop(KNOB, None)
    capi.reload_config()
    del pool, masks
    torch.cuda.empty_cache()
    return ms, kern


def summary(ms, new, base, moved):
    r = [a / b for a, b in zip(ms[new], ms[base])]
    mn, mb = statistics.median(ms[new]), statistics.median(ms[base])
    return {"ms": {new: round(mn, 4), base: round(mb, 4)},
            "GBps_of_k_plus_c": {new: round(moved / mn / 1e6, 1), base: round(moved / mb / 1e6, 1)},
            "ratio_median": round(statistics.median(r), 4), "ratio_range": [round(min(r), 4), round(max(r), 4)],
            "rounds_ms": {v: [round(x, 4) for x in xs] for v, xs in ms.items()}}


def worker(args):
    """One process: --legs parent-check (the K=10/M=16 leg with the knob off,
    whatever library ZFEC_HIP_LIB names) or all (every leg, fused against two-step)."""
    import torch
    assert torch.cuda.is_available(), "verify_wide_bench.py measures on a GPU"
    g = torch.Generator(device="cuda").manual_seed(11)
    out = {}
    if args.legs == "parent-check":
        name, k, m, sz, ns = LARGE[0]
        ms, kern = time_leg(name, k, m, sz, ns, 0.0, {"only": OFF}, args.rounds, args.launches, g)
        out[name] = {"ms": ms["only"], "kernel": kern["only"]}
    else:
        for name, k, m, sz, ns in LARGE:
            for tag, frac in (("clean", 0.0), ("1pct_corrupt", 0.01)):
                ms, kern = time_leg(name, k, m, sz, ns, frac, {"fused": None, "two_step": OFF}, args.rounds,
                                    args.launches, g)
                out["%s_%s" % (name, tag)] = dict(summary(ms, "fused", "two_step", ns * m * sz), kernels=kern)
                print(name, tag, "done", file=sys.stderr, flush=True)
        for units in SMALL_UNITS:
            ns = units // 2
            ms, kern = time_leg("k10_m16_4KiB", 10, 16, 4096, ns, 0.0, {"fused": "1", "two_step": OFF}, args.rounds,
                                args.launches, g)
            out["k10_m16_4KiB_%dunits" % units] = dict(summary(ms, "fused", "two_step", ns * 16 * 4096), kernels=kern)
            print(units, "units done", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "legs": out}))


def run_worker(legs, rounds, launches, lib=None):
    env = dict(os.environ)
    env.pop(KNOB, None)
    if lib:
        env["ZFEC_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--legs", legs, "--rounds", str(rounds),
                        "--launches", str(launches)], env=env, check=True, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "abuild", "parent", "libzfec_hip.so"))
    ap.add_argument("--parent-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_wide_bench.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--legs", default="all")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # (this process never opens the GPU: every measurement is a child process)
    out = {"device": None,
           "timing": "launches back to back between events, rotating over >= 768 MiB of buffer sets (cold); "
                     "fused = this tree's default (threshold legs: %s=1), two_step = %s=%s" % (KNOB, KNOB, OFF)}
    if os.path.exists(args.parent_lib):
        # alternating process rounds: the parent's library, then this tree with the knob off
        par, own = [], []
        for _ in range(args.parent_rounds):
            par += run_worker("parent-check", 1, args.launches, args.parent_lib)["legs"][LARGE[0][0]]["ms"]
            own += run_worker("parent-check", 1, args.launches)["legs"][LARGE[0][0]]["ms"]
        r = [a / b for a, b in zip(own, par)]
        out["parent_check_k10_m16_64x4MiB"] = {
            "what": "parent commit's libzfec_hip.so against this tree with the knob off, one process each per round",
            "ms_parent": [round(x, 4) for x in par], "ms_this_tree_knob_off": [round(x, 4) for x in own],
            "median_ms": {"parent": round(statistics.median(par), 4), "this_tree_knob_off": round(statistics.median(own), 4)},
            "ratio_range": [round(min(r), 4), round(max(r), 4)], "ratio_median": round(statistics.median(r), 4)}
    else:
        out["parent_check_k10_m16_64x4MiB"] = "not run: %s is missing" % os.path.relpath(args.parent_lib, ROOT)
    res = run_worker("all", args.rounds, args.launches)
    out["device"], out["legs"] = res["device"], res["legs"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
