#!/usr/bin/env python3
"""Interleaved A/B of library variants (tools/ab_build.sh builds them into
abuild/<name>/) on the headline: plain `bench.py --steps N` runs, each its own
process loading its variant through ZFEC_HIP_LIB, in A B C .. A B C .. order on
one box.

The gate (--gate BASE,NEW): NEW's median `value` must exceed BASE's median by
more than BASE's own max - min over its runs.

Optional per variant, after the rounds: one --full run (per-kernel encode and
decode times, cold and warm; CPU and extra legs off) and one --dump-outputs run
whose parity.npy / recovered.npy must be byte-identical across the variants.

    python tools/ab_bench.py --variants par,new,notp --rounds 5 --steps 200 \\
        --gate par,new --full --dump --out bench_out/ab_bench.json
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(variant, extra, timeout):
    env = dict(os.environ)
    if variant != "tree":
        env["ZFEC_HIP_LIB"] = os.path.join(ROOT, "abuild", variant, "libzfec_hip.so")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, env=env,
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or len(lines) != 1:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        raise SystemExit("variant %s failed (rc %d)" % (variant, p.returncode))  # nothing more runs after a failure
    return json.loads(lines[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", required=True, help="names under abuild/ (or 'tree': the in-tree library)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gate", default=None, help="BASE,NEW")
    ap.add_argument("--full", action="store_true", help="one --full run per variant after the rounds")
    ap.add_argument("--dump", action="store_true", help="one --dump-outputs run per variant; outputs must be identical")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    variants = args.variants.split(",")
    plain = ["--steps", str(args.steps), "--warmup", str(args.warmup)]
    runs = {v: [] for v in variants}
    for rnd in range(args.rounds):
        for v in variants:
            r = run_bench(v, plain, 300)
            runs[v].append({"value": r["value"], "ms_per_step": r["ms_per_step"]})
            print("round %d %-6s value %.2f  ms/step %.4f  %s" % (rnd, v, r["value"], r["ms_per_step"],
                                                                r.get("kernels")), flush=True)
    doc = {"tool": "tools/ab_bench.py (variants: tools/ab_build.sh)", "order": "interleaved, one process per run",
           "bench": "bench.py --gpus 1 " + " ".join(plain), "unit": "GB/s", "variants": {}}
    for v in variants:
        vals = [x["value"] for x in runs[v]]
        spec = os.path.join(ROOT, "abuild", v, "SPEC")
        doc["variants"][v] = {"spec": open(spec).read().strip() if os.path.exists(spec) else "in-tree build",
                              "runs": runs[v], "median": round(statistics.median(vals), 2), "min": min(vals),
                              "max": max(vals), "spread": round(max(vals) - min(vals), 2)}
    if args.gate:
        base, new = args.gate.split(",")
        b, n = doc["variants"][base], doc["variants"][new]
        gain = round(n["median"] - b["median"], 2)
        doc["gate"] = {"base": base, "new": new, "gain_of_medians": gain, "base_spread": b["spread"],
                       "gain_pct": round(100.0 * gain / b["median"], 2), "passed": gain > b["spread"],
                       "rule": "new median - base median > base max - min"}
    if args.full:
        for v in variants:
            r = run_bench(v, plain + ["--full", "--no-cpu", "--no-extra", "--no-first-seen"], 600)
            roof, dec = r.get("roofline") or {}, r.get("decode_roofline") or {}
            doc["variants"][v]["full"] = {
                "value": r["value"], "kernels": r.get("kernels"),
                "encode_us_cold": roof.get("launch_ms") and round(roof["launch_ms"] * 1e3, 2),
                "encode_us_warm": roof.get("launch_ms_warm") and round(roof["launch_ms_warm"] * 1e3, 2),
                "decode_us_cold": dec.get("launch_ms") and round(dec["launch_ms"] * 1e3, 2),
                "decode_us_warm": dec.get("launch_ms_warm") and round(dec["launch_ms_warm"] * 1e3, 2)}
            print("full  %-6s %s" % (v, json.dumps(doc["variants"][v]["full"])), flush=True)
    if args.dump:
        sums = {}
        for v in variants:
            with tempfile.TemporaryDirectory() as d:
                run_bench(v, ["--steps", "4", "--warmup", "1", "--dump-outputs", d], 300)
                sums[v] = {n: hashlib.sha256(open(os.path.join(d, n), "rb").read()).hexdigest()
                           for n in ("parity.npy", "recovered.npy")}
        same = all(sums[v] == sums[variants[0]] for v in variants)
        doc["dump_outputs"] = {"sha256": sums, "identical": same}
        print("dump-outputs identical: %s" % same, flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    if args.dump and not doc["dump_outputs"]["identical"]:
        raise SystemExit("outputs differ between variants")


if __name__ == "__main__":
    main()
