#!/usr/bin/env python3
"""The register table of kernels.hip's kernels from the amdhsa.kernels metadata
of a device-only assembly (the Makefile's HIPFLAGS plus --cuda-device-only
-S): per kernel its vgpr_count, sgpr_count, private_segment_fixed_size
(scratch), sgpr_spill_count and vgpr_spill_count.  Metadata only; no
instruction is read.

--match REGEX (default "ragged") names the kernels a change is about; the table
holds those.  With two files the second is checked against the first:

  * a matched kernel: no scratch, no VGPR spill, no fewer waves per SIMD
    (512 / (8 * ceil(vgpr / 8))), no more SGPR spills;
  * every other kernel: all five numbers unchanged.

The exit status says whether all hold.

    python tools/kernel_regs.py parent.s [this.s] [--match REGEX] [--out profiles/NAME.json]
"""
import argparse
import json
import re
import subprocess
import sys

KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def table(path):
    """kernel name (template arguments as numbers) -> the five numbers, for every kernel."""
    recs, cur = [], None
    with open(path) as f:
        for line in f:
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
            if not m:
                continue
            key, val = m.groups()
            if key == "name" and val.startswith("_Z"):
                cur = {"name": val}
                recs.append(cur)
            elif cur is not None and key in KEYS:
                cur[key] = int(val)
    recs = [r for r in recs if all(k in r for k in KEYS)]
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in recs), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    out = {}
    for r, n in zip(recs, names):
        # "void zfec_hip::(anonymous namespace)::matapply_ragged<3, 7>(...)" -> "matapply_ragged<3,7>"
        short = re.sub(r"^void |zfec_hip::|\(anonymous namespace\)::", "", n).split("(")[0].replace(" ", "")
        out[short] = [r[k] for k in KEYS]
    return out


def waves(vgpr):
    return 512 // (8 * ((vgpr + 7) // 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this", nargs="?")
    ap.add_argument("--match", default="ragged", help="regex (re.search) of the kernels the change is about")
    ap.add_argument("--out")
    args = ap.parse_args()
    hit = re.compile(args.match).search
    every = table(args.parent)
    parent = {n: v for n, v in every.items() if hit(n)}
    res = {"columns": list(KEYS), "match": args.match, "parent": parent}
    bad = 0
    if args.this:
        every_this = table(args.this)
        this = res["this"] = {n: v for n, v in every_this.items() if hit(n)}
        if sorted(every_this) != sorted(every):
            print("kernel lists differ:", sorted(set(every_this) ^ set(every)))
            bad += 1
        for n in sorted(set(this) & set(parent)):
            p, t = parent[n], this[n]
            broke = t[2] != 0 or t[4] != 0 or waves(t[0]) < waves(p[0]) or t[3] > p[3]
            bad += broke
            if p != t:
                print("%-28s %s -> %s%s" % (n, p, t, "  BROKEN" if broke else ""))
        print("%d kernels match, %d changed, %d break a condition" %
              (len(this), sum(parent.get(n) != this[n] for n in this), bad))
        moved = sorted(n for n in set(every) & set(every_this) if not hit(n) and every[n] != every_this[n])
        for n in moved:
            print("%-28s %s -> %s  OUTSIDE THE MATCH" % (n, every[n], every_this[n]))
        print("%d other kernels, %d moved" % (len(every_this) - len(this), len(moved)))
        bad += len(moved)
        res["others"] = {"kernels": len(every_this) - len(this), "moved": moved}
    else:
        for n in sorted(parent):
            print("%-28s %s" % (n, parent[n]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=0, sort_keys=True)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
