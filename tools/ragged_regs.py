#!/usr/bin/env python3
"""The register table of the ragged kernels from the amdhsa.kernels metadata
of a device-only assembly of kernels.hip (the Makefile's HIPFLAGS plus
--cuda-device-only -S): for every kernel whose name contains "ragged" its
vgpr_count, sgpr_count, private_segment_fixed_size (scratch), sgpr_spill_count
and vgpr_spill_count.  Metadata only; no instruction is read.

With two files it also checks the second against the first, per kernel: no
scratch, no VGPR spill, no fewer waves per SIMD (512 / (8 * ceil(vgpr / 8))),
no more SGPR spills; the exit status says whether all hold.

    python tools/ragged_regs.py parent.s [this.s] [--out profiles/ragged_walk_regs.json]
"""
import argparse
import json
import re
import subprocess
import sys

KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def table(path):
    """kernel name (template arguments as numbers) -> the five numbers."""
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
    recs = [r for r in recs if "ragged" in r["name"] and all(k in r for k in KEYS)]
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
    ap.add_argument("--out")
    args = ap.parse_args()
    parent = table(args.parent)
    res = {"columns": list(KEYS), "parent": parent}
    bad = 0
    if args.this:
        this = res["this"] = table(args.this)
        if sorted(this) != sorted(parent):
            print("kernel lists differ:", sorted(set(this) ^ set(parent)))
            bad += 1
        for n in sorted(set(this) & set(parent)):
            p, t = parent[n], this[n]
            broke = t[2] != 0 or t[4] != 0 or waves(t[0]) < waves(p[0]) or t[3] > p[3]
            bad += broke
            if p != t:
                print("%-28s %s -> %s%s" % (n, p, t, "  BROKEN" if broke else ""))
        print("%d kernels, %d changed, %d break a condition" %
              (len(this), sum(parent.get(n) != this[n] for n in this), bad))
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
