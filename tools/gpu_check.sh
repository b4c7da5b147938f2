#!/bin/bash
# One GPU-box session: parity tests, smoke, a short bench, and a kernel-trace profile.
# Every GPU step has its own time limit; the first failure ends the script.
# Run from the repository root; results go to $OUT (default bench_out/).
set -e
export TMPDIR=/tmp
ROOT=$(pwd)
OUT=${OUT:-$ROOT/bench_out}
mkdir -p $OUT
rocm-smi --showproductname > $OUT/smi.txt 2>&1 || true
timeout -k 10 600 python -m pytest tests -x -q -m gpu > $OUT/pytest_gpu.log 2>&1
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
timeout -k 10 300 python bench.py --full --steps 50 --warmup 5 --cpu-seconds 8 > $OUT/bench.log 2>&1
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run -- python3 $ROOT/bench.py --full --steps 20 --warmup 3 --no-cpu > $OUT/prof.log 2>&1
echo done
