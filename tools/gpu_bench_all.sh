#!/bin/bash
# GPU tests + every bench workload; each GPU step has its own limit, first failure stops.
# Run from the repository root; results go to $OUT (default bench_out/).
set -e
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests -x -q -m gpu > $OUT/pytest_gpu.log 2>&1
timeout -k 10 300 python bench.py --full --cpu-seconds 5 > $OUT/bench_cfg2.log 2>&1
timeout -k 10 300 python bench.py --full --workload cfg3 --steps 20 --cpu-seconds 5 > $OUT/bench_cfg3.log 2>&1
timeout -k 10 300 python bench.py --full --workload cfg4 --steps 20 --cpu-seconds 5 > $OUT/bench_cfg4.log 2>&1
timeout -k 10 300 python bench.py --full --workload cfg5 --steps 10 --cpu-seconds 5 > $OUT/bench_cfg5.log 2>&1
echo all-done
