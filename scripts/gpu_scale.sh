#!/bin/bash
# Size sweep of one workload: per-kernel time vs groups (latency- vs throughput-bound).
set -e
cd "$GRAFT_REPO_ROOT"
export BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
w=${WORKLOAD:-c4}
for g in ${SIZES:-125000 250000 500000 1000000 2000000 4000000}; do
  timeout -k 10 200 python -u bench.py --full --steps 50 --warmup 10 --workload $w --groups $g --no-cpu-baseline > $BENCH_OUT/scale_${w}_$g.json 2> $BENCH_OUT/scale_${w}_$g.err
  python3 scripts/summarize_bench.py $BENCH_OUT/scale_${w}_$g.json ${w}_$g
done
