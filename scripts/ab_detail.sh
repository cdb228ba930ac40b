#!/bin/bash
# A/B with the per-kernel split printed (diagnostic builds under build/).
set -e
cd "$GRAFT_REPO_ROOT"
export BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
for lib in dragonboat_amd/libdragonboat_amd.so ${LIBS}; do
  for w in ${WORKLOADS:-c4}; do
    RBE_LIB=$PWD/$lib RBE_MODE=${MODE:-split} timeout 200 python bench.py --full --workload $w --no-cpu-baseline --steps 100 --warmup 10 > $BENCH_OUT/ab.json 2>$BENCH_OUT/ab.err
    python3 scripts/summarize_bench.py $BENCH_OUT/ab.json "$(basename $lib) $w"
  done
done
