#!/bin/bash
# A/B: the default library against build/ variants, split and fused pipelines.
set -e
cd "$GRAFT_REPO_ROOT"
export BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
for lib in dragonboat_amd/libdragonboat_amd.so ${LIBS}; do
  for mode in ${MODES:-split fused}; do
    for w in ${WORKLOADS:-c4 c2m}; do
      RBE_LIB=$PWD/$lib RBE_MODE=$mode timeout 200 python bench.py --full --workload $w --no-cpu-baseline --also "" --steps 100 --warmup 10 > $BENCH_OUT/ab.json 2>$BENCH_OUT/ab.err
      python3 scripts/summarize_bench.py $BENCH_OUT/ab.json "$(basename $lib) $mode $w" | head -1
    done
  done
done
