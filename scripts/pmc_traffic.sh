#!/bin/bash
# HBM traffic per pipeline kernel from PMC counters: one rocprofv3 pass per
# counter (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950), each
# under its own hard time limit, then scripts/pmc_traffic.py folds them into
# profiles/traffic_<workload>.json.
set -e
cd "$GRAFT_REPO_ROOT"
export BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
export TMPDIR=/tmp
for w in ${WORKLOADS:-c4 c2m}; do
  for ctr in FETCH_SIZE WRITE_SIZE; do
    timeout -s KILL 120 rocprofv3 --pmc $ctr -d $BENCH_OUT/pmc_${w}_$ctr -o run --output-format csv -- python3 bench.py --full --workload $w --steps 10 --warmup 2 --prof-rounds 10 --no-cpu-baseline --also "" > $BENCH_OUT/pmc_${w}_$ctr.log 2>&1
  done
  # request counts (the store audit): TCP->TCC write / read requests
  timeout -s KILL 120 rocprofv3 --pmc TCP_TCC_WRITE_REQ_sum TCP_TCC_READ_REQ_sum -d $BENCH_OUT/pmc_${w}_REQ -o run --output-format csv -- python3 bench.py --full --workload $w --steps 10 --warmup 2 --prof-rounds 10 --no-cpu-baseline --also "" > $BENCH_OUT/pmc_${w}_REQ.log 2>&1
  python3 scripts/pmc_traffic.py $w $BENCH_OUT/pmc_${w}_FETCH_SIZE $BENCH_OUT/pmc_${w}_WRITE_SIZE $BENCH_OUT/pmc_${w}_REQ
done
