#!/bin/bash
# What bounds k_full_list on C3: SQ wait / issue / instruction-mix counters over
# 60 profiled rounds (isolation epochs included), two passes.
set -e
cd "$GRAFT_REPO_ROOT"
export BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
export TMPDIR=/tmp
timeout -s KILL 150 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR -d $BENCH_OUT/pmcfull1 -o run --output-format csv -- python3 bench.py --full --workload c3 --steps 60 --warmup 2 --prof-rounds 60 --no-cpu-baseline > $BENCH_OUT/pmcfull1.log 2>&1
echo pass1 ok
timeout -s KILL 150 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_BRANCH -d $BENCH_OUT/pmcfull2 -o run --output-format csv -- python3 bench.py --full --workload c3 --steps 60 --warmup 2 --prof-rounds 60 --no-cpu-baseline > $BENCH_OUT/pmcfull2.log 2>&1
echo pass2 ok
