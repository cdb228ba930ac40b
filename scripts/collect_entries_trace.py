"""The collection kernels under a kernel trace, k_ce_entries in its two store
forms (DESIGN.md §5 "The Updates' entries"): C2 at 100k x 3, four engines in
turn (RBE_COLLECT_STAGE = 1, 0, 1, 0), each warmed up and then collecting both
lists after each of 20 rounds; the trace names k_ce_entries<true> (staged in
LDS) and k_ce_entries<false> (a lane per record).
    rocprofv3 --kernel-trace --stats -d OUT -- python3 scripts/collect_entries_trace.py"""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragonboat_amd.engine import Engine, RbeEntryList, RBE_ENTRIES_TO_SAVE, RBE_ENTRIES_COMMITTED
for rep in range(2):
    for stage in ("1", "0"):
        os.environ["RBE_COLLECT_STAGE"] = stage
        eng = Engine(device=0, n_groups=100_000, n_replicas=3, wl_enabled=True, wl_start_round=30, ring=64)
        eng.run(120)
        lst = RbeEntryList()
        for _ in range(20):
            eng.step()
            for f in (RBE_ENTRIES_TO_SAVE, RBE_ENTRIES_COMMITTED):
                assert eng.lib.rbe_collect_entries(eng.h, 0, eng.n_rep, f, C.byref(lst)) == 0
        print(stage, lst.n, lst.n_entries, flush=True)
        eng.close()
