"""What a round costs with the cold log's host tier demoting every round
(cfg.host_pool_bytes): a C2-shaped engine (every group appends
every round, snapshots off) once with a page pool so small that every page
is demoted as soon as it is committed and no longer its chain's tail (the
plan is launched after every round; the logs of this workload grow in step,
so the moves come in bursts every 64 rounds), once with the default pool and
no tier.
Prints ms/round for both and the bytes that cross the host link per round
(2 KiB per demoted page; reads of demoted pages do not occur in this
workload: nobody falls behind).  The average hides the bursts, so 70 more
rounds are timed one at a time: their median is a round whose plan finds
nothing to move, their maximum the round that moves a page per replica.   python3 scripts/cold_tier_cost.py [groups] [rounds]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dragonboat_amd.engine import Engine  # noqa: E402

PAGE = 2048
groups = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 400
warm = 200  # past the election and the ring: every replica evicts an entry per round
kw = dict(device=0, n_groups=groups, n_replicas=3, wl_enabled=True, wl_start_round=30, ring=64)
n_rep = groups * 3
# a replica gains a page every 64 rounds, all of them within a few rounds of
# each other: 2.25 pages per replica hold every tail and every new page, and
# are more than half full as soon as the new pages exist
small = dict(pool_bytes=n_rep * PAGE * 9 // 4,
             host_pool_bytes=(4 + (warm + rounds) // 64) * n_rep * PAGE)


def timed(**extra):
    eng = Engine(**kw, **extra)
    eng.run(warm)
    c0 = eng.cold_tier_stats()
    ms = eng.run_timed(rounds)
    c1 = eng.cold_tier_stats()
    singles = sorted(eng.run_timed(1) for _ in range(70))  # (one page boundary at least)
    n, bits = eng.fault_summary()
    st = eng.spill_stats()
    eng.close()
    return dict(ms_per_round=ms / rounds, faults=n, oom=st["oom"],
                hbm_pages_used=st["pool_pages_used"], hbm_pages=st["pool_pages"],
                host_pages_used=c1["host_pages_used"],
                demoted=c1["demoted"] - c0["demoted"], passes=c1["passes"] - c0["passes"],
                single_round_median_ms=singles[len(singles) // 2], single_round_max_ms=singles[-1],
                single_round_next_ms=singles[-2])


base = timed()
tier = timed(**small)
print(json.dumps(dict(groups=groups, rounds=rounds, default_pool=base, tiered=tier,
                      link_bytes_per_round=tier["demoted"] * PAGE / rounds,
                      ms_per_round_default=base["ms_per_round"],
                      ms_per_round_tiered=tier["ms_per_round"])))
