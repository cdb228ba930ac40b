"""What a call of rbe_collect_dropped costs (DESIGN.md §5 "The dropped lists")
next to rbe_collect_outputs over the same range, whose pipeline has the same
shape: on a fresh host-driven engine (cfg.drop_lists) every replica is a
follower without a leader, so a proposal batch and a ReadIndex pushed to about
1% of the replicas are dropped whole by the next step.  Both calls are then
timed on that engine and round with a host clock (each ends in a stream
synchronisation): `reps` warmed calls each, alternating; median, minimum and
maximum, and the ratio of the medians, as one JSON line.
    python3 scripts/collect_dropped_cost.py [groups] [reps]"""
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

groups = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    from dragonboat_amd.engine import Engine, RbeDroppedList, RbeOutputs
    eng = Engine(device=0, n_groups=groups, n_replicas=3, ext_inputs=True, drop_lists=True,
                 in_cap=1 << 17)
    rng = random.Random(1)
    reps_at = sorted(rng.sample(range(eng.n_rep), max(1, eng.n_rep // 100)))
    eng.push_proposals(reps_at, [[(0, r.to_bytes(8, "little"))] * (1 + r % 3) for r in reps_at])
    eng.push_read_index(reps_at, [(r + 1, 7) for r in reps_at])
    eng.step()
    dl, out = RbeDroppedList(), RbeOutputs()

    def dropped():
        assert eng.lib.rbe_collect_dropped(eng.h, 0, eng.n_rep, 0, C.byref(dl)) == 0

    def outputs():
        assert eng.lib.rbe_collect_outputs(eng.h, 0, eng.n_rep, C.byref(out)) == 0

    for _ in range(3):  # warm both buffer sets
        dropped()
        outputs()
    t = {"dropped": [], "outputs": []}
    for _ in range(reps):
        t["dropped"].append(timed(dropped))
        t["outputs"].append(timed(outputs))
    res = dict(groups=groups, replicas=eng.n_rep, listed=int(dl.n), entries=int(dl.n_entries),
               read_indexes=int(dl.n_read_indexes))
    for k, v in t.items():
        v.sort()
        res[k + "_ms"] = dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4),
                              max=round(v[-1], 4))
    res["ratio"] = round(res["dropped_ms"]["median"] / res["outputs_ms"]["median"], 3)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
