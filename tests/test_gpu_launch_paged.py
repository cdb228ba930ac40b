"""The paged rbe_launch on the HIP engine (tests/test_launch_paged.py is the
CPU tier): k_launch_release / k_launch_alloc / k_launch_fill build the cold
part of the launched LogDBs a page per wave, in host pages with
cfg.host_pool_bytes, and k_relaunch installs the chains.  A tiered engine whose
logs have outgrown its HBM pool restarts whole (240 pages against a 127-page
pool), and an engine without a tier restarts inside the pool that held its
logs.

The oracle's side of each scenario (views after every round, the launch
batch, counters and a few entries at the end) is computed once and shared."""
import pytest

import oracle as O
from collect_scenarios import by_replica
from launch_util import restart
from parity_util import counters_match, view_diff
from test_gpu_cold_tier import C2_SMALL, C2_TIER

pytestmark = pytest.mark.gpu

RING = 8
N_REP = 48
_ORACLE = {}


class _Batch:
    """Takes the place of an engine in launch_util.restart: keeps the batch."""

    def launch(self, replicas, states, entries):
        self.args = (list(replicas), list(states), list(entries))


def scenario(at, picks, after):
    """The oracle run `at` rounds, restarted (`picks`: "all", or "followers" =
    one follower per group) over whole LogDBs, and run `after` more rounds."""
    key = (at, picks, after)
    if key not in _ORACLE:
        ref = O.Harness(trace=True, **C2_SMALL)
        views = []
        for _ in range(at):
            ref.run(1)
            views.append(ref.views())
        if picks == "all":
            reps = list(range(N_REP))
        else:
            reps = [next(r for r in range(3 * g, 3 * g + 3) if views[-1][r].role != O.LEADER)
                    for g in range(N_REP // 3)]
        batch = _Batch()
        restart(batch, ref, reps, None)
        for _ in range(after):
            ref.run(1)
            views.append(ref.views())
        ents = {r: [(e.index, e.term) for e in ref.persisted_entries(r, 1, 40)]
                for r in (0, 1, 24, 47)}
        _ORACLE[key] = dict(views=views, batch=batch.args, counters=ref.counters(), entries=ents)
    return _ORACLE[key]


def lockstep(eng, ref, first, last, every=1):
    done = first
    while done < last:
        k = min(every, last - done)
        eng.run(k)
        done += k
        ev, hv = eng.views(), ref["views"][done - 1]
        for i in range(len(hv)):
            d = view_diff(ev[i], hv[i])
            assert d is None, f"first divergence at round {done}, replica {i}: {d}"


def cold_pages(last):
    return (last - RING) // 64 + 1 if last > RING else 0


def view_pages(views):
    return sum(cold_pages(v.last_index) for v in views)


def no_fault(eng):
    n, bits = eng.fault_summary()
    assert n == 0, f"{n} replicas faulted ({bits:#x})"
    assert eng.spill_stats()["oom"] == 0


@pytest.mark.parametrize("mode", ["stepped", "graph20"])
def test_gpu_tiered_whole_node_restart(gpu_available, mode):
    """16 x 3, a 127-page pool over a 1024-page tier, round 300: the 48 logs
    hold 240 cold pages.  All 48 restart over their whole LogDBs: one tail
    each in HBM, the rest in host pages; then 120 rounds in lockstep, stepped
    or 20 rounds per graph replay (with the demotion kernels)."""
    from dragonboat_amd.engine import Engine
    ref = scenario(300, "all", 120)
    every = 20 if mode == "graph20" else 1
    eng = Engine(device=0, trace=True, **C2_TIER, **C2_SMALL)
    lockstep(eng, ref, 0, 300, every=every)
    eng.launch(*ref["batch"])
    total = view_pages(ref["views"][299])
    assert total == 240
    no_fault(eng)
    assert eng.spill_stats()["pool_pages_used"] == N_REP
    assert eng.cold_tier_stats()["host_pages_used"] == total - N_REP
    lockstep(eng, ref, 300, 420, every=every)
    no_fault(eng)
    bad = counters_match(eng.counters(), ref["counters"])
    assert not bad, f"counters differ {bad}"
    for r, want in ref["entries"].items():  # read out of host pages
        assert [(x[0], x[1]) for x in eng.entries(r, 1, 40)] == want, r
    eng.close()


def test_gpu_launch_reuses_what_it_releases(gpu_available):
    """No tier, a 127-page pool, round 120: 96 pages in use, and a restart of
    all 48 replicas needs them again (the per-entry launch left 33 replicas
    with F_NOMEM).  Lockstep to round 150; the third page per replica, near
    round 163, is past what this pool holds."""
    from dragonboat_amd.engine import Engine
    ref = scenario(120, "all", 30)
    eng = Engine(device=0, trace=True, ring=RING, pool_bytes=256 << 10, **C2_SMALL)
    lockstep(eng, ref, 0, 120)
    assert eng.spill_stats()["pool_pages_used"] == view_pages(ref["views"][119]) == 96
    eng.launch(*ref["batch"])
    no_fault(eng)
    assert eng.spill_stats()["pool_pages_used"] == 96
    lockstep(eng, ref, 120, 150)
    no_fault(eng)
    bad = counters_match(eng.counters(), ref["counters"])
    assert not bad, f"counters differ {bad}"
    eng.close()


def test_gpu_tiered_partial_batch(gpu_available):
    """One follower per group restarts at round 300: its pages go back (host
    pages through the host tier's stack) and its chain is rebuilt with the
    tail in HBM; both tiers together hold what the views say."""
    from dragonboat_amd.engine import Engine
    ref = scenario(300, "followers", 60)
    eng = Engine(device=0, trace=True, **C2_TIER, **C2_SMALL)
    lockstep(eng, ref, 0, 300, every=20)
    before = eng.spill_stats()["pool_pages_used"] + eng.cold_tier_stats()["host_pages_used"]
    assert before == view_pages(ref["views"][299])
    eng.launch(*ref["batch"])
    no_fault(eng)
    st, ct = eng.spill_stats(), eng.cold_tier_stats()
    assert st["pool_pages_used"] + ct["host_pages_used"] == before
    assert st["pool_pages_used"] >= N_REP  # (a tail per replica at least)
    lockstep(eng, ref, 300, 360)
    no_fault(eng)
    st, ct = eng.spill_stats(), eng.cold_tier_stats()
    assert st["pool_pages_used"] + ct["host_pages_used"] == view_pages(ref["views"][359])
    bad = counters_match(eng.counters(), ref["counters"])
    assert not bad, f"counters differ {bad}"
    eng.close()


def test_gpu_paged_launch_read_by_collect(gpu_available):
    """rbe_collect_entry_ranges (k_ce_entries) over every replica's whole log,
    pages the launch wrote in both tiers, equals the LogDBs handed over."""
    from dragonboat_amd.engine import Engine
    ref = scenario(300, "all", 120)
    eng = Engine(device=0, trace=True, **C2_TIER, **C2_SMALL)
    eng.run(300)
    reps, states, entries = ref["batch"]
    eng.launch(reps, states, entries)
    no_fault(eng)
    got = by_replica(eng.collect_entry_ranges(reps, [1] * len(reps), [s[3] for s in states]))
    for r, st, want in zip(reps, states, entries):
        assert len(want) == st[3]
        mine = [(e["index"], e["term"], e["type"], e["cmd"]) for e in got[r]]
        assert mine == [tuple(e) for e in want], r
    eng.close()
