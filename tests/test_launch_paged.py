"""The paged rbe_launch on the CPU tier (tests/launch_cpu: the host build of
the step with the passes of dragonboat_amd/csrc/rbe_launch.h as plain loops,
the same RBE_HD functions the HIP kernels call).  A launch whose LogDBs reach
below the ring plans the cold pages on the host, releases the old chains,
takes an id per page, fills the pages and installs the chains:

  * it builds what the serial per-entry launch (soa_launch) builds, at every
    boundary of the cold range;
  * it reuses what it releases, so a whole-node restart fits the pool that
    held the logs;
  * with a host tier every page but a replica's tail goes to a host page, an
    HBM page when the tier is full;
  * with both tiers full the replicas that miss a page fault alone (F_NOMEM),
    hold no chain and leak no page.

The GPU twins are in test_gpu_launch_paged.py."""
import pytest

import oracle as O
from launch_cpu.launch import LaunchCpu
from launch_util import restart
from parity_util import C2, counters_match, run_lockstep, view_diff

RING = 8
SMALL = dict(n_groups=4, n_replicas=3, ring=RING)
C2_SMALL = dict(C2, n_groups=16)
MB_CC_IN_LOG = 0x02
F_NOMEM = 0x100


def term_of(idx):
    return 1 + (idx > 50) + (idx > 120)


def logdb(last, n, special=None, marker=None):
    """A synthetic LogDB ending at `last` with its n newest entries:
    (state, entries).  special: {index: (type, cmd)}."""
    special = special or {}
    ents = []
    for idx in range(last - n + 1, last + 1):
        typ, cmd = special.get(idx, (0, (idx * 1000003).to_bytes(8, "little")))
        ents.append((idx, term_of(idx), typ, cmd))
    state = (3, 0, last, last)
    if marker is not None:  # compacted: the snapshot sits at the marker
        state += (marker, term_of(marker), marker, term_of(marker))
    return state, ents


def cold_pages(last, n=None):
    """Pages of a log's cold part: entries [last - n + 1, last - RING]."""
    n = last if n is None else n
    if n <= RING:
        return 0
    return (last - RING) // 64 - (last - n + 1) // 64 + 1


# (last, n): n == ring; n == ring + 1; last cold index = 0 and = 63 (mod 64);
# first cold index = 63 and = 0 (mod 64); one page filled at neither end;
# a three-page chain
SHAPES = [(8, 8), (9, 9), (72, 72), (135, 100), (200, 138), (200, 137), (120, 50), (190, 190)]
# descending replicas with replicas without a cold page between the others
ORDER = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
ORDER_SHAPES = [(190, 190), (8, 8), (200, 138), (5, 5), (9, 9), (8, 8), (8, 8), (72, 72),
                (135, 100), (8, 3), (200, 137), (120, 50)]


def both(kw):
    return LaunchCpu(paged=True, trace=True, **kw), LaunchCpu(paged=False, trace=True, **kw)


def same_state(a, b, reps, dbs):
    va, vb = a.views(), b.views()
    for r in range(a.n_rep):
        assert view_diff(va[r], vb[r]) is None, (r, view_diff(va[r], vb[r]))
    for r, (st, ents) in zip(reps, dbs):
        lo, hi = ents[0][0], ents[-1][0]
        got = a.entries(r, lo, hi)
        assert got == b.entries(r, lo, hi), r
        assert got == [tuple(e) for e in ents], r
        assert a.mflags(r) == b.mflags(r), r
        assert [pn for _, pn in a.chain(r)] == [pn for _, pn in b.chain(r)], r
    sa, sb = a.spill_stats(), b.spill_stats()
    assert sa["pool_pages_used"] == sb["pool_pages_used"]
    assert sa["oom"] == 0 and sb["oom"] == 0
    assert a.faults()[0] == 0 and b.faults()[0] == 0


def launch_both(a, b, reps, dbs, one_by_one):
    if one_by_one:
        for r, (st, ents) in zip(reps, dbs):
            a.launch([r], [st], [ents])
            b.launch([r], [st], [ents])
    else:
        for e in (a, b):
            e.launch(reps, [st for st, _ in dbs], [ents for _, ents in dbs])


@pytest.mark.parametrize("one_by_one", [False, True])
@pytest.mark.parametrize("order", ["ascending", "descending_mixed"])
def test_paged_equals_serial_boundaries(order, one_by_one):
    a, b = both(SMALL)
    a.run(3)
    b.run(3)
    if order == "ascending":
        reps, shapes = list(range(len(SHAPES))), SHAPES
    else:
        reps, shapes = ORDER, ORDER_SHAPES
    dbs = [logdb(last, n) for last, n in shapes]
    launch_both(a, b, reps, dbs, one_by_one)
    same_state(a, b, reps, dbs)
    assert a.spill_stats()["pool_pages_used"] == sum(cold_pages(l, n) for l, n in shapes)
    for r, (last, n) in zip(reps, shapes):
        assert len(a.chain(r)) == cold_pages(last, n), r


@pytest.mark.parametrize("one_by_one", [False, True])
def test_paged_equals_serial_compacted(one_by_one):
    """Marker 70, entries 71..200: the first cold index lies in mid-page."""
    kw = dict(SMALL, snapshot_entries=20, compaction_overhead=5)
    a, b = both(kw)
    reps = [4, 1]
    dbs = [logdb(200, 130, marker=70), logdb(150, 80, marker=70)]
    launch_both(a, b, reps, dbs, one_by_one)
    same_state(a, b, reps, dbs)
    assert [pn for _, pn in a.chain(4)] == [1, 2, 3]
    assert a.snapshot_state() == b.snapshot_state()


def test_paged_config_change_in_cold_part():
    """A ConfigChange only below the ring still sets MB_CC_IN_LOG (the flag
    gates the next campaign, raft.go hasConfigChangeToApply)."""
    kw = dict(SMALL, membership=True)
    a, b = both(kw)
    cc = {5: (1, b"\x00" * 16)}
    reps = [2, 6, 7]
    dbs = [logdb(100, 100, special=cc), logdb(100, 100), logdb(8, 8, special=cc)]
    launch_both(a, b, reps, dbs, False)
    same_state(a, b, reps, dbs)
    assert a.mflags(2) & MB_CC_IN_LOG and not a.mflags(6) & MB_CC_IN_LOG
    assert a.mflags(7) & MB_CC_IN_LOG  # (in the ring: relaunch_replica's own loop)


def test_paged_heap_entry_in_cold_slot():
    kw = dict(SMALL, heap_bytes=1 << 20)
    a, b = both(kw)
    big = bytes(range(100))
    dbs = [logdb(150, 150, special={37: (0, big), 149: (0, big[::-1])})]
    launch_both(a, b, [5], dbs, False)
    same_state(a, b, [5], dbs)
    assert a.entries(5, 37, 37)[0][3] == big


def view_pages(views, replicas=None):
    replicas = range(len(views)) if replicas is None else replicas
    return sum(cold_pages(views[r].last_index) for r in replicas)


def lockstep(eng, ref, rounds):
    d = run_lockstep(eng, ref, rounds, every=1)
    assert d is None, f"first divergence {d}"


def test_launch_reuses_what_it_releases():
    """16 x 3, a 127-page pool, round 120: the logs hold 96 pages.  A restart
    of all 48 replicas over their whole LogDBs needs the same 96 again; taking
    them only from the other parity's stack and the bump counter leaves 33
    replicas with F_NOMEM.  (The third page per replica starts near round 163
    and this pool cannot hold it: the run stops at 150.)"""
    eng = LaunchCpu(trace=True, ring=RING, pool_bytes=256 << 10, **C2_SMALL)
    ref = O.Harness(**C2_SMALL)
    lockstep(eng, ref, 120)
    assert eng.spill_stats()["pool_pages_used"] == view_pages(ref.views()) == 96
    restart(eng, ref, list(range(eng.n_rep)), None)
    n, bits = eng.faults()
    assert n == 0, f"{n} replicas faulted ({bits:#x})"
    st = eng.spill_stats()
    assert st["oom"] == 0 and st["pool_pages_used"] == view_pages(ref.views())
    lockstep(eng, ref, 30)
    assert eng.faults()[0] == 0 and eng.spill_stats()["oom"] == 0
    assert not counters_match(eng.counters(), ref.counters())


def tier_split(eng, replicas):
    """Every listed replica: its chain's tail in HBM, the rest in host pages."""
    first = eng.spill_stats()["pool_pages"] + 1
    for r in replicas:
        ids = [p for p, _ in eng.chain(r)]
        assert ids and ids[-1] < first and all(p >= first for p in ids[:-1]), (r, ids)


def test_launch_places_pages_in_host_tier():
    eng = LaunchCpu(trace=True, ring=RING, host_pool_bytes=1024 * 2048, **C2_SMALL)
    ref = O.Harness(**C2_SMALL)
    lockstep(eng, ref, 300)
    assert eng.tier_stats() == dict(host_pages_used=0, host_pages=1024)  # (no demotion here)
    everyone = list(range(eng.n_rep))
    restart(eng, ref, everyone, None)
    total = view_pages(ref.views())
    assert total > 200
    assert eng.faults()[0] == 0 and eng.spill_stats()["oom"] == 0
    assert eng.spill_stats()["pool_pages_used"] == 48
    assert eng.tier_stats()["host_pages_used"] == total - 48
    tier_split(eng, everyone)
    lockstep(eng, ref, 120)
    assert not counters_match(eng.counters(), ref.counters())
    for r in (0, 1, 24, 47):
        want = [(e.index, e.term) for e in ref.persisted_entries(r, 1, 40)]
        assert [(x[0], x[1]) for x in eng.entries(r, 1, 40)] == want, r
    # one follower per group
    views = ref.views()
    picks = [next(r for r in range(3 * g, 3 * g + 3) if views[r].role != O.LEADER)
             for g in range(16)]
    restart(eng, ref, picks, None)
    tier_split(eng, picks)
    st, ts = eng.spill_stats(), eng.tier_stats()
    assert st["pool_pages_used"] + ts["host_pages_used"] == view_pages(ref.views())
    lockstep(eng, ref, 60)
    assert eng.faults()[0] == 0 and eng.spill_stats()["oom"] == 0
    assert not counters_match(eng.counters(), ref.counters())


def test_launch_full_tier_falls_back_to_hbm():
    eng = LaunchCpu(trace=True, ring=RING, host_pool_bytes=100 * 2048, **C2_SMALL)
    ref = O.Harness(**C2_SMALL)
    lockstep(eng, ref, 300)
    restart(eng, ref, list(range(eng.n_rep)), None)
    total = view_pages(ref.views())
    assert eng.tier_stats()["host_pages_used"] == 100
    assert eng.spill_stats()["pool_pages_used"] == total - 100
    assert eng.faults()[0] == 0 and eng.spill_stats()["oom"] == 0
    lockstep(eng, ref, 30)
    assert eng.faults()[0] == 0


def test_launch_exhaustion_is_per_replica():
    """48 LogDBs of 5 pages over a 100-page tier and a 63-page pool.  The host
    build allocates in batch order: the tier serves four pages each of
    replicas 0-24, whose tails take 25 HBM pages; the other 38 HBM pages serve
    replicas 25-31 whole (35) and three pages of replica 32, which gives them
    back.  Replicas 32-47 fault alone and hold nothing."""
    eng = LaunchCpu(trace=True, n_groups=16, n_replicas=3, ring=RING, pool_bytes=64 * 2048,
                    host_pool_bytes=100 * 2048)
    assert eng.spill_stats()["pool_pages"] == 63
    reps = list(range(48))
    dbs = [logdb(300, 300) for _ in reps]
    assert cold_pages(300) == 5
    eng.launch(reps, [st for st, _ in dbs], [ents for _, ents in dbs])
    faulted = [r for r in reps if not eng.chain(r)]
    assert faulted == list(range(32, 48))
    n, bits = eng.faults()
    assert n == len(faulted) and bits == F_NOMEM
    assert eng.spill_stats()["oom"] & 1
    for r in reps:
        if r in faulted:
            continue
        assert len(eng.chain(r)) == 5
        assert eng.entries(r, 1, 300) == [tuple(e) for e in dbs[r][1]], r
    used = eng.spill_stats()["pool_pages_used"] + eng.tier_stats()["host_pages_used"]
    assert used == 5 * (48 - len(faulted))
