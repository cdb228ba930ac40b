"""The cold log's host tier on the HIP engine (cfg.host_pool_bytes;
tests/test_cold_tier.py is the CPU tier): with snapshots off the cold log
keeps every evicted entry, so a page pool of any size fills; with the tier the
committed pages below each tail move to host-pinned memory after the round
(k_cold_demote_plan / k_cold_demote_copy) and are read there in place.  Small
pools that run out without the tier (test_cold_tier.py shows they do) run 620
rounds in lockstep with the oracle, fault-free.

Page budgets, from the oracle's views of these runs (a page holds 64 entries;
every entry below a replica's 8-entry ring is in its cold log): the C2 shape
ends with 480 pages, of which at most 48 are not demotable (tails and
uncommitted pages) and at most 32 are new in a round, against 127 HBM pages;
LONG_ISO ends with 695 (CheckQuorum) or 745 pages, at most 80 / 99 not
demotable and 64 new in a round, against 255 HBM pages."""
import pytest

import oracle as O
from parity_util import C2, counters_match, view_diff
from test_spill import LONG_ISO

pytestmark = pytest.mark.gpu

ROUNDS = 620
C2_SMALL = dict(C2, n_groups=16)
C2_TIER = dict(ring=8, pool_bytes=256 << 10, host_pool_bytes=2 << 20)
ISO_TIER = dict(ring=8, pool_bytes=512 << 10, host_pool_bytes=4 << 20)

_ORACLE = {}


def oracle_run(kw):
    """The oracle's views after each of ROUNDS rounds, its counters (at the
    end, and at the rounds an export is taken and its resumed run ends) and a
    few replicas' first 40 persisted entries at the end: computed once per
    configuration and shared (never changed) by the cases that use it."""
    key = tuple(sorted(kw.items()))
    if key not in _ORACLE:
        ref = O.Harness(trace=True, **kw)
        views, at = [], {}
        for rnd in range(1, ROUNDS + 1):
            ref.run(1)
            views.append(ref.views())
            if rnd in (340, 540):
                at[rnd] = ref.counters()
        n = kw["n_groups"] * kw["n_replicas"]
        ents = {r: [(e.index, e.term) for e in ref.persisted_entries(r, 1, 40)]
                for r in (0, 1, n // 2, n - 1)}
        _ORACLE[key] = dict(views=views, counters=ref.counters(), counters_at=at, entries=ents)
    return _ORACLE[key]


def lockstep(eng, ref, first, last, every=1, skip=()):
    """Rounds (first, last] of the engine, compared with the oracle's views
    every `every` rounds."""
    done = first
    while done < last:
        k = min(every, last - done)
        eng.run(k)
        done += k
        ev, hv = eng.views(), ref["views"][done - 1]
        for i in range(len(hv)):
            d = view_diff(ev[i], hv[i], skip)
            assert d is None, f"first divergence at round {done}, replica {i}: {d}"


def check_end(eng, ref, counters=True):
    n, bits = eng.fault_summary()
    assert n == 0, f"{n} replicas faulted ({bits:#x})"
    if counters:
        bad = counters_match(eng.counters(), ref["counters"])
        assert not bad, f"counters differ {bad}"
    assert eng.spill_stats()["oom"] == 0
    for r, want in ref["entries"].items():  # a boundary read out of host pages
        assert [(x[0], x[1]) for x in eng.entries(r, 1, 40)] == want, r


@pytest.mark.parametrize("mode", ["stepped", "full", "untraced", "graph20"])
def test_gpu_c2_small_pool_with_host_tier(gpu_available, monkeypatch, mode):
    """16 x 3 with a proposal per group per round: 480 pages of cold log by
    round 620 in a 127-page pool.  Stepped every round (traced, the full
    handler table alone, untraced) and 20 rounds at a time, where the
    demotion kernels replay inside the captured graph."""
    from dragonboat_amd.engine import Engine
    if mode == "full":
        monkeypatch.setenv("RBE_MODE", "full")
    trace = mode != "untraced"
    ref = oracle_run(C2_SMALL)
    eng = Engine(device=0, trace=trace, **C2_TIER, **C2_SMALL)
    lockstep(eng, ref, 0, ROUNDS, every=20 if mode == "graph20" else 1,
             skip=() if trace else ("digest",))
    check_end(eng, ref)
    st, ct = eng.spill_stats(), eng.cold_tier_stats()
    print(f"c2 {mode}: hbm pages {st['pool_pages_used']} of {st['pool_pages']}, "
          f"host pages {ct['host_pages_used']} of {ct['host_pages']}, "
          f"demoted {ct['demoted']} in {ct['passes']} passes")
    assert ct["host_pages"] == (2 << 20) // 2048
    assert ct["host_pages_used"] > 0 and ct["demoted"] >= ct["host_pages_used"] and ct["passes"] > 0
    # the two tiers together hold exactly what one big pool holds
    big = Engine(device=0, trace=trace, ring=8, **C2_SMALL)
    big.run(ROUNDS)
    assert big.cold_tier_stats() == dict(host_pages_used=0, host_pages=0, demoted=0, passes=0)
    assert st["pool_pages_used"] + ct["host_pages_used"] == big.spill_stats()["pool_pages_used"]
    big.close()
    eng.close()


@pytest.mark.parametrize("check_quorum", [True, False])
def test_gpu_long_isolation_with_host_tier(gpu_available, check_quorum):
    """5 replicas, every other group's leader isolated for 150 of every 200
    rounds.  With CheckQuorum the returning replica's catch-up Replicate is
    read from the leader's host pages; without it the isolated leader's stale
    tail is cut back (a rewrite below the tail of its cold log)."""
    from dragonboat_amd.engine import Engine
    kw = dict(LONG_ISO, check_quorum=check_quorum)
    ref = oracle_run(kw)
    eng = Engine(device=0, trace=True, **ISO_TIER, **kw)
    lockstep(eng, ref, 0, ROUNDS)
    check_end(eng, ref)
    st, ct = eng.spill_stats(), eng.cold_tier_stats()
    print(f"long_iso cq={check_quorum}: hbm pages {st['pool_pages_used']} of {st['pool_pages']}, "
          f"host pages {ct['host_pages_used']}, demoted {ct['demoted']} in {ct['passes']} passes")
    assert ct["host_pages_used"] > 0 and st["spill_peak_bytes"] > 0
    eng.close()


@pytest.mark.parametrize("target", ["default_pool", "tiered"])
def test_gpu_host_tier_export_import(gpu_available, target):
    """A tiered engine's export at round 340 (mid-isolation, most pages on the
    host) resumes bit-exact for 200 rounds in a fresh engine without a tier,
    and in a fresh tiered engine with the same 512 KiB pool, whose rebuild puts
    every page but the tails straight into host pages."""
    from dragonboat_amd.engine import Engine
    kw = dict(LONG_ISO, check_quorum=False)
    ref = oracle_run(kw)
    a = Engine(device=0, trace=True, **ISO_TIER, **kw)
    lockstep(a, ref, 0, 340, every=20)
    sa, ca = a.spill_stats(), a.cold_tier_stats()
    assert ca["host_pages_used"] > 0 and sa["oom"] == 0
    bad = counters_match(a.counters(), ref["counters_at"][340])
    assert not bad, f"counters differ at the export {bad}"
    snap = a.export_groups()
    a.close()
    if target == "tiered":
        b = Engine(device=0, trace=True, **ISO_TIER, **kw)
    else:
        b = Engine(device=0, trace=True, ring=8, **kw)
    b.import_groups(snap, resume=True)
    sb, cb = b.spill_stats(), b.cold_tier_stats()
    assert sb["pool_pages_used"] + cb["host_pages_used"] == \
        sa["pool_pages_used"] + ca["host_pages_used"]
    if target == "tiered":  # only the tails (one per replica at most) are in HBM
        assert sb["pool_pages_used"] <= b.n_rep
    lockstep(b, ref, 340, 540)
    n, bits = b.fault_summary()
    assert n == 0, f"{n} replicas faulted ({bits:#x})"
    # a resumed engine counts from the import: its counters equal what the
    # oracle counted over the same 200 rounds
    c0, c1 = ref["counters_at"][340], ref["counters_at"][540]
    bad = counters_match(b.counters(), {k: c1[k] - c0[k] for k in c1})
    assert not bad, f"counters differ over the resumed rounds {bad}"
    assert b.spill_stats()["oom"] == 0
    b.close()
