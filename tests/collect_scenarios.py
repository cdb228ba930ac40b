"""Batched read of the Updates' entries (rbe_collect_entries /
rbe_collect_entry_ranges): scenarios shared by the CPU tier
(tests/test_collect_entries.py, the host build of tests/collect_cpu) and the
GPU tier (tests/test_gpu_collect_entries.py, the HIP engine through the C
ABI), each against the oracle harness.  `make(**cfg)` builds the engine.

The node loop hands every node's EntriesToSave to logdb.SaveRaftState in one
batch and the CommittedEntries to the state machine (execengine.go:523,
node.go:959-977).  A Tracker does that with the collected lists after every
round: the save lists replayed into a Python LogDB (entries from the first
index on replace everything at and above it) must end equal to the oracle's
LogDB, and the committed lists, concatenated, must be the entries 1..processed
once and in order, equal to the oracle's and across the replicas of a group.
Every round it also checks the lists against the calls that existed before
(the Updates' ranges, rbe_get_entries + rbe_get_entry_cmds on a sample)."""
import numpy as np

import oracle as O
from dragonboat_amd.engine import (RBE_E_INVALID, RBE_E_STATE, RBE_ENTRIES_COMMITTED,
                                   RBE_ENTRIES_TO_SAVE, SESSION_FIELDS)
from heap_util import mixed_cmd
from input_util import run_driven
from launch_util import restart
from parity_util import C2, view_diff
from transport_util import deliver, owner

SAVE, COMMITTED = RBE_ENTRIES_TO_SAVE, RBE_ENTRIES_COMMITTED


def entry_dicts(lst, i):
    """Range i of a collected list as Engine.entry_records returns entries."""
    rep, eoff, ents, coff, cmds = lst
    out = []
    for j in range(int(eoff[i]), int(eoff[i + 1])):
        e = ents[j]
        n = int(e["cmd_len"])
        if coff is None:
            cmd = bytes(e["cmd"][:min(16, n)])
        else:
            assert int(coff[j]) % 16 == 0
            cmd = cmds[int(coff[j]):int(coff[j]) + n].tobytes()
            pad = cmds[int(coff[j]) + n:int(coff[j + 1])]
            assert len(pad) < 16 and not pad.any(), "padding bytes are zero"
            assert bytes(e["cmd"][:min(16, n)]) == cmd[:16]
        out.append(dict(index=int(e["index"]), term=int(e["term"]), type=int(e["type"]), cmd=cmd,
                        **{f: int(e[f]) for f in SESSION_FIELDS}))
    return out


def by_replica(lst):
    return {int(r): entry_dicts(lst, i) for i, r in enumerate(lst[0])}


def same_as_oracle(mine, theirs):
    """Index, Term, Type, the session fields and the first 64 Cmd bytes."""
    assert len(mine) == len(theirs)
    for a, b in zip(mine, theirs):
        assert (a["index"], a["term"], a["type"]) == (b.index, b.term, b.type), (a, b)
        assert tuple(a[f] for f in SESSION_FIELDS) == tuple(getattr(b, f) for f in SESSION_FIELDS)
        assert a["cmd"][:64] == b.cmd[:64], (a["index"], len(a["cmd"]))


def update_ranges(eng):
    """{replica: (save_lo, save_hi, apply_lo, apply_hi)} of the last Updates."""
    if hasattr(eng, "collect_updates"):
        rep, ups = eng.collect_updates()
    else:
        ups = eng.updates()
        rep = range(len(ups))
    return {int(r): tuple(int(u[f]) for f in ("save_lo", "save_hi", "apply_lo", "apply_hi"))
            for r, u in zip(rep, ups)}


class Tracker:
    def __init__(self, eng, n, pushed=None, sample=2):
        self.eng, self.n, self.pushed, self.sample = eng, n, pushed, sample
        self.logdb = [[] for _ in range(eng.n_rep)]
        self.applied = [[] for _ in range(eng.n_rep)]
        self.rounds = 0
        self.longest = {SAVE: 0, COMMITTED: 0}
        self.entries = 0

    def after_round(self, first=False):
        eng = self.eng
        lists = {w: eng.collect_entries(which=w) for w in (SAVE, COMMITTED)}
        if first:  # before the first step: empty lists
            for lst in lists.values():
                assert len(lst[0]) == 0 and len(lst[2]) == 0 and list(lst[1]) == [0]
            return
        self.rounds += 1
        rng = update_ranges(eng)
        for w, lst in lists.items():
            rep, eoff = lst[0], lst[1]
            want = [(r, x[0 if w == SAVE else 2], x[1 if w == SAVE else 3])
                    for r, x in sorted(rng.items())]
            want = [(r, lo, hi) for r, lo, hi in want if lo <= hi]
            assert [int(r) for r in rep] == [r for r, _, _ in want]
            assert [int(x) for x in np.diff(eoff)] == [hi - lo + 1 for _, lo, hi in want]
            assert int(eoff[0]) == 0 and int(eoff[-1]) == len(lst[2])
            got = by_replica(lst)
            for r, lo, hi in want:
                assert [e["index"] for e in got[r]] == list(range(lo, hi + 1))
                self.longest[w] = max(self.longest[w], hi - lo + 1)
                self.entries += hi - lo + 1
            # against rbe_get_entries + rbe_get_entry_cmds, a rotating sample
            for k in range(min(self.sample, len(want))):
                r, lo, hi = want[(self.rounds * 7 + k * 3) % len(want)]
                assert got[r] == eng.entry_records(r, lo, hi), (w, r, lo, hi)
            # records only: the same records, no Cmd pointers
            bare = eng.collect_entries(which=w, cmds=False)
            assert bare[3] is None and bare[4] is None
            assert np.array_equal(bare[0], rep) and np.array_equal(bare[1], eoff)
            assert bare[2].tobytes() == lst[2].tobytes()
            # a sub-range that starts and ends inside a group
            first, count = self.n + 1, eng.n_rep - 2 * self.n
            if count > 0:
                part = by_replica(eng.collect_entries(first, count, which=w))
                assert part == {r: v for r, v in got.items() if first <= r < first + count}
            if self.pushed is not None:
                for es in got.values():
                    for e in es:
                        assert len(e["cmd"]) <= 16 or e["cmd"] in self.pushed, e["index"]
            for r, es in got.items():
                if w == SAVE:
                    del self.logdb[r][es[0]["index"] - 1:]
                    assert len(self.logdb[r]) == es[0]["index"] - 1
                    self.logdb[r].extend(es)
                else:
                    self.applied[r].extend(es)

    def finish(self, ref):
        views = ref.views()
        for r in range(self.eng.n_rep):
            last = ref.persisted(r)[3]
            same_as_oracle(self.logdb[r], ref.persisted_entries(r, 1, last) if last else [])
            done = views[r].processed
            assert [e["index"] for e in self.applied[r]] == list(range(1, done + 1)), r
            same_as_oracle(self.applied[r], ref.persisted_entries(r, 1, done) if done else [])
            g0 = r - r % self.n
            k = min(len(self.applied[r]), len(self.applied[g0]))
            assert self.applied[r][:k] == self.applied[g0][:k], "replicas of a group agree"


def no_faults(eng):
    assert eng.faults()[0] == 0


def oracle_logdb(make, mes):
    """Cases 1 and 2: driven mixed-size session proposals through the heap."""
    kw = dict(C2, n_groups=8, ext_inputs=True, max_entry_size=mes)
    eng, ref = make(trace=True, heap_bytes=64 << 20, **kw), O.Harness(**kw)
    pushed = set()

    def keep(ops):
        for kind, _, a in ops:
            if kind == "prop":
                pushed.update(bytes(e.cmd) for e in a)

    t = Tracker(eng, kw["n_replicas"], pushed)
    d = run_driven(eng, ref, 120, seed=13, cmd=mixed_cmd, on_ops=keep, session=True,
                   before_round=lambda rnd: t.after_round(first=rnd == 0))
    assert d is None, f"first divergence {d}"
    t.after_round()
    no_faults(eng)
    t.finish(ref)
    assert t.rounds == 120 and t.entries > 500, (t.rounds, t.entries)


def lockstep(eng, ref, rounds, each=None):
    for rnd in range(rounds):
        eng.step()
        ref.step()
        ev, hv = eng.views(), ref.views()
        for i in range(len(hv)):
            d = view_diff(ev[i], hv[i])
            assert d is None, f"first divergence at round {rnd}, replica {i}: {d}"
        if each:
            each()


ISO = dict(n_groups=4, n_replicas=5, check_quorum=True, wl_enabled=True, wl_start_round=30,
           iso_period=60, iso_len=40, iso_mod=1)


def cold_and_ring(make):
    """Case 3: a returning leader's catch-up appends 20 entries and applies 31
    in one step with a ring of 8: one save range and one committed range reach
    from the cold log into the ring."""
    eng, ref = make(trace=True, ring=8, **ISO), O.Harness(**ISO)
    t = Tracker(eng, ISO["n_replicas"])
    lockstep(eng, ref, 130, t.after_round)
    no_faults(eng)
    t.finish(ref)
    assert t.longest[SAVE] > 8 and t.longest[COMMITTED] > 8, t.longest


def relaunch_replay(make):
    """Case 4: a replica relaunched over its whole LogDB applies its log again
    from index 1 in one Update, most of it below the ring."""
    kw = dict(C2, n_groups=4)
    eng, ref = make(trace=True, ring=8, **kw), O.Harness(**kw)
    lockstep(eng, ref, 200)
    restart(eng, ref, [1], None)
    lockstep(eng, ref, 1)
    got = by_replica(eng.collect_entries(which=COMMITTED))
    assert 1 in got and got[1][0]["index"] == 1
    hi = got[1][-1]["index"]
    assert hi - 8 > 100, hi  # (the oracle: [1, 181], 173 of them below the ring)
    same_as_oracle(got[1], ref.persisted_entries(1, 1, hi))
    assert got[1] == eng.entry_records(1, 1, hi)
    no_faults(eng)


def launch_then_collect(make):
    """Between an rbe_launch and the step after it the launched entries are in
    the logs while their heap records (session fields, Cmds over 16 bytes) are
    still staged for that step: the ranges read back every field, as
    rbe_get_entries + rbe_get_entry_cmds do, before the step and after it."""
    eng = make(trace=True, n_groups=2, n_replicas=3, ext_inputs=True, heap_bytes=1 << 20)
    long = bytes(range(256)) * 5 + b"tail"  # 1,284 bytes: copied by a whole wave
    ents = [(1, 1, 0, b"a" * 40, 5, 6, 7, 8), (2, 1, 0, b"b", 1 << 60, 0, 3, 0),
            (3, 2, 2, b"", 0, 0, 0, 0), (4, 2, 0, long, 9, 1 << 50, 0, 2),
            (5, 2, 0, b"c" * 17, 0, 0, 0, 0)]
    other = [(1, 1, 0, b"z" * 300, 1, 2, 3, 4)]
    eng.launch([0, 4], [(2, 0, 2, 5), (1, 0, 1, 1)], [ents, other])
    for stepped in (False, True):
        got = eng.collect_entry_ranges([0, 4, 0], [1, 1, 4], [5, 1, 4])
        for i, (r, lo, want) in enumerate(((0, 1, ents), (4, 1, other), (0, 4, ents[3:4]))):
            mine = entry_dicts(got, i)
            assert [(x["index"], x["term"], x["type"], x["cmd"], x["key"], x["client_id"],
                     x["series_id"], x["responded_to"]) for x in mine] == want, (stepped, i)
            assert mine == eng.entry_records(r, lo, lo + len(want) - 1)
        bare = eng.collect_entry_ranges([0, 4, 0], [1, 1, 4], [5, 1, 4], cmds=False)
        assert bare[2].tobytes() == got[2].tobytes() and bare[3] is None
        eng.step()
    no_faults(eng)


def host_tier_ranges(make):
    """Case 5 (GPU only): whole logs whose older pages the demotion moved to
    host-pinned memory, read in one call."""
    kw = dict(C2, n_groups=16)
    eng = make(trace=True, ring=8, pool_bytes=256 << 10, host_pool_bytes=2 << 20, **kw)
    ref = O.Harness(**kw)
    eng.run(330)
    ref.run(330)
    ev, hv = eng.views(), ref.views()
    for i in range(len(hv)):
        assert view_diff(ev[i], hv[i]) is None, i
    assert eng.cold_tier_stats()["host_pages_used"] > 0
    no_faults(eng)
    reps = list(range(eng.n_rep))
    last = [hv[r].last_index for r in reps]
    lst = eng.collect_entry_ranges(reps, [1] * len(reps), last)
    assert [int(r) for r in lst[0]] == reps
    for i, r in enumerate(reps):
        mine = entry_dicts(lst, i)
        same_as_oracle(mine, ref.persisted_entries(r, 1, last[r]))
        assert mine == eng.entry_records(r, 1, last[r]), r


def _rc(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except RuntimeError as e:  # (the host build's getters raise a plain one)
        return getattr(e, "rc", None)
    return 0


def bad_arguments(make, raw):
    """Case 6: refusals.  `raw(eng, name, *args)` calls the C function `name`
    with a null-able handle and out pointer and returns its code."""
    kw = dict(C2, n_groups=4)
    eng, ref = make(trace=True, **kw), O.Harness(**kw)
    for w in (SAVE, COMMITTED):  # before the first step: empty lists
        lst = eng.collect_entries(which=w)
        assert len(lst[0]) == 0 and len(lst[2]) == 0 and list(lst[1]) == [0] and list(lst[3]) == [0]
    lockstep(eng, ref, 60)
    last = ref.views()[2].last_index
    assert last > 5
    ok = eng.collect_entry_ranges([2, 0, 2], [1, 2, last], [last, 2, last])
    assert [int(r) for r in ok[0]] == [2, 0, 2]  # call order, a replica twice
    assert [int(x) for x in ok[1]] == [0, last, last + 1, last + 2]
    assert entry_dicts(ok, 0) == eng.entry_records(2, 1, last)
    assert entry_dicts(ok, 2) == eng.entry_records(2, last, last)
    for rep, lo, hi in (([2], [0], [1]), ([2], [3], [2]), ([2], [1], [last + 1]),
                        ([eng.n_rep], [1], [1]), ([0, 2], [1, 1], [1, last + 1])):
        assert _rc(eng.collect_entry_ranges, rep, lo, hi) == RBE_E_INVALID, (rep, lo, hi)
    for which in (0, SAVE | COMMITTED, 4):
        assert _rc(eng.collect_entries, which=which) == RBE_E_INVALID
    assert _rc(eng.collect_entries, 0, 0) == RBE_E_INVALID
    assert _rc(eng.collect_entries, 3, eng.n_rep) == RBE_E_INVALID
    assert raw(eng, "collect_entries", False, True) == RBE_E_INVALID   # null handle
    assert raw(eng, "collect_entries", True, False) == RBE_E_INVALID   # null out
    assert raw(eng, "collect_entry_ranges", False, True) == RBE_E_INVALID
    assert raw(eng, "collect_entry_ranges", True, False) == RBE_E_INVALID
    no_faults(eng)


def lapped_heap(make, get_entries_rc):
    """Case 6: a heap smaller than the log window (the shape of
    test_heap_laps_report_compacted): a range reaching 60 entries back holds
    records a later lap overwrote.  `get_entries_rc(eng, replica, lo, hi)` is
    the code of rbe_get_entries alone."""
    kw = dict(C2, n_groups=4, ext_inputs=True)
    eng, ref = make(trace=True, heap_bytes=256 << 10, **kw), O.Harness(**kw)
    d = run_driven(eng, ref, 120, seed=9, cmd=lambda rng: rng.randbytes(4000), density=0.3)
    assert d is None, f"first divergence {d}"
    last = ref.views()[0].last_index
    lo = max(1, last - 60)
    assert _rc(eng.collect_entry_ranges, [0], [lo], [last]) == RBE_E_STATE
    # records only read a heap record's header and first 16 bytes: the same
    # answer as rbe_get_entries on the same range, and on one it can serve
    assert get_entries_rc(eng, 0, lo, last) == RBE_E_STATE
    assert _rc(eng.collect_entry_ranges, [0], [lo], [last], cmds=False) == RBE_E_STATE
    assert get_entries_rc(eng, 0, last, last) == 0
    got = eng.collect_entry_ranges([0], [last], [last])
    assert entry_dicts(got, 0) == eng.entry_records(0, last, last)
    bare = eng.collect_entry_ranges([0], [last], [last], cmds=False)
    assert bare[2].tobytes() == got[2].tobytes() and bare[3] is None
    no_faults(eng)


def compacted_range(make):
    """Case 6: with snapshots on, a range below the compaction marker."""
    kw = dict(C2, n_groups=4, snapshot_entries=20, compaction_overhead=5)
    eng, ref = make(trace=True, **kw), O.Harness(**kw)
    lockstep(eng, ref, 120)
    marker = ref.snapshot_state(0)[0]
    last = ref.views()[0].last_index
    assert 1 < marker < last
    assert _rc(eng.collect_entry_ranges, [0], [1], [last]) == RBE_E_STATE
    assert _rc(eng.entry_records, 0, 1, last) != 0
    # up to the marker the answer is rbe_get_entries' (the ring may still hold
    # the last compacted entries): refused by both, or the same entries
    for lo in (marker, max(1, marker - 1)):
        if _rc(eng.entry_records, 0, lo, last) == 0:
            assert entry_dicts(eng.collect_entry_ranges([0], [lo], [last]), 0) == \
                eng.entry_records(0, lo, last)
        else:
            assert _rc(eng.collect_entry_ranges, [0], [lo], [last]) == RBE_E_STATE
    got = eng.collect_entry_ranges([0, 1], [marker + 1, last], [last, last])
    assert entry_dicts(got, 0) == eng.entry_records(0, marker + 1, last)
    no_faults(eng)


def replica_mode(make):
    """Case 7: two engines of a replica-per-engine deployment (rep_world = 2,
    rep_compact off) over the in-process transport: each rank's save list
    names only replicas it steps, and the ranks' lists together are the list
    of one engine stepping every replica."""
    kw = dict(C2, n_groups=8)
    n, world = kw["n_replicas"], 2
    engs = [make(trace=True, rep_world=world, rep_rank=r, **kw) for r in range(world)]
    one = make(trace=True, **kw)
    seen = 0
    for rnd in range(80):
        for e in engs + [one]:
            e.step()
        deliver(engs, n, one.n_rep)
        for w in (SAVE, COMMITTED):
            union = {}
            for rank, e in enumerate(engs):
                got = by_replica(e.collect_entries(which=w))
                assert all(owner(r // n, r % n, world) == rank for r in got), (rank, sorted(got))
                union.update(got)
            assert union == by_replica(one.collect_entries(which=w)), (rnd, w)
            seen += len(union)
    assert seen > 200
    for e in engs + [one]:
        no_faults(e)
