"""Dropped lists (rbe_collect_dropped / rbe_get_dropped): scenarios shared by
the CPU tier (tests/test_dropped_collect.py, the host build of
tests/dropped_cpu) and the GPU tier (tests/test_gpu_dropped_collect.py, the HIP
engine through the C ABI).  `make(**cfg)` builds the engine.

The oracle harness exposes no per-replica dropped lists (it folds them into the
trace digest, which pins the counts and the content hash of every step's
dropped entries already).  These scenarios add contents and order: the batched
list against the per-replica getter field for field, against what was pushed,
and against the reference rule on a single oracle Raft object.  Every scenario
returns what it observed, so the GPU tier can compare the device with the host
build list for list."""
import ctypes as C
import random

import numpy as np

import oracle as O
from dragonboat_amd.engine import (RBE_E_INVALID, RBE_E_STATE, RBE_ENTRIES_COMMITTED,
                                   RbeDroppedList)
from input_util import apply_engine, apply_oracle, run_driven
from outbox_scenarios import deliver_batched, faults, lockstep
from ingest_spill_scenarios import step_all
from transport_util import owner

F_NOMEM = 0x100
E_CONFIG_CHANGE = 1


def ent_t(e, cmd):
    """An rbe_entry and its whole Cmd as a tuple."""
    return (e.index, e.term, e.type, e.cmd_len, e.key, e.client_id, e.series_id, e.responded_to,
            bytes(cmd))


def check_raw(d, cmds):
    """The offsets of the raw lists are consistent; each cmd_off is a multiple
    of 16, a Cmd's first 16 bytes are its record's, and the pad bytes are zero."""
    n, ne, nr = len(d["replica"]), len(d["entries"]), len(d["read_indexes"])
    rep = [int(r) for r in d["replica"]]
    assert rep == sorted(set(rep))
    eoff, roff = d["ent_off"], d["ri_off"]
    assert len(eoff) == n + 1 and int(eoff[0]) == 0 and int(eoff[-1]) == ne
    assert len(roff) == n + 1 and int(roff[0]) == 0 and int(roff[-1]) == nr
    de, dr = np.diff(eoff.astype(np.int64)), np.diff(roff.astype(np.int64))
    assert (de >= 0).all() and (dr >= 0).all() and ((de + dr) > 0).all(), "a listed replica has a drop"
    assert not d["entries"]["index"].any(), "a dropped proposal has no index"
    if not cmds:
        assert d["cmd_off"] is None and d["cmds"] is None
        return
    coff, blob = d["cmd_off"], d["cmds"]
    assert len(coff) == ne + 1 and int(coff[0]) == 0 and int(coff[-1]) == len(blob)
    for j in range(ne):
        a, b, ln = int(coff[j]), int(coff[j + 1]), int(d["entries"][j]["cmd_len"])
        assert a % 16 == 0 and b - a == (ln + 15) // 16 * 16, (j, a, b, ln)
        assert not blob[a + ln:b].any(), "padding bytes are zero"
        assert bytes(d["entries"][j]["cmd"][:min(16, ln)]) == blob[a:a + min(16, ln)].tobytes()


def observe(eng, first=0, count=None, counts=True, owned=None):
    """The lists of [first, first + count) as {replica: ([entry tuples],
    [contexts])}, after checking the batched call against the raw layout, the
    call without Cmds, rbe_get_dropped of every replica of the range and, with
    `counts`, the Updates' n_dropped_entries / n_dropped_read_indexes."""
    count = eng.n_rep - first if count is None else count
    check_raw(eng.collect_dropped(first, count, raw=True), True)
    check_raw(eng.collect_dropped(first, count, cmds=False, raw=True), False)
    got = eng.collect_dropped(first, count)
    bare = eng.collect_dropped(first, count, cmds=False)
    assert list(got) == list(bare)
    out = {}
    for r, (en, cm, ri) in got.items():
        assert first <= r < first + count
        assert bare[r][1] is None and bare[r][2] == ri
        assert [bytes(x) for x in bare[r][0]] == [bytes(x) for x in en], "the same records"
        out[r] = ([ent_t(e, c) for e, c in zip(en, cm)], ri)
    ups = eng.updates(first, count) if counts else None
    for r in range(first, first + count):
        if owned is not None and not owned(r):
            assert r not in out, "a replica another rank steps is not listed"
            continue
        en, cm, ri = eng.get_dropped(r)
        one = ([ent_t(e, c) for e, c in zip(en, cm)], ri)
        assert out.get(r, ([], [])) == one, (r, out.get(r), one)
        if counts:
            u = ups[r - first]
            assert len(one[0]) == u.n_dropped_entries and len(one[1]) == u.n_dropped_read_indexes, \
                (r, len(one[0]), u.n_dropped_entries, len(one[1]), u.n_dropped_read_indexes)
    return out


def pushed_t(e):
    """What a pushed proposal (an (type, cmd) pair or an O.Entry) comes back as,
    Index and Term aside."""
    if isinstance(e, tuple):
        return (e[0], len(e[1]), 0, 0, 0, 0, bytes(e[1]))
    return (e.type, len(e.cmd), e.key, e.client_id, e.series_id, e.responded_to, bytes(e.cmd))


def body(t):
    return t[2:]


# ------------------------------------------------------------------ 1. exact by construction
def exact(make):
    """A fresh 4 x 3 engine: before round 1 every replica is a follower without
    a leader, so what is pushed to it is dropped whole, in push order, with
    Index 0 — and the oracle's Raft object, stepped with the same Propose and
    ReadIndex, drops the same."""
    kw = dict(n_groups=4, n_replicas=3, ext_inputs=True)
    eng = make(trace=True, drop_lists=True, **kw)
    rng = random.Random(11)
    ops, want = [], {}
    for r in range(eng.n_rep):
        batch = [(rng.choice((0, 2, 3)), bytes([r, j]) + rng.randbytes(rng.randrange(15)))
                 for j in range(1 + r % 3)]
        ctx = ((r + 1) << 32 | 5, 1000 + r)
        ops += [("prop", r, batch), ("read", r, ctx)]
        want[r] = ([(0, 0) + pushed_t(e) for e in batch], [ctx])
        ref = O.Raft.new(r % 3 + 1, peers=(1, 2, 3))
        ref.handle(O.msg(O.Propose, **{"from": r % 3 + 1},
                         entries=[O.Entry(type=t, cmd=c) for t, c in batch]))
        ref.handle(O.msg(O.ReadIndex, **{"from": r % 3 + 1}, hint=ctx[0], hint_high=ctx[1]))
        assert [(e.index, e.term) + pushed_t(e) for e in ref.dropped_entries()] == want[r][0]
        assert ref.dropped_read_indexes() == want[r][1]
    assert observe(eng) == {}, "before the first step: empty lists"
    apply_engine(eng, ops)
    assert observe(eng) == {}, "pushed, not stepped"
    eng.step()
    got = observe(eng)
    assert got == want
    assert observe(eng, 4, 5) == {r: want[r] for r in range(4, 9)}
    eng.step()
    assert observe(eng) == {}, "the next round drops nothing"
    assert faults(eng) == 0
    return got


# ------------------------------------------------------------------ 2. driven lockstep
DRIVEN = dict(n_groups=16, n_replicas=3, ext_inputs=True, iso_period=40, iso_len=20, iso_mod=1)
# the seed with which the schedule below drops (checked on the host build):
# forwarded Proposes meet transferring and deposed leaders, reads meet leaders
# without a committed entry of their term
DRIVEN_SEED = 5


class Tracker:
    """Every pushed batch, and every dropped list checked against them: each
    dropped entry equals a pushed one byte for byte, the entries of a batch stay
    contiguous and in order, no batch is dropped twice."""

    def __init__(self):
        self.batches = []      # (replica pushed to, [bodies])
        self.where = {}        # body -> [(batch, position)]
        self.ctxs = set()
        self.dropped_batches = set()
        self.dropped_bodies = []
        self.n_ent = self.n_ri = self.forwarded = 0

    def on_ops(self, ops):
        for kind, r, a in ops:
            if kind == "prop":
                b = len(self.batches)
                self.batches.append((r, [pushed_t(e) for e in a]))
                for j, e in enumerate(a):
                    self.where.setdefault(pushed_t(e), []).append((b, j))
            elif kind == "read":
                self.ctxs.add(tuple(a))

    def check(self, lists):
        for r, (ents, ris) in lists.items():
            self.n_ent += len(ents)
            self.n_ri += len(ris)
            for c in ris:
                assert c in self.ctxs, (r, c)
            i = 0
            while i < len(ents):
                assert ents[i][0] == 0, "Index 0"
                at = self.where.get(body(ents[i]))
                assert at, ("not a pushed entry", r, ents[i])
                # the batch this run belongs to: one whose whole body list follows here
                fit = [b for b, j in at if j == 0 and b not in self.dropped_batches and
                       [body(x) for x in ents[i:i + len(self.batches[b][1])]] == self.batches[b][1]]
                assert fit, ("a batch cut or reordered, or dropped twice", r, i, ents[i])
                b = max(fit, key=lambda x: len(self.batches[x][1]))  # (equal bodies: the longest)
                self.dropped_batches.add(b)
                self.dropped_bodies += self.batches[b][1]
                if self.batches[b][0] != r:
                    self.forwarded += 1
                i += len(self.batches[b][1])


def _seq_cmd(long):
    """Identifiable Cmds: a running number, then 0-12 (without a heap) or up
    to 196 more bytes; with a heap one in twelve is empty."""
    seq = [0]

    def cmd(rng):
        seq[0] += 1
        if long and rng.random() < 1 / 12:
            return b""
        return seq[0].to_bytes(4, "little") + rng.randbytes(rng.randrange(197 if long else 13))
    return cmd


def driven(make, session=False, rounds=150, drop_lists=True, extra=None):
    """input_util.run_driven's schedule in lockstep with the harness; every
    round every replica's lists are observed and checked (Tracker)."""
    kw = dict(DRIVEN)
    ekw = dict(kw, heap_bytes=1 << 20) if session else kw
    cfg = dict(ekw, drop_lists=drop_lists)
    cfg.update(extra or {})
    eng, ref = make(trace=True, **cfg), O.Harness(**kw)
    tr = Tracker()
    seen, applied = [], set()

    def before_round(rnd):
        if rnd and drop_lists:
            got = observe(eng)
            tr.check(got)
            seen.append(got)
            if hasattr(eng, "collect_entries"):  # the round's CommittedEntries, batched
                _, _, ents, coff, blob = eng.collect_entries(which=RBE_ENTRIES_COMMITTED)
                for j, e in enumerate(ents):
                    c = blob[int(coff[j]):int(coff[j]) + int(e["cmd_len"])].tobytes()
                    applied.add((int(e["type"]), len(c), int(e["key"]), int(e["client_id"]),
                                 int(e["series_id"]), int(e["responded_to"]), c))
        elif rnd:
            seen.append(_everything(eng))

    d = run_driven(eng, ref, rounds, seed=DRIVEN_SEED, density=0.5, cmd=_seq_cmd(session),
                   on_ops=tr.on_ops, before_round=before_round, session=session)
    assert d is None, f"first divergence {d}"
    before_round(rounds)
    assert faults(eng) == 0
    if not drop_lists:
        return seen, eng
    c = ref.counters()
    assert tr.n_ent == c["dropped_proposals"] and tr.n_ri == c["dropped_reads"], \
        (tr.n_ent, tr.n_ri, c["dropped_proposals"], c["dropped_reads"])
    # the run really drops, and drops forwarded Proposes
    assert tr.n_ent >= 20 and tr.n_ri >= 10 and tr.forwarded >= 1, (tr.n_ent, tr.n_ri, tr.forwarded)
    # no dropped entry is in its group's committed log (entries pushed once)
    once = {b for b in tr.dropped_bodies if len(tr.where[b]) == 1}
    assert not once & applied, "a dropped entry was handed to the state machine"
    views = ref.views()
    for g in range(kw["n_groups"]):
        r = max(range(3 * g, 3 * g + 3), key=lambda x: views[x].committed)
        if views[r].committed:
            for e in eng.entry_records(r, 1, views[r].committed):
                b = (e["type"], len(e["cmd"]), e["key"], e["client_id"], e["series_id"],
                     e["responded_to"], e["cmd"])
                assert b not in once, (g, e)
    return seen, eng


def _everything(eng):
    """Views, Updates and outbox lists of a round (scenario 11)."""
    v = bytes(eng.views())
    u = bytes(eng.updates())
    ob = eng.collect_outbox(raw=True)
    return v, u, {k: (None if x is None else x.tobytes()) for k, x in ob.items()}


# the parent commit's spill_stats() for driven(drop_lists=False), on the host build
PARENT_SPILL = {False: dict(pool_pages_used=58, spill_peak_bytes=6592, oom=0),
                True: dict(pool_pages_used=60, spill_peak_bytes=6080, oom=0)}


def nothing_else_moved(make, session=False):
    """The schedule of 2 at drop_lists = 0 and 1: views, Updates, outbox lists
    and counters are identical round for round, and at 0 the spill tiers are
    used exactly as on the parent commit."""
    off, e0 = driven(make, session, drop_lists=False)
    kw = dict(DRIVEN)
    ekw = dict(kw, heap_bytes=1 << 20) if session else kw
    e1, ref = make(trace=True, drop_lists=True, **ekw), O.Harness(**kw)
    on = []
    d = run_driven(e1, ref, 150, seed=DRIVEN_SEED, density=0.5, cmd=_seq_cmd(session),
                   before_round=lambda rnd: rnd and on.append(_everything(e1)), session=session)
    assert d is None
    on.append(_everything(e1))
    assert len(on) == len(off) == 150
    for rnd, (a, b) in enumerate(zip(off, on)):
        assert a == b, f"round {rnd} differs with drop_lists on"
    assert e0.counters() == e1.counters()
    st = e0.spill_stats()
    assert {k: st[k] for k in PARENT_SPILL[session]} == PARENT_SPILL[session], st
    return st


# ------------------------------------------------------------------ 3. transferring leader
def transferring_leader(make, tiny=False):
    """A leader asked to transfer drops its own proposals and the Proposes its
    followers forward: in one step the forwarded batch (a message) comes before
    the node's own batch.  `tiny`: maxm = ecap = 1, so the forwarded entries
    come out of the round spill heap."""
    kw = dict(n_groups=4, n_replicas=3, ext_inputs=True)
    extra = dict(maxm=1, ecap=1) if tiny else {}
    eng, ref = make(trace=True, drop_lists=True, **kw, **extra), O.Harness(**kw)
    lockstep(eng, ref, 40)
    v = ref.views()
    lead = [r for r in range(3) if v[r].role == O.LEADER][0]
    foll = [r for r in range(3) if r != lead][0]
    fb = [(0, b"follower-%d" % j) for j in range(3)]
    lb = [(2, b"leader-%d" % j) for j in range(2)]

    def both(ops):
        apply_engine(eng, ops)
        apply_oracle(ref, ops)
        lockstep(eng, ref, 1)
        return observe(eng)

    got = [both([("xfer", lead, foll + 1), ("prop", foll, fb)])]
    got.append(both([("prop", lead, lb)]))
    want = [(0, v[lead].term) + pushed_t(e) for e in fb] + [(0, 0) + pushed_t(e) for e in lb]
    assert [body(x) for x in got[1][lead][0]] == [body(x) for x in want], got
    assert faults(eng) == 0
    if tiny:
        assert eng.spill_stats()["spill_peak_bytes"] > 0
    return got


# ------------------------------------------------------------------ 4. pending ConfigChange
def pending_config_change(make):
    """Two ConfigChange proposals at the leader in consecutive rounds: the
    second comes back as one dropped entry of type ConfigChange with its 8-byte
    Cmd, and the log took an empty Application entry in its place."""
    kw = dict(n_groups=2, n_replicas=3, ext_inputs=True, membership=True)
    eng, ref = make(trace=True, drop_lists=True, **kw), O.Harness(**kw)
    lockstep(eng, ref, 40)
    lead = [r for r in range(3) if ref.views()[r].role == O.LEADER][0]
    seen = []
    for _ in range(2):
        eng.propose_config_change([lead], [O.CC_REMOVE_NODE], [(lead + 1) % 3 + 1])
        ref.push(O.PUSH_CC_PROPOSE, lead, O.CC_REMOVE_NODE, (lead + 1) % 3 + 1)
        lockstep(eng, ref, 1)
        seen.append(observe(eng))
    assert seen[0] == {}
    (ents, ris), = [seen[1][lead]]
    assert list(seen[1]) == [lead] and len(ents) == 1 and ris == []
    last = ref.views()[lead].last_index
    first_cc, repl = eng.entry_records(lead, last - 1, last)
    assert first_cc["type"] == E_CONFIG_CHANGE and len(first_cc["cmd"]) == 8
    assert ents[0][2] == E_CONFIG_CHANGE and ents[0][3] == 8 and ents[0][8] == first_cc["cmd"]
    assert repl["type"] == 0 and repl["cmd"] == b"", "an empty Application entry took its place"
    assert eng.updates()[lead].n_dropped_entries == 1
    assert faults(eng) == 0
    return seen


# ------------------------------------------------------------------ 5. growth and block edges
GROW = (64, 65, 64, 62, 1, 1, 2, 3)  # prefix sums 255, 256, 257 after four, five, six replicas


def growth_and_block_edges(make):
    """One batch of n entries to a leaderless follower for n around the list's
    floor and its doublings, in ranges whose totals end below, on and past a
    256-lane block of the entries pass."""
    eng = make(trace=True, drop_lists=True, n_groups=4, n_replicas=3, ext_inputs=True)
    batches = [[(0, bytes([r]) + j.to_bytes(2, "little")) for j in range(n)]
               for r, n in enumerate(GROW)]
    eng.push_proposals(list(range(len(GROW))), batches)
    eng.step()
    got = observe(eng)
    for r, b in enumerate(batches):
        assert [body(x) for x in got[r][0]] == [pushed_t(e) for e in b], r
    for count, total in ((4, 255), (5, 256), (6, 257)):
        part = observe(eng, 0, count)
        assert sum(len(x[0]) for x in part.values()) == total
        assert part == {r: got[r] for r in range(count)}
    assert observe(eng, 1, 3) == {r: got[r] for r in (1, 2, 3)}
    assert faults(eng) == 0 and eng.spill_stats()["spill_peak_bytes"] > 0
    return got


# ------------------------------------------------------------------ 6. ReadIndexes past dri_cap
def read_indexes_past_dri_cap(make):
    """dri_cap = 1: a candidate that takes one ReadIndex lists the context
    twice (the reference's double append, raft.go:1935-1940), read out of the
    round spill heap."""
    kw = dict(n_groups=6, n_replicas=3, ext_inputs=True)
    eng, ref = make(trace=True, drop_lists=True, dri_cap=1, **kw), O.Harness(**kw)
    doubles, seen = 0, []
    for rnd in range(40):
        cand = [r for r, v in enumerate(ref.views()) if v.role == O.CANDIDATE]
        ops = [("read", r, (7000 + rnd, r)) for r in cand]
        apply_engine(eng, ops)
        apply_oracle(ref, ops)
        lockstep(eng, ref, 1)
        got = observe(eng)
        seen.append(got)
        for r in cand:
            ris = got.get(r, ([], []))[1]
            if ris == [(7000 + rnd, r)] * 2:
                doubles += 1
    assert doubles >= 1, "no candidate took a ReadIndex"
    assert faults(eng) == 0 and eng.spill_stats()["spill_peak_bytes"] > 0
    return seen


# ------------------------------------------------------------------ 7. Cmds and a lapped record
def lapped_record(make, raw):
    """A dropped heap entry whose record later pushes lap.  A Propose a
    follower forwards in round N is dropped by its transferring leader in round
    N + 1: after that step the record is in no log, in no outbox and older than
    the last flush's batch, so nothing keeps the heap from going round over it.
    The call succeeds before the lap; after it the whole call is RBE_E_STATE
    with *out all zero, with and without Cmds, and rbe_get_dropped refuses the
    replica.  `raw(eng, first, count, flags)` returns (code, RbeDroppedList)."""
    kw = dict(n_groups=2, n_replicas=3, ext_inputs=True)
    eng, ref = make(trace=True, drop_lists=True, heap_bytes=64 << 10, **kw), O.Harness(**kw)
    lockstep(eng, ref, 40)
    v = ref.views()
    lead = [r for r in range(3) if v[r].role == O.LEADER][0]
    foll = [r for r in range(3) if r != lead][0]
    big = O.Entry(type=0, cmd=b"d" * 3000, key=77, client_id=5, series_id=6, responded_to=4)
    ops = [("xfer", lead, foll + 1), ("prop", foll, [big])]
    apply_engine(eng, ops)
    apply_oracle(ref, ops)
    lockstep(eng, ref, 2)
    got = observe(eng)
    assert [body(x) for x in got[lead][0]] == [pushed_t(big)], got
    rc, o = raw(eng, 0, eng.n_rep, 0)
    assert rc == 0 and o.n_entries == 1 and o.cmd_bytes == 3008
    # 20 records of 3,032 B and two of 1,032 B: the head goes past one lap
    rest = [r for r in (3, 4, 5) + tuple(range(3)) if r != lead]
    for r, n, ln in zip(rest, (7, 7, 6, 2), (3000, 3000, 3000, 1000)):
        eng.push_proposals([r], [[O.Entry(type=0, cmd=b"y" * ln) for _ in range(n)]])
    zero = bytes(C.sizeof(RbeDroppedList))
    for flags in (0, 0x100):  # records only read the record's header: the same answer
        rc, o = raw(eng, 0, eng.n_rep, flags)
        assert rc == RBE_E_STATE, (flags, rc)
        assert bytes(o) == zero, "*out is zeroed"
    try:
        eng.get_dropped(lead)
        assert False, "rbe_get_dropped read a lapped record"
    except RuntimeError as e:
        assert e.rc == RBE_E_STATE
    assert raw(eng, 3, 3, 0)[0] == 0, "a range without that replica is served"
    return got


# ------------------------------------------------------------------ 8. spill heap too small
def spill_heap_too_small(make):
    """A round spill heap too short for a 65-entry list: the replica carries
    RBE_FAULT_NOMEM and lists no entries; the others are listed as usual."""
    eng = make(trace=True, drop_lists=True, n_groups=4, n_replicas=3, ext_inputs=True,
               spill_bytes=4096)
    big = [(0, j.to_bytes(2, "little")) for j in range(65)]
    eng.push_proposals([2], [big])
    ctxs = {r: (900 + r, r) for r in (0, 2, 7)}
    eng.push_read_index(list(ctxs), list(ctxs.values()))
    eng.step()
    got = observe(eng, counts=False)
    assert got == {r: ([], [c]) for r, c in ctxs.items()}
    ups = eng.updates()
    assert ups[2].n_dropped_entries == 65 and ups[2].fault & F_NOMEM
    assert all(not ups[r].fault for r in range(eng.n_rep) if r != 2)
    return got


# ------------------------------------------------------------------ 9. replica mode
def replica_mode(make, rounds=60):
    """Two engines over rep_world = 2 behind the batched transport loop: each
    lists only the replicas it steps, and the union of the lists satisfies the
    invariants of the driven scenario."""
    kw = dict(n_groups=4, n_replicas=3, ext_inputs=True)
    n, world = 3, 2
    engs = [make(trace=True, drop_lists=True, rep_world=world, rep_rank=r, **kw)
            for r in range(world)]
    rng, tr, seen = random.Random(3), Tracker(), []
    cmd = _seq_cmd(False)
    for rnd in range(rounds):
        ops = []
        for r in range(12):
            if rng.random() < 0.4:
                ops.append(("prop", r, [(0, cmd(rng)) for _ in range(rng.randrange(1, 4))]))
            if rng.random() < 0.3:
                ops.append(("read", r, ((rnd + 1) << 32 | r, rng.randrange(1 << 30))))
            if rnd > 25 and rng.random() < 0.05:
                ops.append(("xfer", r, rng.randrange(1, n + 1)))
        tr.on_ops(ops)
        for rank, e in enumerate(engs):
            apply_engine(e, [o for o in ops if owner(o[1] // n, o[1] % n, world) == rank])
        step_all(engs)
        union = {}
        for rank, e in enumerate(engs):
            got = observe(e, owned=lambda r: owner(r // n, r % n, world) == rank)
            assert not set(got) & set(union)
            union.update(got)
        tr.check(union)
        seen.append(union)
        deliver_batched(engs, n)
    assert tr.n_ent >= 10 and tr.n_ri >= 5 and tr.forwarded >= 1, (tr.n_ent, tr.n_ri, tr.forwarded)
    for e in engs:
        assert faults(e) == 0
    return seen


# ------------------------------------------------------------------ 10. off, arguments, lifetime
def off_and_arguments(make, raw):
    kw = dict(n_groups=4, n_replicas=3, ext_inputs=True)
    off = make(trace=True, **kw)
    off.step()
    assert raw(off, 0, off.n_rep, 0)[0] == RBE_E_STATE, "drop_lists = 0"
    try:
        off.get_dropped(0)
        assert False, "rbe_get_dropped with drop_lists = 0"
    except RuntimeError as e:
        assert e.rc == RBE_E_STATE
    eng = make(trace=True, drop_lists=True, **kw)
    R = eng.n_rep
    d = eng.collect_dropped(raw=True)  # before the first step: empty lists, RBE_OK
    assert len(d["replica"]) == 0 and list(d["ent_off"]) == [0] and list(d["ri_off"]) == [0]
    assert list(d["cmd_off"]) == [0]
    assert raw(eng, 0, R, 0, handle=False)[0] == RBE_E_INVALID  # null e
    assert raw(eng, 0, R, 0, out=False)[0] == RBE_E_INVALID     # null out
    assert raw(eng, 0, 0, 0)[0] == RBE_E_INVALID                 # count == 0
    assert raw(eng, R, 1, 0)[0] == RBE_E_INVALID                 # a range past n_rep
    assert raw(eng, 3, R, 0)[0] == RBE_E_INVALID
    for bad in (1, 2, 4, 0x80, 0x200, 1 << 31):  # RBE_ENTRIES_NO_CMDS is the only flag
        assert raw(eng, 0, R, bad)[0] == RBE_E_INVALID, bad
    batches = [[(0, b"r%d-%d" % (r, j)) for j in range(2)] for r in range(R)]
    eng.push_proposals(list(range(R)), batches)
    eng.push_read_index(list(range(R)), [(50 + r, r) for r in range(R)])
    eng.step()
    got = observe(eng)
    assert len(got) == R
    # a list stays valid across an rbe_collect_outbox and between
    # rbe_collect_step_begin and _end
    rc, o = raw(eng, 0, R, 0)
    assert rc == 0 and o.n_entries == 2 * R and o.n_read_indexes == R

    def snap():
        return (C.string_at(C.cast(o.entries, C.c_void_p), 72 * o.n_entries),
                C.string_at(C.cast(o.read_indexes, C.c_void_p), 16 * o.n_read_indexes),
                C.string_at(C.cast(o.ent_off, C.c_void_p), 8 * (o.n + 1)),
                C.string_at(C.cast(o.cmds, C.c_void_p), o.cmd_bytes))
    before = snap()
    eng.collect_outbox()
    assert snap() == before
    if hasattr(eng, "collect_step_begin"):
        plain = eng.collect_step()
        eng.collect_step_begin()
        mid = eng.collect_dropped(raw=True)
        late = eng.collect_step_end()
        for a, b in zip(plain, late):
            assert a.tobytes() == b.tobytes()
        whole = eng.collect_dropped(raw=True)
        for k in whole:
            assert whole[k].tobytes() == mid[k].tobytes(), k
    # after an import of a range the range lists no dropped entries but still
    # lists its dropped ReadIndexes (the snapshot's planes carry them)
    eng.import_groups(eng.export_groups(1, 2))
    after = observe(eng, counts=False)
    for r in range(R):
        want = ([], got[r][1]) if 3 <= r < 9 else got[r]
        assert after[r] == want, r
    assert faults(eng) == 0
    return got, after
