"""Batched outbox (rbe_collect_outbox): scenarios shared by the CPU tier
(tests/test_outbox_collect.py, the host build of tests/outbox_cpu) and the GPU
tier (tests/test_gpu_outbox_collect.py, the HIP engine through the C ABI).
`make(**cfg)` builds the engine; `full_only=True` asks for full-table mode.

The oracle of the gather is rbe_get_outbox itself: every round the batched
lists must be the concatenation of outbox(r) over the senders, message for
message, entry for entry and Cmd byte for Cmd byte (the Cmds 16-B padded with
zero bytes, the one deliberate difference).  The oracle of the protocol is the
harness under oracle/: the engines run in lockstep with it."""
import ctypes as C
import random

import numpy as np

import oracle as O
from dragonboat_amd.engine import RBE_E_INVALID, RBE_E_STATE, RbeOutboxList, outbox_list_split
from ingest_spill_scenarios import ISO_40_20, MIXED, step_all
from input_util import apply_engine, apply_oracle
from parity_util import view_diff
from transport_util import deliver, owner

M_PROPOSE, M_REPLICATE, M_INSTALL_SNAPSHOT, M_QUIESCE = 7, 12, 16, 21


def faults(e):
    return e.fault_summary()[0] if hasattr(e, "fault_summary") else e.faults()[0]


def check_raw(d, cmds):
    """The offsets of the raw lists are consistent; each cmd_off is a multiple
    of 16, a Cmd's first 16 bytes are its record's, and the pad bytes are zero."""
    n, nm, ne = len(d["replica"]), len(d["messages"]), len(d["entries"])
    rep = [int(r) for r in d["replica"]]
    assert rep == sorted(set(rep))
    moff, eoff = d["msg_off"], d["ent_off"]
    assert len(moff) == n + 1 and int(moff[0]) == 0 and int(moff[-1]) == nm
    assert (np.diff(moff.astype(np.int64)) > 0).all(), "a listed sender has a message"
    assert len(eoff) == nm + 1 and int(eoff[0]) == 0 and int(eoff[-1]) == ne
    assert (np.diff(eoff.astype(np.int64)) >= 0).all()
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


def sender_lists(eng, r):
    """outbox(r) cut into messages with their entries and Cmds."""
    msgs, ents, cmds = eng.outbox(r, 64, 64, 4096)  # (grown when short)
    out, ei = [], 0
    for m in msgs:
        ne = m.n_entries
        out.append((m, ents[ei:ei + ne], cmds[ei:ei + ne]))
        ei += ne
    assert ei == len(ents)
    return out


def expected(per, first, count, keep):
    """{sender: (message bytes, entry bytes, Cmds)} of senders [first, first +
    count) from the per-sender lists, keeping the messages keep(sender, m)
    allows; a sender left without a message is not listed."""
    want = {}
    for r, lst in per.items():
        if not first <= r < first + count:
            continue
        ms, es, cs = [], [], []
        for m, e, c in lst:
            if keep(r, m):
                ms.append(bytes(m))
                es.extend(bytes(x) for x in e)
                cs.extend(c)
        if ms:
            want[r] = (ms, es, cs)
    return want


def got_lists(eng, first, count, cmds=True, **kw):
    d = eng.collect_outbox(first, count, cmds=cmds, raw=True, **kw)
    check_raw(d, cmds)
    got = {}
    for r, (m, e, c) in outbox_list_split(d).items():
        got[r] = ([bytes(x) for x in m], [bytes(x) for x in e], c)
    return got


def no_cmds(want):
    return {r: (m, e, None) for r, (m, e, c) in want.items()}


class Checker:
    """Every round: the whole engine and an inner range that starts and ends
    mid-group, both Cmd modes, against the per-replica call."""

    def __init__(self, eng, n, owned=None):
        self.eng, self.n = eng, n
        self.owned = owned or (lambda r: True)
        self.types, self.msgs, self.ents = set(), 0, 0
        self.longest_list = self.longest_ents = 0

    def per_sender(self):
        return {r: sender_lists(self.eng, r) for r in range(self.eng.n_rep) if self.owned(r)}

    def after_round(self):
        eng, n = self.eng, self.n
        per = self.per_sender()
        for r, lst in per.items():
            by_dst = {}
            for m, e, _ in lst:
                self.types.add(m.type)
                self.msgs += 1
                self.ents += len(e)
                by_dst[m.to] = by_dst.get(m.to, 0) + (m.type != M_QUIESCE)
                self.longest_ents = max(self.longest_ents, len(e))
            self.longest_list = max([self.longest_list] + list(by_dst.values()))
        every = lambda r, m: True
        ranges = [(0, eng.n_rep)]
        if eng.n_rep > 2 * n + 2:
            ranges.append((n + 1, eng.n_rep - 2 * n - 2))
        for first, count in ranges:
            want = expected(per, first, count, every)
            assert got_lists(eng, first, count) == want, (first, count)
            assert got_lists(eng, first, count, cmds=False) == no_cmds(want), (first, count)
        return per


def lockstep(eng, ref, rounds, each=None, ids=None, n=None):
    for rnd in range(rounds):
        eng.step()
        ref.step()
        ev, hv = eng.views(), ref.views()
        for i in range(len(hv)):
            h = hv[i]
            if ids is not None:
                from test_node_ids import mapped
                h = mapped(h, ids[i // n])
            d = view_diff(ev[i], h)
            assert d is None, f"first divergence at round {rnd}, replica {i}: {d}"
        if each:
            each()


C2_12 = dict(n_groups=12, n_replicas=3, wl_enabled=True, wl_start_round=30)
C4_12 = dict(n_groups=12, n_replicas=3, quiesce=True, wl_enabled=True, wl_start_round=30,
             wl_active_mod=2, wl_read_permille=900)
C3_7 = dict(n_groups=4, n_replicas=7, check_quorum=True, wl_enabled=True, wl_start_round=40,
            iso_period=50, iso_len=30, iso_mod=2)
SNAP = dict(n_groups=6, n_replicas=3, check_quorum=True, wl_enabled=True, wl_start_round=20,
            iso_period=60, iso_len=40, iso_mod=1, snapshot_entries=16, compaction_overhead=4)

# name: (config, rounds, message types that must occur)
EQUAL = {
    "C2": (C2_12, 70, {M_REPLICATE, 14}),  # from round 1: RequestVote (14) of the first elections
    "C4_quiesce": (C4_12, 230, {M_REPLICATE, M_QUIESCE}),  # the first notices: round 215
    "C3_groups_of_7": (C3_7, 110, {M_REPLICATE}),
    "snapshots": (SNAP, 130, {M_REPLICATE, M_INSTALL_SNAPSHOT}),  # the first: round 102
}


def equal_to_per_replica(make, name):
    kw, rounds, types = EQUAL[name]
    eng, ref = make(trace=True, **kw), O.Harness(**kw)
    assert eng.collect_outbox() == {}  # before the first step
    chk = Checker(eng, kw["n_replicas"])
    lockstep(eng, ref, rounds, chk.after_round)
    assert faults(eng) == 0
    assert types <= chk.types, (types, chk.types)
    assert chk.msgs > rounds and chk.ents > 0
    # with one engine every destination is local: nothing is remote
    assert eng.collect_outbox(remote_only=True) == {}


def node_ids_any_order(make):
    """Node ids that do not ascend with the slots: From, To and the hints go
    through the group's id row, the order stays the slot order."""
    from test_node_ids import random_ids
    kw = dict(C3_7, n_replicas=5, n_groups=6, xfer_period=7, xfer_mod=2)
    n = kw["n_replicas"]
    ids = [list(reversed(row)) for row in random_ids(kw["n_groups"], n, seed=9)]
    eng, ref = make(trace=True, **kw), O.Harness(**kw)
    eng.set_node_ids(0, ids)
    chk = Checker(eng, n)
    seen = set()

    def each():
        for r, lst in chk.after_round().items():
            for m, _, _ in lst:
                assert m.from_ == ids[r // n][r % n] and m.to in ids[r // n]
                seen.add(m.type)

    lockstep(eng, ref, 90, each, ids=ids, n=n)
    assert faults(eng) == 0
    assert {M_REPLICATE, 14} <= seen, seen


TINY = dict(maxm=1, rtr_cap=1, dri_cap=1, ecap=1, rq_cap=1, ring=8)
# name: (config, capacities, rounds)
SPILL = {
    "iso_40_20": (ISO_40_20, dict(maxm=1, ecap=1, ring=8), 100),
    "mixed_tiny": (MIXED, TINY, 120),
}


def spilled(make, name, full_only=False):
    """Lists past maxm and entries past ecap are read out of the round spill
    heap.  A run that never spills proves nothing: the conditions are asserted."""
    kw, caps, rounds = SPILL[name]
    eng, ref = make(trace=True, full_only=full_only, **caps, **kw), O.Harness(**kw)
    chk = Checker(eng, kw["n_replicas"])
    lockstep(eng, ref, rounds, chk.after_round)
    assert faults(eng) == 0
    st = eng.spill_stats()
    assert st["oom"] == 0 and st["spill_peak_bytes"] > 0
    assert chk.longest_list > caps["maxm"], "no list of more than maxm messages was collected"
    assert chk.longest_ents > caps["ecap"], "no message with more entries than ecap was collected"


CMD_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 1000)


def cmds_and_heap_records(make):
    """Host proposals of every Cmd length around the inline limit (16 B) and
    the one-lane limit of the Cmd copy (64 B), with and without session fields,
    at leaders (Replicates) and at followers (forwarded Proposes that carry
    entries with Index 0): every byte and every pad byte."""
    kw = dict(n_groups=6, n_replicas=3, ext_inputs=True)
    eng, ref = make(trace=True, heap_bytes=1 << 20, **kw), O.Harness(**kw)
    n, rng = 3, random.Random(5)
    chk = Checker(eng, n)
    lockstep(eng, ref, 40)  # elections
    lens_seen = {M_REPLICATE: set(), M_PROPOSE: set()}
    session_seen = {True: set(), False: set()}
    pushed = set()
    for rnd in range(2 * len(CMD_LENS) + 6):
        ops = []
        if rnd < 2 * len(CMD_LENS):
            ln, sess = CMD_LENS[rnd % len(CMD_LENS)], rnd >= len(CMD_LENS)
            for r in range(eng.n_rep):  # leaders and followers alike
                ents = []
                for _ in range(1 + (r % 2)):
                    e = O.Entry(type=0, cmd=rng.randbytes(ln))
                    if sess:
                        e.key, e.client_id = rng.randrange(1, 1 << 60), rng.randrange(1, 1 << 20)
                        e.series_id, e.responded_to = rng.randrange(1, 1 << 30), rng.randrange(1 << 10)
                    pushed.add(bytes(e.cmd))
                    ents.append(e)
                ops.append(("prop", r, ents))
        apply_engine(eng, ops)
        apply_oracle(ref, ops)
        lockstep(eng, ref, 1)
        for r, lst in chk.after_round().items():
            for m, es, cs in lst:
                for e, c in zip(es, cs):
                    assert m.type in (M_REPLICATE, M_PROPOSE)
                    if m.type == M_PROPOSE:
                        assert e.index == 0
                    lens_seen[m.type].add(len(c))
                    session_seen[bool(e.key)].add(len(c))
                    assert len(c) <= 16 or c in pushed
    assert faults(eng) == 0
    for t in lens_seen:
        assert set(CMD_LENS) <= lens_seen[t], (t, sorted(lens_seen[t]))
    assert set(CMD_LENS) <= session_seen[True] and set(CMD_LENS) <= session_seen[False]


def staged_records(make):
    """A call between a proposal's push and the step that takes it: the records
    still staged for that step are uploaded first and change nothing of what
    the last round's outboxes hold."""
    kw = dict(n_groups=4, n_replicas=3, ext_inputs=True)
    eng, ref = make(trace=True, heap_bytes=1 << 20, **kw), O.Harness(**kw)
    chk = Checker(eng, 3)
    lockstep(eng, ref, 40)
    for rnd in range(6):
        ops = [("prop", r, [O.Entry(type=0, cmd=bytes([rnd, r]) * 100, key=7 + r)])
               for r in range(eng.n_rep)]
        apply_engine(eng, ops)
        apply_oracle(ref, ops)
        chk.after_round()  # staged, not stepped
        lockstep(eng, ref, 1, chk.after_round)
    assert chk.ents > 0 and faults(eng) == 0


def _rc(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except RuntimeError as e:
        return getattr(e, "rc", None)
    return 0


def lapped_record(make, raw):
    """A heap record a later lap overwrote.  The heap never laps a record a
    live entry names (a push that would is refused), so a sender's own outbox
    cannot get there in one engine's life; a resume can: engine A's checkpoint
    without a heap section, whose outbox holds a Replicate of a 3,000-byte
    record at heap position 0, is resumed on engine B, whose 64 KiB heap has
    gone round more than once.  The whole call is RBE_E_STATE with *out zeroed,
    and rbe_get_outbox refuses the same replica.
    `raw(eng, first, count, flags, dst_rank)` returns (code, RbeOutboxList)."""
    kw = dict(n_groups=2, n_replicas=3, ext_inputs=True)
    a, ref = make(trace=True, heap_bytes=64 << 10, **kw), O.Harness(**kw)
    lockstep(a, ref, 40)
    lead = [r for r, v in enumerate(ref.views()) if v.role == O.LEADER][0]
    ops = [("prop", lead, [O.Entry(type=0, cmd=b"x" * 3000)])]
    apply_engine(a, ops)
    apply_oracle(ref, ops)
    lockstep(a, ref, 1)
    got = a.collect_outbox(lead, 1)
    assert any(e.cmd_len == 3000 for e in got[lead][1]), "the Replicate carries the record"
    snap = a.export_groups()
    b = make(trace=True, heap_bytes=64 << 10, **kw)
    ok = 0
    for _ in range(60):  # 3,032 B a record: 44 of them are two laps
        try:
            b.push_proposals([0, 3], [[O.Entry(type=0, cmd=b"y" * 3000)]] * 2)
            ok += 2
        except RuntimeError:
            pass  # (a live record in the way: refused whole, try after the step)
        b.step()
        if ok >= 44:
            break
    assert ok >= 44, ok
    b.import_groups(snap, resume=True)
    assert _rc(b.outbox, lead) != 0, "rbe_get_outbox refuses the lapped record"
    zero = bytes(C.sizeof(RbeOutboxList))
    for flags in (0, 0x100):  # records only read the record's header: the same answer
        rc, o = raw(b, 0, b.n_rep, flags, -1)
        assert rc == RBE_E_STATE, (flags, rc)
        assert bytes(o) == zero, "*out is zeroed"
    # a range without that sender is served
    rest = [r for r in range(b.n_rep) if r // 3 != lead // 3]
    assert raw(b, rest[0], len(rest), 0, -1)[0] == 0


def deliver_batched(engs, n):
    """One transport hop in place of transport_util.deliver: each rank makes
    one collect_outbox(remote_only=True, dst_rank=d) per destination rank and
    the lists go to d's push_messages as they are.  Returns the messages moved."""
    world = len(engs)
    batches = [([], [], [], []) for _ in range(world)]
    moved = 0
    for rank, e in enumerate(engs):
        for d in range(world):
            if d == rank:
                continue
            gs, ms, es, cs = batches[d]
            for r, (m, en, cm) in e.collect_outbox(remote_only=True, dst_rank=d).items():
                assert owner(r // n, r % n, world) == rank
                assert all(owner(r // n, x.to - 1, world) == d for x in m)
                gs.extend([r // n] * len(m))
                ms.extend(m)
                es.extend(en)
                cs.extend(cm)
                moved += len(m)
    for rank, e in enumerate(engs):
        e.push_messages(*batches[rank])
    return moved


def replica_mode(make, kw, world, rounds, extra, every=25):
    """W engines behind the batched transport loop are bit-exact with the
    oracle, and the loop moves what transport_util.deliver moves on a twin set
    of engines run beside it.  Every round the per-rank calls, the unfiltered
    call and the remote-only call equal the filtered per-replica lists.  (A rank
    lists its own senders only: what push_messages delivered for a remote
    sender, spilled past maxm / ecap or not, is the next step's to read, and
    the parity with the oracle shows that it arrived whole.)"""
    n = kw["n_replicas"]
    engs = [make(trace=True, rep_world=world, rep_rank=r, **kw, **extra) for r in range(world)]
    twins = [make(trace=True, rep_world=world, rep_rank=r, **kw, **extra) for r in range(world)]
    ref = O.Harness(**kw)
    n_rep = len(ref.views())
    moved = moved_twin = 0
    for done in range(1, rounds + 1):
        step_all(engs)
        step_all(twins)
        ref.step()
        for rank, e in enumerate(engs):
            own = lambda r: owner(r // n, r % n, world) == rank
            per = Checker(e, n, own).per_sender()
            dst = lambda r, m: owner(r // n, m.to - 1, world)
            assert got_lists(e, 0, e.n_rep) == expected(per, 0, e.n_rep, lambda r, m: True)
            assert got_lists(e, 0, e.n_rep, remote_only=True) == \
                expected(per, 0, e.n_rep, lambda r, m: dst(r, m) != rank)
            first, count = n + 1, e.n_rep - 2 * n - 2
            for d in range(world):
                if d != rank:
                    assert got_lists(e, first, count, cmds=False, dst_rank=d) == \
                        no_cmds(expected(per, first, count, lambda r, m: dst(r, m) == d))
        moved += deliver_batched(engs, n)
        moved_twin += deliver(twins, n, n_rep)
        if done % every and done != rounds:
            continue
        hv = ref.views()
        evs = [e.views() for e in engs]
        for r in range(n_rep):
            d = view_diff(evs[owner(r // n, r % n, world)][r], hv[r])
            assert d is None, f"first divergence {(done, r) + d}"
    assert moved == moved_twin and moved > rounds, (moved, moved_twin)
    for e in engs + twins:
        assert faults(e) == 0
    return engs


def arguments_and_lifetime(make, raw):
    kw = dict(C2_12, n_groups=4)
    eng, ref = make(trace=True, **kw), O.Harness(**kw)
    # before the first step: empty lists, RBE_OK
    d = eng.collect_outbox(raw=True)
    assert len(d["replica"]) == 0 and list(d["msg_off"]) == [0] and list(d["ent_off"]) == [0]
    assert list(d["cmd_off"]) == [0] and len(d["messages"]) == 0
    lockstep(eng, ref, 50)
    R = eng.n_rep
    assert raw(eng, 0, R, 0, -1)[0] == 0
    assert raw(eng, 0, R, 0, -1, handle=False)[0] == RBE_E_INVALID  # null e
    assert raw(eng, 0, R, 0, -1, out=False)[0] == RBE_E_INVALID     # null out
    assert raw(eng, 0, 0, 0, -1)[0] == RBE_E_INVALID                 # count == 0
    assert raw(eng, R, 1, 0, -1)[0] == RBE_E_INVALID                 # a range past n_rep
    assert raw(eng, 3, R, 0, -1)[0] == RBE_E_INVALID
    for bad in (2, 4, 0x80, 0x200, 1 << 31):  # any other bit (2: RBE_COLLECT_SKIP_LOCAL)
        assert raw(eng, 0, R, bad, -1)[0] == RBE_E_INVALID, bad
    assert raw(eng, 0, R, 1 | 0x100, -1)[0] == 0
    for rank in (0, 1, -2):  # rep_world <= 1: dst_rank must be -1
        assert raw(eng, 0, R, 0, rank)[0] == RBE_E_INVALID, rank
    two = make(trace=True, rep_world=3, rep_rank=1, **kw)
    two.step()
    for rank, want in ((-1, 0), (0, 0), (2, 0), (1, RBE_E_INVALID), (3, RBE_E_INVALID),
                       (-2, RBE_E_INVALID)):
        assert raw(two, 0, two.n_rep, 1, rank)[0] == want, rank
    # a list stays readable after a collection of entries
    rc, o = raw(eng, 0, R, 0, -1)
    assert rc == 0 and o.n_messages > 0
    before = (C.string_at(C.cast(o.messages, C.c_void_p), o.n_messages * 80),
              C.string_at(C.cast(o.msg_off, C.c_void_p), 8 * (o.n + 1)),
              C.string_at(C.cast(o.entries, C.c_void_p), 72 * o.n_entries))
    if hasattr(eng, "collect_entries"):
        eng.collect_entries()
        eng.collect_entries(which=2)
        after = (C.string_at(C.cast(o.messages, C.c_void_p), o.n_messages * 80),
                 C.string_at(C.cast(o.msg_off, C.c_void_p), 8 * (o.n + 1)),
                 C.string_at(C.cast(o.entries, C.c_void_p), 72 * o.n_entries))
        assert after == before
    # between rbe_collect_step_begin and _end: both results intact
    if hasattr(eng, "collect_step_begin"):
        plain = eng.collect_step()
        whole = eng.collect_outbox(raw=True)
        eng.collect_step_begin()
        mid = eng.collect_outbox(raw=True)
        late = eng.collect_step_end()
        for a, b in zip(plain, late):
            assert a.tobytes() == b.tobytes()
        for k in whole:
            assert whole[k].tobytes() == mid[k].tobytes(), k
    assert faults(eng) == 0
