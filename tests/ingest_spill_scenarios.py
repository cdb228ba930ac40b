"""Inbound transport past maxm / ecap: the scenarios of
tests/test_ingest_spill.py (the host build tests/ingest_cpu), each against the
oracle harness.  `make(**cfg)` builds the engine under test, so an engine
behind the C ABI can run them too.

A replica that was isolated for longer than ecap rounds is caught up with one
Replicate of more than ecap entries (raft.go:709-740: sized by MaxEntrySize
alone), and with small capacities a (sender, destination) list holds more than
maxm messages.  Peer.Handle takes both (peer.go:186-198), so the spilling
forms of rbe_wire_ingest and rbe_push_messages (rbe_ingest_spill.h) keep them
in the round spill heap, in the layout a local sender's step leaves
(rbe_spill.h).  Every shape below is refused with RBE_E_NOMEM by the forms
that do not spill."""
import pytest

import oracle as O
from dragonboat_amd.engine import RBE_E_NOMEM, InputError, RbeMessage, make_entry
from parity_util import view_diff
from transport_util import deliver, deliver_wire, run_transport

ISO_70_50 = dict(n_groups=4, n_replicas=3, wl_enabled=True, wl_start_round=20, iso_period=70,
                 iso_len=50, iso_mod=1)
ISO_40_20 = dict(n_groups=4, n_replicas=3, wl_enabled=True, wl_start_round=20, iso_period=40,
                 iso_len=20, iso_mod=1)
MIXED = dict(n_groups=12, n_replicas=5, check_quorum=True, quiesce=True, wl_enabled=True,
             wl_start_round=25, wl_active_mod=2, wl_read_permille=500, iso_period=37, iso_len=20,
             iso_mod=2, seed=12345)

# name: (config, world, rounds, capacities, wire)
SHAPES = {
    # a catch-up Replicate of ~50 entries against the default ecap of 32
    "iso70_w2_wire": (ISO_70_50, 2, 160, {}, True),
    "iso70_w3_push": (ISO_70_50, 3, 160, {}, False),
    # 5 replicas, CheckQuorum, every other group isolated
    "n5_cq_w3_wire": (dict(n_groups=6, n_replicas=5, check_quorum=True, wl_enabled=True,
                           wl_start_round=20, iso_period=70, iso_len=50, iso_mod=2), 3, 220, {},
                      True),
    # small capacities: lists past maxm as well
    "ecap4_w2_wire": (ISO_40_20, 2, 100, dict(ecap=4, ring=8), True),
    "maxm1_w2_push": (ISO_40_20, 2, 100, dict(maxm=1, ecap=1, ring=8), False),
    "mixed_tiny_w2_push": (MIXED, 2, 300, dict(maxm=1, ecap=1, rtr_cap=1, dri_cap=1, rq_cap=1,
                                               ring=8), False),
    "mixed_tiny_w2_wire": (MIXED, 2, 300, dict(maxm=1, ecap=1, rtr_cap=1, dri_cap=1, rq_cap=1,
                                               ring=8), True),
}


def engines(make, world, kw, extra):
    return [make(trace=True, rep_world=world, rep_rank=r, **kw, **extra) for r in range(world)]


def faults(e):
    return e.fault_summary()[0] if hasattr(e, "fault_summary") else e.faults()[0]


def close(engs):
    for e in engs:
        if hasattr(e, "close"):
            e.close()


def step_all(engs):
    """One round of every engine (the isolation epochs' leader bits ORed first)."""
    iso = [e.iso_leaders() for e in engs]
    if iso[0] is not None:
        bits = iso[0].copy()
        for b in iso[1:]:
            bits |= b
        for e in engs:
            e.set_iso_leaders(bits)
    for e in engs:
        e.step()


def peaks_without_hops(make, world, kw, extra, rounds):
    """The round spill heap peak of each engine stepped with no transport hop
    at all: what its own senders reach on their own."""
    engs = engines(make, world, kw, extra)
    for _ in range(rounds):
        step_all(engs)
    out = [e.spill_stats()["spill_peak_bytes"] for e in engs]
    close(engs)
    return out


# The shape whose engines, stepped with no hop at all, spill MORE than in the
# connected run (replicas that never hear from their peers keep re-sending):
# measured on the host build, peaks 736 / 768 bytes connected against 928 / 896
# alone, although every heal's catch-up spills inbound (1536 / 928 bytes over
# the run).  There the peak comparison cannot show the inbound spill.
PEAK_BELOW_ALONE = ("ecap4_w2_wire",)


def spill_parity(make, name, every=25, shape=None):
    """The shape over the transport equals the oracle, nothing faults, no tier
    ran out, and inbound lists or entries did spill: some engine's spill peak
    lies above what the same engines reach when stepped with no hop at all
    (rbe_spill_stats shows only the peak), and an engine that counts what its
    inbound batches took of the spill heap (the host build: SpillCtl::used
    around every hop) shows it directly."""
    kw, world, rounds, extra, wire = shape or SHAPES[name]
    engs = engines(make, world, kw, extra)
    ref = O.Harness(**kw)
    d, moved = run_transport(engs, ref, kw["n_replicas"], rounds, every=every, wire=wire)
    assert d is None, f"{name}: first divergence {d}"
    assert moved > rounds, "the transport carried (almost) nothing"
    stats = [e.spill_stats() for e in engs]
    for e, st in zip(engs, stats):
        assert faults(e) == 0
        assert st["oom"] == 0
    got = [st["spill_peak_bytes"] for st in stats]
    inbound = [getattr(e, "inbound_spill_bytes", None) for e in engs]
    close(engs)
    alone = peaks_without_hops(make, world, kw, extra, rounds)
    print(f"{name}: spill peaks {got}, without hops {alone}, inbound spill bytes {inbound}")
    if inbound[0] is not None:
        assert any(inbound), "no inbound batch spilled"
        assert all(g > 0 for g, i in zip(got, inbound) if i)
    if name not in PEAK_BELOW_ALONE:
        assert any(g > a for g, a in zip(got, alone)), (got, alone)
    else:
        assert inbound[0] is not None, "only the direct count can show this shape's inbound spill"


def push_equals_wire(make, name, rounds):
    """The same rounds through rbe_push_messages and through rbe_wire_ingest
    leave identical replica views on both engine sets, round by round."""
    kw, world, _, extra, _ = SHAPES[name]
    a, b = engines(make, world, kw, extra), engines(make, world, kw, extra)
    n, n_rep = kw["n_replicas"], kw["n_groups"] * kw["n_replicas"]
    total = 0
    for rnd in range(rounds):
        step_all(a)
        step_all(b)
        deliver(a, n, n_rep)
        total += deliver_wire(b)[0]
        va, vb = [e.views() for e in a], [e.views() for e in b]
        for r in range(world):
            for i in range(n_rep):
                assert view_diff(va[r][i], vb[r][i]) is None, (rnd, r, i)
    assert total > rounds
    pa = [e.spill_stats()["spill_peak_bytes"] for e in a]
    pb = [e.spill_stats()["spill_peak_bytes"] for e in b]
    assert pa == pb, (pa, pb)
    for e in a + b:
        assert faults(e) == 0
    close(a + b)
    return a, b


def catch_up(n_entries, wire):
    """A hand-built catch-up: node 2 → node 1 of group 0, one Replicate of
    n_entries entries after index 0.  Returns the push arguments, or the
    frame's bytes."""
    if wire:
        import wire as W
        m = dict(type=12, to=1, cluster_id=1, term=1, log_term=0, log_index=0, commit=0,
                 reject=False, hint=0, hint_high=0)
        m["from"] = 2
        ents = [dict(term=1, index=i + 1, cmd=b"%d" % i) for i in range(n_entries)]
        return W.frame(W.batch_bytes([(m, ents)], 0, "", 0))
    rep = RbeMessage(type=12, to=1, from_=2, term=1, log_index=0, n_entries=n_entries)
    ents = [make_entry(cmd=b"%d" % i, index=i + 1, term=1) for i in range(n_entries)]
    return [0], [rep], ents, [b"%d" % i for i in range(n_entries)]


def refusal(make, wire):
    """A spill heap share too small for the catch-up: the hop is refused whole
    with RBE_E_NOMEM, the exhaustion flag stays clear, no replica faults, and
    after one more step the engine equals a twin that was handed an empty
    batch at that hop.

    rep_world = 2 and spill_bytes = 2048 give each rank 64 granules; the
    Replicate's 40 entries are more than ecap = 32, so they need 80."""
    kw = dict(n_groups=4, n_replicas=3, wl_enabled=False)
    e, twin = [make(trace=True, rep_world=2, rep_rank=0, spill_bytes=2048, **kw) for _ in range(2)]
    for x in (e, twin):
        x.step()
        # a first hop that fits
        if wire:
            x.wire_ingest(catch_up(3, True))
        else:
            x.push_messages(*catch_up(3, False))
        x.step()
    assert e.spill_stats()["spill_peak_bytes"] == 0  # its own steps never spilled
    with pytest.raises(InputError) as ei:
        if wire:
            e.wire_ingest(catch_up(40, True))
        else:
            e.push_messages(*catch_up(40, False))
    assert ei.value.rc == RBE_E_NOMEM
    if wire:
        twin.wire_ingest(b"")
    else:
        twin.push_messages([], [], [])
    st = e.spill_stats()
    assert st["oom"] == 0 and st["spill_peak_bytes"] == 0
    for x in (e, twin):
        x.step()
    assert faults(e) == 0
    ve, vt = e.views(), twin.views()
    for i in range(len(ve)):
        assert view_diff(ve[i], vt[i]) is None, i
    # a catch-up that fits the share is taken: 30 entries past a used arena
    both = [catch_up(3, wire), catch_up(31, wire)]
    if wire:
        e.wire_ingest(both[0] + both[1])
    else:
        e.push_messages(*[a + b for a, b in zip(*both)])
    st = e.spill_stats()
    assert st["oom"] == 0 and st["spill_peak_bytes"] == 31 * 32
    e.step()
    assert faults(e) == 0
    close([e, twin])
