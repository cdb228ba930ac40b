"""Inbound transport past maxm / ecap on the CPU tier: W host builds of the
device step, each stepping the replicas it owns, exchange every cross-engine
message through rbe_push_messages or as frames through rbe_wire_ingest
(tests/ingest_cpu: the spilling forms of dragonboat_amd/csrc/rbe_ingest_spill.h).
Shapes whose catch-up Replicates carry more than ecap entries, or whose lists
hold more than maxm messages, must equal the oracle stepping all replicas in
one process; every one of them is refused with RBE_E_NOMEM by the forms the
HIP engine runs today (rbe_ingest.h, rbe_xchg.h), which do not spill.  The
engine is not wired to the spilling forms yet."""
import pytest

import oracle as O
import ingest_spill_scenarios as I
import session_scenarios as S
from dragonboat_amd.engine import RBE_E_NOMEM, InputError
from ingest_cpu.ingest import IngestCpu
from test_spill import LONG_ISO
from transport_util import run_transport


class ParentCpu(IngestCpu):
    """The receiving side as it was: full lists and arenas are refused."""

    def wire_ingest(self, data):
        return self.wire_ingest_parent(data)

    def push_messages(self, groups, msgs, ents, cmds=None):
        self.push_messages_parent(groups, msgs, ents, cmds)


@pytest.mark.parametrize("name", list(I.SHAPES))
def test_ingest_spill_parity_cpu(name):
    I.spill_parity(IngestCpu, name)


LONG_ISO_W2 = (LONG_ISO, 2, 420, {}, True)


def test_ingest_spill_long_iso_cpu():
    """test_spill.LONG_ISO (16 x 5, isolated for 150 rounds) over frames: the
    heal's catch-ups are far past ecap."""
    I.spill_parity(IngestCpu, "long_iso_w2_wire", shape=LONG_ISO_W2)


@pytest.mark.parametrize("name", list(I.SHAPES) + ["long_iso_w2_wire"])
def test_shape_was_refused_before(name):
    """None of the shapes is vacuous: the refusing form of the two calls
    answers RBE_E_NOMEM somewhere in the same run."""
    kw, world, rounds, extra, wire = I.SHAPES.get(name, LONG_ISO_W2)
    engs = I.engines(ParentCpu, world, kw, extra)
    with pytest.raises(InputError) as ei:
        run_transport(engs, O.Harness(**kw), kw["n_replicas"], rounds, wire=wire)
    assert ei.value.rc == RBE_E_NOMEM


@pytest.mark.parametrize("name,rounds", [("iso70_w2_wire", 130), ("maxm1_w2_push", 100)])
def test_ingest_spill_push_equals_wire_cpu(name, rounds):
    I.push_equals_wire(IngestCpu, name, rounds)


def test_push_and_wire_leave_the_same_spill_heap():
    """The placement rule is written twice, in rbe_ingest_spill.h
    ingest_sender_spill (frames, sorted runs) and in rbe_xchg.h
    messages_to_records (push, exchange records); this holds the two together:
    the same batch through either leaves the same bytes in the round spill
    heap."""
    kw = dict(n_groups=4, n_replicas=3, wl_enabled=False)
    a, b = [IngestCpu(trace=True, rep_world=2, rep_rank=0, maxm=2, ecap=4, **kw) for _ in range(2)]
    for e in (a, b):
        e.step()
    # node 2 → node 1 of group 0: three Replicates (a list past maxm = 2), the
    # second and third past the arena of 4
    gs, ms, es, cs = [], [], [], []
    for n in (3, 5, 2):
        g, m, e, c = I.catch_up(n, False)
        gs, ms, es, cs = gs + g, ms + m, es + e, cs + c
    import wire as W
    batch = []
    for n in (3, 5, 2):
        m = dict(type=12, to=1, cluster_id=1, term=1, log_term=0, log_index=0, commit=0,
                 reject=False, hint=0, hint_high=0)
        m["from"] = 2
        batch.append((m, [dict(term=1, index=i + 1, cmd=b"%d" % i) for i in range(n)]))
    frames = W.frame(W.batch_bytes(batch, 0, "", 0))
    a.push_messages(gs, ms, es, cs)
    b.wire_ingest(frames)
    ha, hb = a.spill_heap(0), b.spill_heap(0)
    assert ha == hb
    # the list's block (3 Msg of 64 B) and 5 + 2 entries of 32 B
    assert a.spill_stats()["spill_peak_bytes"] == b.spill_stats()["spill_peak_bytes"] == 3 * 64 + 7 * 32
    assert any(ha[:3 * 64 + 7 * 32])
    for e in (a, b):
        e.step()
        assert e.faults()[0] == 0
    va, vb = a.views(), b.views()
    assert all(I.view_diff(va[i], vb[i]) is None for i in range(len(va)))


@pytest.mark.parametrize("wire", [False, True])
def test_ingest_spill_session_entries_cpu(wire):
    """Heap Cmds and session fields with an arena of one entry: a forwarded
    Propose's or Replicate's entries spill, their records go to the payload
    heap, and every Cmd reads back."""
    made = []

    def make(**kw):
        made.append(IngestCpu(ecap=1, **kw))
        return made[-1]

    S.session_over_transport(make, 2, wire=wire)
    assert all(e.inbound_spill_bytes > 0 for e in made), [e.inbound_spill_bytes for e in made]


@pytest.mark.parametrize("wire", [False, True])
def test_ingest_spill_refused_when_the_share_is_short(wire):
    I.refusal(IngestCpu, wire)

