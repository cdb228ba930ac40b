"""Inbound transport past maxm / ecap on the HIP engine: rbe_wire_ingest
(both forms) and rbe_push_messages keep a (sender, destination) list of more
than maxm messages and a message's entries past the sender's ecap in this
engine's share of the round spill heap (rbe_ingest_spill.h), as the host build
tests/ingest_cpu does.  The scenarios of ingest_spill_scenarios.py (CPU twin:
test_ingest_spill.py) on the device, each against the oracle, and beside the
host build: the spill peaks and the inbound spill bytes must be the host
build's, since the granules are placed by one rule without atomics.

Every one of the parity shapes was refused with RBE_E_NOMEM before the engine
spilled (test_ingest_spill.test_shape_was_refused_before shows it on the
refusing forms)."""
import pytest

import ingest_spill_scenarios as I
import oracle as O
import session_scenarios as S
from dragonboat_amd.engine import RBE_E_NOMEM, Engine, InputError
from ingest_cpu.ingest import IngestCpu
from test_transport import CASES
from transport_util import run_transport

pytestmark = pytest.mark.gpu

# the shape that faulted the first wiring: every
# message capacity at 1 over frames
SHAPES = dict(I.SHAPES)
SHAPES["maxm1_w2_wire"] = (I.ISO_40_20, 2, 100, dict(maxm=1, ecap=1, ring=8), True)


class Recorded(Engine):
    """An engine that keeps its figures as they were when the scenario closed it."""

    def close(self):
        if getattr(self, "h", None):
            self.final = _figures(self)
        super().close()


class _Made:
    """make(**kw) that keeps what it built: the HIP engine, or the host build."""

    def __init__(self, host=False):
        self.host, self.engs = host, []

    def __call__(self, **kw):
        e = IngestCpu(**kw) if self.host else Recorded(device=0, **kw)
        self.engs.append(e)
        return e

    def figures(self, n):
        """(spill peak bytes, inbound spill bytes) of the first n engines made."""
        return [getattr(e, "final", None) or _figures(e) for e in self.engs[:n]]


def _figures(e):
    return e.spill_stats()["spill_peak_bytes"], e.inbound_spill_bytes


def _make(**kw):
    return Engine(device=0, **kw)


@pytest.fixture(scope="module")
def host_figures():
    """The host build's figures per shape, computed once per shape."""
    cache = {}

    def get(name):
        if name not in cache:
            made = _Made(host=True)
            I.spill_parity(made, name, shape=SHAPES[name])
            cache[name] = made.figures(SHAPES[name][1])
        return cache[name]

    return get


def _parity(name, host_figures):
    made = _Made()
    I.spill_parity(made, name, shape=SHAPES[name])
    got, exp = made.figures(SHAPES[name][1]), host_figures(name)
    print(f"{name}: (spill peak, inbound spill) bytes per engine {got}, host build {exp}")
    assert any(inb for _, inb in got), "no inbound batch spilled"
    assert got == exp


@pytest.mark.parametrize("name", list(SHAPES))
def test_gpu_ingest_spill_parity(gpu_available, monkeypatch, host_figures, name):
    """Bit-exact with the oracle, no fault, no exhaustion flag, and the host
    build's spill peaks and inbound spill bytes."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    monkeypatch.delenv("RBE_INGEST_EXACT", raising=False)
    _parity(name, host_figures)


@pytest.mark.parametrize("name", ["iso70_w2_wire", "maxm1_w2_wire"])
def test_gpu_ingest_spill_exact_path(gpu_available, monkeypatch, host_figures, name):
    """The exact path (read-backs between the stages) gives what the
    no-read-back path gives: the oracle's views and the host build's figures,
    which test_gpu_ingest_spill_parity holds the other path to."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    monkeypatch.setenv("RBE_INGEST_EXACT", "1")
    _parity(name, host_figures)


@pytest.mark.parametrize("name,rounds", [("iso70_w2_wire", 130), ("maxm1_w2_push", 100)])
def test_gpu_ingest_spill_push_equals_wire(gpu_available, monkeypatch, name, rounds):
    monkeypatch.delenv("RBE_MODE", raising=False)
    made = _Made()
    I.push_equals_wire(made, name, rounds)
    world = I.SHAPES[name][1]
    fa, fb = made.figures(2 * world)[:world], made.figures(2 * world)[world:]
    assert fa == fb and any(inb for _, inb in fa), (fa, fb)


@pytest.mark.parametrize("wire", [False, True], ids=["push", "wire"])
def test_gpu_ingest_spill_refused_when_the_share_is_short(gpu_available, monkeypatch, wire):
    """The hop is refused whole, oom and the peak untouched, the engine equals
    its twin that got an empty batch; then a 31-entry catch-up leaves a peak
    of exactly 31 x 32 bytes.  The refusal and the spill are counted."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    made = _Made()
    I.refusal(made, wire)
    e, twin = made.engs
    assert e.final == (31 * 32, 31 * 32), e.final
    assert twin.final == (0, 0), twin.final


def test_gpu_inbound_spill_stats(gpu_available, monkeypatch):
    """rbe_inbound_spill_stats: bytes taken, batches that spilled, batches
    refused.  spill_bytes = 2048 over two ranks leaves each 64 granules; with
    ecap = 4 a Replicate of n > 4 entries needs 2 n."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    kw = dict(n_groups=4, n_replicas=3, wl_enabled=False)
    e = _make(trace=True, rep_world=2, rep_rank=0, spill_bytes=2048, ecap=4, **kw)
    e.step()
    assert e.inbound_spill_stats() == dict(bytes=0, batches=0, refused=0)
    for n, wire in ((33, True), (40, False), (80, True)):
        with pytest.raises(InputError) as ei:
            if wire:
                e.wire_ingest(I.catch_up(n, True))
            else:
                e.push_messages(*I.catch_up(n, False))
        assert ei.value.rc == RBE_E_NOMEM
    assert e.inbound_spill_stats() == dict(bytes=0, batches=0, refused=3)
    e.wire_ingest(I.catch_up(4, True))  # fits the arena: nothing spills
    assert e.inbound_spill_stats() == dict(bytes=0, batches=0, refused=3)
    e.wire_ingest(I.catch_up(10, True))  # 20 granules
    e.push_messages(*I.catch_up(22, False))  # 44 more: exactly the share
    assert e.inbound_spill_stats() == dict(bytes=64 * 16, batches=2, refused=3)
    assert e.inbound_spill_bytes == 64 * 16
    st = e.spill_stats()
    assert st["spill_peak_bytes"] == 64 * 16 and st["oom"] == 0, st
    with pytest.raises(InputError):  # the share is used up
        e.wire_ingest(I.catch_up(5, True))
    assert e.inbound_spill_stats()["refused"] == 4
    e.step()  # the round reads the last batch and gives the granules back
    assert e.fault_summary()[0] == 0
    e.step()
    e.wire_ingest(I.catch_up(32, True))  # the whole share again
    assert e.inbound_spill_stats() == dict(bytes=2 * 64 * 16, batches=3, refused=4)
    e.close()


@pytest.mark.parametrize("wire", [False, True], ids=["push", "wire"])
def test_gpu_ingest_spill_session_entries(gpu_available, monkeypatch, wire):
    """Heap Cmds and session fields with an arena of one entry: the entries
    spill, their records go to the payload heap, every Cmd reads back."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    made = _Made()

    def make(**kw):
        return made(ecap=1, **kw)

    S.session_over_transport(make, 2, wire=wire)
    got = [e.inbound_spill_bytes for e in made.engs]
    assert all(b > 0 for b in got), got
    for e in made.engs:
        st = e.spill_stats()
        assert st["oom"] == 0, st
        e.close()


@pytest.mark.parametrize("wire", [True, False], ids=["wire", "push"])
def test_gpu_batch_that_fits_spills_nothing(gpu_available, monkeypatch, wire):
    """test_transport.CASES' first case: nothing is past maxm / ecap, so the
    inbound statistics stay zero (and the run equals the oracle as before)."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    kw, world, rounds, extra = CASES[next(iter(CASES))]
    engs = [_make(trace=True, rep_world=world, rep_rank=r, **kw, **extra) for r in range(world)]
    d, moved = run_transport(engs, O.Harness(**kw), kw["n_replicas"], rounds, wire=wire)
    assert d is None, f"first divergence {d}"
    assert moved > rounds
    for e in engs:
        assert e.fault_summary()[0] == 0
        assert e.inbound_spill_stats() == dict(bytes=0, batches=0, refused=0)
        assert e.inbound_spill_bytes == 0
        e.close()
