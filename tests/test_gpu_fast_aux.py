"""The fast steps at N = 3 with plane capacities below their own limits, on
the HIP engine (tests/test_fast_aux.py is the CPU twin): the default pipeline
steps N = 3 in the summary-word form (k_fast_both, rbe_kernels.h kListAux),
whose speculative message loads must stay inside the lists whatever the
clamped counts say (rbe_fast.h lead_gather_slot / foll_gather_slot); the
other pipelines step the plain form, and all of them equal the oracle round
by round.  12 groups x 3 replicas x 300 rounds each."""
import pytest

import oracle as O
from parity_util import counters_match, run_lockstep
from replica_aux import run_aux_case
from test_fast_aux import CAPS, mixed

pytestmark = pytest.mark.gpu


def _run(caps, trace, fast_both):
    from dragonboat_amd.engine import Engine
    kw = mixed(3)
    eng = Engine(device=0, trace=trace, **CAPS[caps], **kw)
    ref = O.Harness(trace=trace, **kw)
    d = run_lockstep(eng, ref, 300, every=1, skip=() if trace else ("digest",))
    assert d is None, f"first divergence {d}"
    n, bits = eng.fault_summary()
    assert n == 0, f"faults {bits:#x}"
    bad = counters_match(eng.counters(), ref.counters())
    assert not bad, f"counters differ {bad}"
    st = eng.spill_stats()
    assert st["spill_peak_bytes"] > 0 and st["pool_pages_used"] > 0 and st["oom"] == 0, st
    names = eng.kernel_names()
    assert ("k_fast_both" in names) == fast_both, names
    # the boundary reads the spilled lists and ReadyToReads: the collected
    # outputs of the last round equal the per-replica getters
    moff, msgs, roff, rtrs = eng.collect_outputs(0, eng.n_rep)
    for r in range(eng.n_rep):
        assert moff[r + 1] - moff[r] == len(eng.messages(r))
        assert roff[r + 1] - roff[r] == len(eng.ready_to_reads(r))
    fast_steps = eng.kernel_counters(names.index("k_fast_both"))["steps"] if fast_both else None
    print(f"caps={caps} trace={trace} steps={eng.counters()['steps']} k_fast_both steps={fast_steps} "
          f"spill={st}")
    eng.close()
    if fast_both:  # replica-rounds the kernel's fast steps took (a declined one counts nothing)
        assert fast_steps > 0


@pytest.mark.parametrize("trace", [True, False], ids=["traced", "untraced"])
@pytest.mark.parametrize("caps", list(CAPS))
def test_gpu_summary_form_small_capacities(gpu_available, monkeypatch, caps, trace):
    """Measured on an MI355X, 10800 replica-rounds each, traced = untraced:
    k_fast_both's steps counter 3504 (tiny), 6511 (fast), 7163 (maxm3), 8345
    (maxm4), spill peaks 49952 / 28544 / 26112 / 2368 bytes as on the host
    build.  With `tiny` the leader step declines every round (rtr_cap < RQ,
    ecap < 2: its outputs would not fit) and the follower step takes the
    rounds with at most rtr_cap = 1 inbound message."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    _run(caps, trace, True)


@pytest.mark.parametrize("mode,caps", [("split", "tiny"), ("split", "maxm3"), ("fused", "tiny"),
                                       ("fused", "maxm3"), ("full", "tiny")])
def test_gpu_other_pipelines_small_capacities(gpu_available, monkeypatch, mode, caps):
    monkeypatch.setenv("RBE_MODE", mode)
    _run(caps, True, False)


def test_gpu_replica_per_rank_tiny_n3(gpu_available, monkeypatch):
    """Replica mode at N = 3 with every capacity 1 (replica_aux.py)."""
    monkeypatch.delenv("RBE_MODE", raising=False)
    run_aux_case(monkeypatch, gpu=True)


def test_gpu_replica_per_rank_tiny_n5(gpu_available, monkeypatch):
    """test_replica_gloo's MIXED_tiny_w2 on the device, which test_gpu_replica.py
    does not run: lists and entries past the capacities cross ranks."""
    from test_replica_gloo import run_case
    monkeypatch.delenv("RBE_MODE", raising=False)
    run_case("MIXED_tiny_w2", gpu=True)
