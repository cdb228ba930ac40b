"""The fast steps' summary-word form (k_fast_both at N = 3: the inbound count
words rebuilt from the 7-bit fields of the work-list entry, rbe_step.h
inbound_aux) at plane capacities below the fast steps' own limits.

In that form the inbound message loads issue before the step checks that it
takes the round, from clamped counts: a list in the round spill heap gives
A = B = 7 whatever maxm is.  rbe_fast.h lead_gather_slot / foll_gather_slot
keep every such load inside the sender's list.  Here, on the host build of the
step (tests/soa_cpu):

  * tests/fast_aux_cpu/fast_aux_cpu.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers: every summary field, maxm and
    gather slot through those two functions, then short tiny-capacity runs;
  * the MIXED-shaped workload of test_spill.py at N = 3, 4, 5 with maxm = 1..4,
    summary-word form and plain form, each against the oracle round by round;
  * C4_DENSE (N = 3, Quiesce, group sleep) with small capacities;
  * an N = 3 replica-per-rank case with every capacity at 1 (replica_aux.py
    adds it to test_replica_gloo.CASES).

The GPU twins are in test_gpu_fast_aux.py."""
import os
import subprocess

import pytest

import oracle as O
from parity_util import C4_DENSE, counters_match, run_lockstep
from replica_aux import run_aux_case
from soa_cpu.soa import SoaCpu
from test_spill import TINY

HERE = os.path.dirname(os.path.abspath(__file__))

# maxm below / at the leader's MAXM (4 at N = 3), all below the follower's FMAXM (6)
CAPS = {"tiny": TINY["tiny"], "fast": TINY["fast"], "maxm3": dict(maxm=3, ring=8),
        "maxm4": dict(maxm=4, ring=8)}


def mixed(n):
    """The workload of test_spill.test_lists_and_queues_past_capacity, n replicas."""
    return dict(n_groups=12, n_replicas=n, check_quorum=True, quiesce=True, wl_enabled=True,
                wl_start_round=25, wl_active_mod=2, wl_read_permille=500, iso_period=37,
                iso_len=20, iso_mod=2, seed=12345)


def test_fast_aux_cpu(tmp_path):
    """The alignment check is off: the host engine's planes are byte vectors
    and calloc'd blocks, not the 256-byte aligned device allocations."""
    exe = tmp_path / "fast_aux_cpu"
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize=alignment", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(HERE, "fast_aux_cpu", "fast_aux_cpu.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("fast_aux_cpu ok"), out.stdout + out.stderr
    assert not out.stderr, out.stderr  # (a recovered sanitizer report)


def _lockstep(kw, caps, staged, trace, rounds):
    eng = SoaCpu(staged=staged, trace=trace, **caps, **kw)
    ref = O.Harness(trace=trace, **kw)
    d = run_lockstep(eng, ref, rounds, every=1, skip=() if trace else ("digest",))
    assert d is None, f"staged={staged}: first divergence {d}"
    n, bits = eng.faults()
    assert n == 0, f"staged={staged}: faults {bits:#x}"
    bad = counters_match(eng.counters(), ref.counters())
    assert not bad, f"staged={staged}: counters differ {bad}"
    return eng


@pytest.mark.parametrize("trace", [True, False], ids=["traced", "untraced"])
@pytest.mark.parametrize("caps", list(CAPS))
@pytest.mark.parametrize("n", [3, 4, 5])
def test_summary_form_small_capacities(n, caps, trace):
    """Both forms equal the oracle, spill, and decline the same rounds."""
    slow = {}
    for staged in (4, 0):
        eng = _lockstep(mixed(n), CAPS[caps], staged, trace, 300)
        st = eng.spill_stats()
        assert st["spill_peak_bytes"] > 0 and st["oom"] == 0, st
        slow[staged] = eng.slow_total()
        assert slow[staged] < eng.counters()["steps"], "no fast step took a round"
    assert slow[4] == slow[0], slow


@pytest.mark.parametrize("caps", ["fast", "maxm3"])
def test_c4_dense_small_capacities(caps):
    """C4_DENSE untraced (group sleep on) in the summary-word form.  The
    workload does spill at both capacities (98048 and 57856 bytes of the round
    spill heap at the peak on the host build), so that is asserted too."""
    slow = {}
    for staged in (4, 0):
        eng = _lockstep(C4_DENSE, CAPS[caps], staged, False, 400)
        st = eng.spill_stats()
        assert st["spill_peak_bytes"] > 0 and st["oom"] == 0, st
        slow[staged] = eng.slow_total()
        assert slow[staged] < eng.counters()["steps"], "no fast step took a round"
    assert slow[4] == slow[0], slow


def test_replica_per_rank_tiny_n3(monkeypatch):
    """C4-shaped, three ranks, every capacity 1, the summary-word form: every
    owned replica equals the oracle (test_replica_gloo.run_case)."""
    run_aux_case(monkeypatch)
