"""Self-contained checkpoints on the HIP engine (rbe_export_groups_ex, the
heap section of rbe_import_groups; dragonboat_amd/csrc/rbe_checkpoint_kernels.h):
the scenarios of tests/checkpoint_scenarios.py, and the host build's bytes
against the device's for the same run.  The CPU-tier twin is
tests/test_checkpoint.py."""
import pytest

import checkpoint_scenarios as S
from parity_util import C3

pytestmark = pytest.mark.gpu


def mk(**kw):
    from dragonboat_amd.engine import Engine
    return Engine(device=0, trace=True, **kw)


def mk_cpu(**kw):
    from checkpoint_cpu.checkpoint import CheckpointCpu
    return CheckpointCpu(trace=True, **kw)


def test_gpu_plain_ex_export_is_export_groups(gpu_available):
    dev = S.identity(mk, C3, 141)
    # the host build of the same run: the same bytes
    cpu = mk_cpu(**C3)
    cpu.run(141)
    assert cpu.export_groups(device=True) == dev


def test_gpu_plain_ex_export_with_a_host_tier(gpu_available):
    S.identity(mk, S.TIER_KW, S.TIER_ROUNDS, tier_stats=True)


def test_gpu_resume_in_a_fresh_engine(gpu_available):
    S.resume_fresh(mk, "gpu")


def test_gpu_section_is_the_host_builds(gpu_available):
    """The heap section the device gathers equals the host build's, byte for
    byte, for the same driven run."""
    a, b = S.heap_source(mk, "gpu"), S.heap_source(mk_cpu, "gpu-cpu")
    assert a["snap"] == b["snap"]


def test_gpu_section_shape(gpu_available):
    S.section_shape(mk, "gpu")


def test_gpu_wrap_and_laps(gpu_available):
    S.wrap_and_laps(mk)


def test_gpu_inflight_forward(gpu_available):
    S.inflight_forward(mk)


def test_gpu_handoff(gpu_available):
    S.handoff(mk)


def test_gpu_refusals(gpu_available):
    S.refusals(mk, "gpu")
