"""Self-contained checkpoints on the host build (tests/checkpoint_cpu: the
RBE_HD functions of dragonboat_amd/csrc/rbe_checkpoint.h as plain loops on the
host build of the step): the scenarios of tests/checkpoint_scenarios.py.  The
GPU tier runs the same through the HIP engine (tests/test_gpu_checkpoint.py)."""
import checkpoint_scenarios as S
from checkpoint_cpu.checkpoint import CheckpointCpu
from parity_util import C3


def mk(**kw):
    return CheckpointCpu(trace=True, **kw)


def test_plain_ex_export_is_export_groups():
    S.identity(mk, C3, 141)


def test_plain_ex_export_with_a_host_tier():
    S.identity(mk, S.TIER_KW, S.TIER_ROUNDS)


def test_resume_in_a_fresh_engine():
    S.resume_fresh(mk, "cpu")


def test_section_shape():
    S.section_shape(mk, "cpu")


def test_wrap_and_laps():
    S.wrap_and_laps(mk)


def test_inflight_forward():
    S.inflight_forward(mk)


def test_handoff():
    S.handoff(mk)


def test_refusals():
    S.refusals(mk, "cpu")
