"""rbe_collect_outbox on the CPU tier: the per-replica, per-message and
per-entry logic of the HIP kernels (dragonboat_amd/csrc/rbe_outbox.h) driven as
loops over whole 256-lane blocks on the planes of the host build
(tests/outbox_cpu), against rbe_get_outbox and the oracle.  The scenarios are
in outbox_scenarios.py; test_gpu_outbox_collect.py runs them on the HIP engine.
tests/outbox_cpu/outbox_main.cpp is built with -fsanitize=address,undefined and
run as a program of its own."""
import ctypes as C
import os
import subprocess

import pytest

import outbox_scenarios as S
from dragonboat_amd.engine import RbeOutboxList
from ingest_spill_scenarios import SHAPES
from outbox_cpu.outbox import OutboxCpu, lib
from test_transport import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(**kw):
    return OutboxCpu(**kw)


def _raw(eng, first, count, flags, dst_rank, handle=True, out=True):
    o = RbeOutboxList()
    rc = lib().soa_collect_outbox(eng.h if handle else None, first, count, flags, dst_rank,
                                  C.byref(o) if out else None)
    return rc, o


@pytest.mark.parametrize("name", list(S.EQUAL))
def test_equal_to_the_per_replica_call(name):
    S.equal_to_per_replica(_make, name)


def test_node_ids_in_any_order():
    S.node_ids_any_order(_make)


@pytest.mark.parametrize("name,full_only", [("iso_40_20", False), ("mixed_tiny", False),
                                            ("mixed_tiny", True)])
def test_spilled_lists_and_entries(name, full_only):
    S.spilled(_make, name, full_only)


def test_cmds_and_heap_records():
    S.cmds_and_heap_records(_make)


def test_staged_records_are_uploaded_first():
    S.staged_records(_make)


def test_lapped_record_is_refused():
    S.lapped_record(_make, _raw)


@pytest.mark.parametrize("name", ["C2_w2", "C3_iso_w3", "maxm1_w2_push"])
def test_replica_mode_transport_loop(name):
    if name in CASES:
        kw, world, rounds, extra = CASES[name]
    else:
        kw, world, rounds, extra, _ = SHAPES[name]
    engs = S.replica_mode(_make, kw, world, rounds, extra)
    if name == "maxm1_w2_push":  # inbound-spilled lists of remote senders were delivered
        assert any(e.inbound_spill_bytes for e in engs)


def test_arguments_and_lifetime():
    S.arguments_and_lifetime(_make, _raw)


def test_sanitized_passes_over_whole_blocks(tmp_path):
    """outbox_main.cpp under AddressSanitizer and UBSan: the passes over whole
    256-lane blocks (lanes past the range, a grid larger than the totals) on
    the tiny-capacity shape, every round against outbox_messages.  The
    alignment check is off, as in test_ingest_dev.py: the host engine's planes
    are byte vectors and calloc'd blocks, not 256-byte aligned allocations."""
    exe = str(tmp_path / "outbox_main")
    src = os.path.join(ROOT, "tests", "outbox_cpu", "outbox_main.cpp")
    subprocess.run(["g++", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize=alignment", "-fno-sanitize-recover=undefined", "-o", exe,
                    src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("outbox_main ok"), out.stdout + out.stderr
    assert not out.stderr, out.stderr  # (a recovered sanitizer report)
