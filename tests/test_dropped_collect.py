"""rbe_collect_dropped / rbe_get_dropped on the CPU tier: the recording of the
general step (cfg.drop_lists) and the per-replica, per-entry and per-context
logic of the HIP kernels (dragonboat_amd/csrc/rbe_dropped.h) driven as loops
over whole 256-lane blocks on the planes of the host build (tests/dropped_cpu).
The scenarios are in dropped_scenarios.py; test_gpu_dropped_collect.py runs
them on the HIP engine and compares the device with this tier.
tests/dropped_cpu/dropped_main.cpp is built with -fsanitize=address,undefined
and run as a program of its own."""
import ctypes as C
import os
import subprocess

import pytest

import dropped_scenarios as S
from dragonboat_amd.engine import RbeDroppedList
from dropped_cpu.dropped import DroppedCpu, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(**kw):
    return DroppedCpu(**kw)


def raw(eng, first, count, flags, handle=True, out=True):
    o = RbeDroppedList()
    rc = lib().soa_collect_dropped(eng.h if handle else None, first, count, flags,
                                   C.byref(o) if out else None)
    return rc, o


def test_exact_by_construction():
    S.exact(make)


@pytest.mark.parametrize("session", [False, True])
def test_driven_lockstep_with_the_harness(session):
    S.driven(make, session)


@pytest.mark.parametrize("tiny", [False, True])
def test_transferring_leader(tiny):
    S.transferring_leader(make, tiny)


def test_pending_config_change():
    S.pending_config_change(make)


def test_list_growth_and_block_edges():
    S.growth_and_block_edges(make)


def test_read_indexes_past_dri_cap():
    S.read_indexes_past_dri_cap(make)


def test_lapped_record_is_refused():
    S.lapped_record(make, raw)


def test_spill_heap_too_small():
    S.spill_heap_too_small(make)


def test_replica_mode():
    S.replica_mode(make)


def test_off_and_arguments():
    S.off_and_arguments(make, raw)


@pytest.mark.parametrize("session", [False, True])
def test_nothing_else_moved(session):
    S.nothing_else_moved(make, session)


def test_sanitized_passes_over_whole_blocks(tmp_path):
    """dropped_main.cpp under AddressSanitizer and UBSan (built by
    __graft_entry__.build(); here when it is missing): the recording and the
    passes over whole 256-lane blocks with grids larger than the totals, every
    round against soa_get_dropped, and the fixed number of passes a call makes.
    The alignment check is off, as in test_outbox_collect.py: the host engine's
    planes are byte vectors and calloc'd blocks."""
    exe = os.path.join(ROOT, "tests", "dropped_cpu", "dropped_main")
    if not os.path.exists(exe):
        exe = str(tmp_path / "dropped_main")
        src = os.path.join(ROOT, "tests", "dropped_cpu", "dropped_main.cpp")
        subprocess.run(["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize=alignment", "-fno-sanitize-recover=undefined", "-o", exe,
                        src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("dropped_main ok"), out.stdout + out.stderr
    assert not out.stderr, out.stderr  # (a recovered sanitizer report)
