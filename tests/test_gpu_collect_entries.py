"""rbe_collect_entries / rbe_collect_entry_ranges on the HIP engine: the
entries of the Updates of many replicas gathered on the device (the ring, the
cold log in HBM and in its host tier, the payload heap) in a fixed number of
launches, copies and waits, against the oracle's LogDB and the per-replica
getters.  The scenarios are in collect_scenarios.py; test_collect_entries.py
runs them on the host build."""
import ctypes as C

import pytest

import collect_scenarios as S
from dragonboat_amd.engine import RBE_ENTRIES_TO_SAVE, RbeEntry, RbeEntryList

pytestmark = pytest.mark.gpu


def _make(**kw):
    from dragonboat_amd.engine import Engine
    return Engine(device=0, **kw)


def _raw(eng, name, handle, out):
    o = RbeEntryList()
    h, op = (eng.h if handle else None), (C.byref(o) if out else None)
    one = (C.c_uint64 * 1)(1)
    if name == "collect_entries":
        return eng.lib.rbe_collect_entries(h, 0, 1, RBE_ENTRIES_TO_SAVE, op)
    return eng.lib.rbe_collect_entry_ranges(h, 1, one, one, one, 0, op)


def _get_entries_rc(eng, replica, lo, hi):
    arr = (RbeEntry * (hi - lo + 1))()
    return eng.lib.rbe_get_entries(eng.h, replica, lo, hi, arr)


@pytest.mark.parametrize("mes", [0, 9000])
def test_gpu_lists_replay_to_the_oracle_logdb(gpu_available, mes):
    S.oracle_logdb(_make, mes)


def test_gpu_ranges_across_the_cold_log_and_the_ring(gpu_available):
    S.cold_and_ring(_make)


def test_gpu_relaunched_replica_replays_its_log(gpu_available):
    S.relaunch_replay(_make)


def test_gpu_host_tier_pages(gpu_available):
    S.host_tier_ranges(_make)


def test_gpu_launched_entries_read_back_before_the_step(gpu_available):
    S.launch_then_collect(_make)


def test_gpu_bad_arguments_are_refused(gpu_available):
    S.bad_arguments(_make, _raw)


def test_gpu_lapped_heap_records_are_refused(gpu_available):
    S.lapped_heap(_make, _get_entries_rc)


def test_gpu_compacted_entries_are_refused(gpu_available):
    S.compacted_range(_make)


def test_gpu_replica_mode_lists_owned_replicas(gpu_available):
    S.replica_mode(_make)
