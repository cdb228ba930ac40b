"""rbe_collect_entries / rbe_collect_entry_ranges on the CPU tier: the
per-range and per-entry logic of the HIP kernels (dragonboat_amd/csrc/
rbe_collect.h) driven as plain loops over the planes of the host build
(tests/collect_cpu), against the oracle's LogDB and the per-replica getters.
The scenarios are in collect_scenarios.py; test_gpu_collect_entries.py runs
them on the HIP engine."""
import ctypes as C

import pytest

import collect_scenarios as S
from collect_cpu.collect import CollectCpu, lib
from dragonboat_amd.engine import RBE_ENTRIES_TO_SAVE, RbeEntry, RbeEntryList


def _make(**kw):
    return CollectCpu(**kw)


def _raw(eng, name, handle, out):
    o = RbeEntryList()
    h, op = (eng.h if handle else None), (C.byref(o) if out else None)
    one = (C.c_uint64 * 1)(1)
    if name == "collect_entries":
        return lib().soa_collect_entries(h, 0, 1, RBE_ENTRIES_TO_SAVE, op)
    return lib().soa_collect_entry_ranges(h, 1, one, one, one, 0, op)


def _get_entries_rc(eng, replica, lo, hi):
    arr = (RbeEntry * (hi - lo + 1))()
    return lib().soa_get_entries(eng.h, replica, lo, hi, arr)


@pytest.mark.parametrize("mes", [0, 9000])
def test_lists_replay_to_the_oracle_logdb(mes):
    S.oracle_logdb(_make, mes)


def test_ranges_across_the_cold_log_and_the_ring():
    S.cold_and_ring(_make)


def test_relaunched_replica_replays_its_log():
    S.relaunch_replay(_make)


def test_launched_entries_read_back_before_the_step():
    S.launch_then_collect(_make)


def test_bad_arguments_are_refused():
    S.bad_arguments(_make, _raw)


def test_lapped_heap_records_are_refused():
    S.lapped_heap(_make, _get_entries_rc)


def test_compacted_entries_are_refused():
    S.compacted_range(_make)


def test_replica_mode_lists_owned_replicas():
    S.replica_mode(_make)
