"""rbe_collect_dropped / rbe_get_dropped on the HIP engine: the general step's
recording (cfg.drop_lists) and the batched read, gathered on the device in a
fixed number of launches, copies and waits.  Every case runs its scenario of
dropped_scenarios.py on the device, with the constructed expectations the
scenario asserts, and compares what it observed with the host build
(tests/dropped_cpu) on the same inputs, list for list."""
import ctypes as C
import functools

import pytest

import dropped_scenarios as S
from dragonboat_amd.engine import RbeDroppedList

pytestmark = pytest.mark.gpu


def make(**kw):
    from dragonboat_amd.engine import Engine
    return Engine(device=0, **kw)


def raw(eng, first, count, flags, handle=True, out=True):
    o = RbeDroppedList()
    rc = eng.lib.rbe_collect_dropped(eng.h if handle else None, first, count, flags,
                                     C.byref(o) if out else None)
    return rc, o


@functools.lru_cache(maxsize=None)
def host(name, *args):
    """The host build's observations of a scenario (computed once)."""
    import test_dropped_collect as T
    fn = getattr(S, name)
    if name in ("lapped_record", "off_and_arguments"):
        return fn(T.make, T.raw)
    return fn(T.make, *args)


def test_gpu_exact_by_construction(gpu_available):
    assert S.exact(make) == host("exact")


@pytest.mark.parametrize("session", [False, True])
def test_gpu_driven_lockstep_with_the_harness(gpu_available, session):
    assert S.driven(make, session)[0] == host("driven", session)[0]


@pytest.mark.parametrize("tiny", [False, True])
def test_gpu_transferring_leader(gpu_available, tiny):
    assert S.transferring_leader(make, tiny) == host("transferring_leader", tiny)


def test_gpu_pending_config_change(gpu_available):
    assert S.pending_config_change(make) == host("pending_config_change")


def test_gpu_list_growth_and_block_edges(gpu_available):
    assert S.growth_and_block_edges(make) == host("growth_and_block_edges")


def test_gpu_read_indexes_past_dri_cap(gpu_available):
    assert S.read_indexes_past_dri_cap(make) == host("read_indexes_past_dri_cap")


def test_gpu_lapped_record_is_refused(gpu_available):
    assert S.lapped_record(make, raw) == host("lapped_record")


def test_gpu_spill_heap_too_small(gpu_available):
    assert S.spill_heap_too_small(make) == host("spill_heap_too_small")


def test_gpu_replica_mode(gpu_available):
    assert S.replica_mode(make) == host("replica_mode")


def test_gpu_off_and_arguments(gpu_available):
    assert S.off_and_arguments(make, raw) == host("off_and_arguments")


def test_gpu_nothing_else_moved(gpu_available):
    """drop_lists = 0 against 1 on the device, round for round (the spill
    constants are the host build's: the device's heap use is its own)."""
    off, e0 = S.driven(make, drop_lists=False)
    on, e1 = S.driven(make, drop_lists=False, extra=dict(drop_lists=True))
    assert off == on
    assert e0.counters() == e1.counters()
