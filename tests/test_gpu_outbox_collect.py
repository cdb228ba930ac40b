"""rbe_collect_outbox on the HIP engine: the last round's messages of many
senders with their entries and Cmds, gathered on the device in a fixed number
of launches, copies and waits, against rbe_get_outbox and the oracle.  The
scenarios are in outbox_scenarios.py; test_outbox_collect.py runs them on the
host build."""
import ctypes as C
import os

import pytest

import outbox_scenarios as S
from dragonboat_amd.engine import RbeOutboxList
from ingest_spill_scenarios import SHAPES
from test_transport import CASES

pytestmark = pytest.mark.gpu


def _make(full_only=False, **kw):
    from dragonboat_amd.engine import Engine
    if not full_only:
        return Engine(device=0, **kw)
    old = os.environ.get("RBE_MODE")
    os.environ["RBE_MODE"] = "full"  # (read by rbe_create)
    try:
        return Engine(device=0, **kw)
    finally:
        if old is None:
            del os.environ["RBE_MODE"]
        else:
            os.environ["RBE_MODE"] = old


def _raw(eng, first, count, flags, dst_rank, handle=True, out=True):
    o = RbeOutboxList()
    rc = eng.lib.rbe_collect_outbox(eng.h if handle else None, first, count, flags, dst_rank,
                                    C.byref(o) if out else None)
    return rc, o


@pytest.mark.parametrize("name", list(S.EQUAL))
def test_gpu_equal_to_the_per_replica_call(gpu_available, name):
    S.equal_to_per_replica(_make, name)


def test_gpu_node_ids_in_any_order(gpu_available):
    S.node_ids_any_order(_make)


@pytest.mark.parametrize("name,full_only", [("iso_40_20", False), ("mixed_tiny", False),
                                            ("mixed_tiny", True)])
def test_gpu_spilled_lists_and_entries(gpu_available, name, full_only):
    S.spilled(_make, name, full_only)


def test_gpu_cmds_and_heap_records(gpu_available):
    S.cmds_and_heap_records(_make)


def test_gpu_staged_records_are_uploaded_first(gpu_available):
    S.staged_records(_make)


def test_gpu_lapped_record_is_refused(gpu_available):
    S.lapped_record(_make, _raw)


@pytest.mark.parametrize("name", ["C2_w2", "maxm1_w2_push"])
def test_gpu_replica_mode_transport_loop(gpu_available, name):
    if name in CASES:
        kw, world, rounds, extra = CASES[name]
    else:
        kw, world, rounds, extra, _ = SHAPES[name]
    S.replica_mode(_make, kw, world, rounds, extra)


def test_gpu_arguments_and_lifetime(gpu_available):
    S.arguments_and_lifetime(_make, _raw)
