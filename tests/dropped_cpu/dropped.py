"""TEST-ONLY wrapper of libdropped_cpu.so: the host build of the step
(tests/soa_cpu) with the spilling inbound transport (tests/ingest_cpu), the
batched outbox (tests/outbox_cpu) and the dropped lists on top
(dropped_cpu.cpp).

A variant build of the host library, loaded through a second copy of
tests/soa_cpu/soa.py as tests/outbox_cpu/outbox.py does, so the soa module the
other tests use is not touched.
"""
import ctypes as C
import importlib.util
import os

import soa_cpu.soa as _plain
from dragonboat_amd.engine import (RbeDroppedList, RbeEntry, RbeMessage, RbeOutboxList,
                                   RbeSystemCtx, RbeUpdate, dropped_call, dropped_list_call,
                                   outbox_list_call, push_messages_call)

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("dropped_cpu._soa_variant", _plain.__file__)
soa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(soa)
_typed = False


def lib():
    """libdropped_cpu.so with soa.lib()'s signatures and the new ones."""
    global _typed
    if not _typed:
        p = os.path.join(_HERE, "libdropped_cpu.so")
        if not os.path.exists(p):
            raise RuntimeError(f"{p} missing: run __graft_entry__.build()")
        env = os.environ.get("SOA_LIB")
        os.environ["SOA_LIB"] = p  # (read once, by the copy's first lib())
        try:
            L = soa.lib()
        finally:
            if env is None:
                del os.environ["SOA_LIB"]
            else:
                os.environ["SOA_LIB"] = env
        P = C.POINTER
        L.soa_set_drop_lists.restype = C.c_int
        L.soa_set_drop_lists.argtypes = [C.c_void_p]
        L.soa_collect_dropped.restype = C.c_int
        L.soa_collect_dropped.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                          P(RbeDroppedList)]
        L.soa_get_dropped.restype = C.c_int
        L.soa_get_dropped.argtypes = [C.c_void_p, C.c_uint64, P(RbeEntry), C.c_uint32,
                                      P(C.c_uint32), C.c_void_p, C.c_uint64, P(C.c_uint64),
                                      P(RbeSystemCtx), C.c_uint32, P(C.c_uint32)]
        L.soa_get_updates.restype = C.c_int
        L.soa_get_updates.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, P(RbeUpdate)]
        L.soa_dropped_extra_blocks.argtypes = [C.c_uint64]
        L.soa_dropped_passes.restype = C.c_uint32
        L.soa_import_groups_dropped.restype = C.c_int
        L.soa_import_groups_dropped.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        L.soa_collect_outbox.restype = C.c_int
        L.soa_collect_outbox.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.c_int32, P(RbeOutboxList)]
        L.soa_push_messages_spill.restype = C.c_int
        L.soa_push_messages_spill.argtypes = [C.c_void_p, C.c_uint64, P(C.c_uint64),
                                              P(RbeMessage), P(RbeEntry), C.c_void_p]
        _typed = True
    return soa.lib()


class DroppedCpu(soa.SoaCpu):
    """SoaCpu on the variant library with Engine.collect_dropped / get_dropped
    (drop_lists=True switches the recording on, as cfg.drop_lists does)."""

    def __init__(self, drop_lists=False, **kw):
        lib()
        super().__init__(**kw)
        if drop_lists and lib().soa_set_drop_lists(self.h):
            raise RuntimeError("soa_set_drop_lists failed")

    def collect_dropped(self, first=0, count=None, cmds=True, raw=False):
        count = self.n_rep - first if count is None else count
        return dropped_list_call(lib().soa_collect_dropped, "soa_collect_dropped", self.h, first,
                                 count, cmds, raw)

    def get_dropped(self, replica):
        return dropped_call(lib().soa_get_dropped, self.h, replica)

    def updates(self, first=0, count=None):
        count = self.n_rep - first if count is None else count
        arr = (RbeUpdate * max(1, count))()
        rc = lib().soa_get_updates(self.h, first, count, arr)
        if rc:
            raise RuntimeError(f"soa_get_updates rc={rc}")
        return arr

    def collect_outbox(self, first=0, count=None, remote_only=False, dst_rank=-1, cmds=True,
                       raw=False):
        count = self.n_rep - first if count is None else count
        return outbox_list_call(lib().soa_collect_outbox, "soa_collect_outbox", self.h, first,
                                count, remote_only, dst_rank, cmds, raw)

    def push_messages(self, groups, msgs, ents, cmds=None):
        push_messages_call(lib().soa_push_messages_spill, self.h, groups, msgs, ents, cmds)

    def import_groups(self, snap, resume=False):
        rc = lib().soa_import_groups_dropped(self.h, snap, len(snap), 1 if resume else 0)
        if rc != 0:
            raise soa.SnapshotError(rc)
