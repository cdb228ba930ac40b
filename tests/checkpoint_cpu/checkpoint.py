"""TEST-ONLY wrapper of libcheckpoint_cpu.so: the host build of the step
(tests/soa_cpu) with the batched entry collection (tests/collect_cpu) and the
self-contained checkpoints (checkpoint_cpu.cpp) on top.

As tests/collect_cpu/collect.py does, the variant library gets a copy of
tests/soa_cpu/soa.py of its own, loaded under another name and pointed at the
variant through SOA_LIB, so the soa module the other tests use is not touched.
"""
import ctypes as C
import importlib.util
import os

import soa_cpu.soa as _plain
from dragonboat_amd.engine import (RBE_ENTRIES_NO_CMDS, RBE_EXPORT_HEAP, RbeEntryList,
                                   entry_list_call, entry_ranges_args, export_ex_call)

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("checkpoint_cpu._soa_variant", _plain.__file__)
soa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(soa)
_typed = False


def lib():
    """libcheckpoint_cpu.so with soa.lib()'s signatures and the new ones."""
    global _typed
    if not _typed:
        p = os.path.join(_HERE, "libcheckpoint_cpu.so")
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
        u64p = C.POINTER(C.c_uint64)
        L.soa_collect_entry_ranges.restype = C.c_int
        L.soa_collect_entry_ranges.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, u64p,
                                               C.c_uint32, C.POINTER(RbeEntryList)]
        L.soa_export_groups_ex.restype = C.c_int
        L.soa_export_groups_ex.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                           C.c_void_p, C.c_uint64, u64p]
        L.soa_import_groups_ck.restype = C.c_int
        L.soa_import_groups_ck.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        _typed = True
    return soa.lib()


class SnapshotError(RuntimeError):
    def __init__(self, rc):
        super().__init__(f"snapshot call failed with rc={rc}")
        self.rc = rc


class CheckpointCpu(soa.SoaCpu):
    """SoaCpu on the variant library, with Engine.export_groups(heap=, device=),
    Engine.import_groups on snapshots with a heap section, and
    Engine.collect_entry_ranges."""

    def __init__(self, **kw):
        lib()
        super().__init__(**kw)

    def close(self):
        if getattr(self, "h", None):
            lib().soa_destroy(self.h)
            self.h = None

    def fault_summary(self):
        return self.faults()

    def collect_entry_ranges(self, replicas, los, his, cmds=True):
        args, keep = entry_ranges_args(replicas, los, his)
        return entry_list_call(lib().soa_collect_entry_ranges, "soa_collect_entry_ranges",
                               self.h, *args, 0 if cmds else RBE_ENTRIES_NO_CMDS)

    def export_groups(self, first=0, count=None, cap=None, heap=False, device=False):
        count = self.n_groups - first if count is None else count
        if not (heap or device):
            return super().export_groups(first, count, cap)
        return export_ex_call(lib().soa_export_groups_ex, self.h, first, count,
                              RBE_EXPORT_HEAP if heap else 0, cap)

    def import_groups(self, snap, resume=False):
        rc = lib().soa_import_groups_ck(self.h, snap, len(snap), 1 if resume else 0)
        if rc != 0:
            raise SnapshotError(rc)
