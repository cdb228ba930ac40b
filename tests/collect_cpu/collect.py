"""TEST-ONLY wrapper of libcollect_cpu.so: the host build of the step
(tests/soa_cpu) with the batched entry collection on top (collect_cpu.cpp).

The library is a variant build of the host library: soa_cpu.cpp unchanged plus
three functions.  It gets a module of its own — a second copy of
tests/soa_cpu/soa.py, loaded under another name and pointed at the variant the
way soa.lib() takes any variant (SOA_LIB) — so every call of a CollectCpu, of
whatever kind, resolves `lib()` to the variant, and the soa module the other
tests use is not touched.
"""
import ctypes as C
import importlib.util
import os

import numpy as np

import soa_cpu.soa as _plain
from dragonboat_amd.engine import (RBE_ENTRIES_NO_CMDS, RBE_ENTRIES_TO_SAVE, UPDATE_DTYPE,
                                   RbeEntryList, RbeUpdate, entry_list_call, entry_ranges_args)

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("collect_cpu._soa_variant", _plain.__file__)
soa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(soa)
_typed = False


def lib():
    """libcollect_cpu.so with soa.lib()'s signatures and the new ones."""
    global _typed
    if not _typed:
        p = os.path.join(_HERE, "libcollect_cpu.so")
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
        L.soa_collect_entries.restype = C.c_int
        L.soa_collect_entries.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                          C.POINTER(RbeEntryList)]
        L.soa_collect_entry_ranges.restype = C.c_int
        L.soa_collect_entry_ranges.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, u64p,
                                               C.c_uint32, C.POINTER(RbeEntryList)]
        L.soa_get_updates.restype = C.c_int
        L.soa_get_updates.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(RbeUpdate)]
        _typed = True
    return soa.lib()


class CollectCpu(soa.SoaCpu):
    """SoaCpu on the variant library, with Engine.collect_entries /
    Engine.collect_entry_ranges and the Updates."""

    def __init__(self, **kw):
        lib()
        super().__init__(**kw)

    def collect_entries(self, first=0, count=None, which=RBE_ENTRIES_TO_SAVE, cmds=True):
        count = self.n_rep - first if count is None else count
        return entry_list_call(lib().soa_collect_entries, "soa_collect_entries", self.h, first,
                               count, which | (0 if cmds else RBE_ENTRIES_NO_CMDS))

    def collect_entry_ranges(self, replicas, los, his, cmds=True):
        args, keep = entry_ranges_args(replicas, los, his)
        return entry_list_call(lib().soa_collect_entry_ranges, "soa_collect_entry_ranges",
                               self.h, *args, 0 if cmds else RBE_ENTRIES_NO_CMDS)

    def updates(self, first=0, count=None):
        """The last round's Updates (Engine.updates) as a numpy array."""
        count = self.n_rep - first if count is None else count
        arr = (RbeUpdate * max(1, count))()
        rc = lib().soa_get_updates(self.h, first, count, arr)
        if rc:
            raise RuntimeError(f"soa_get_updates rc={rc}")
        return np.frombuffer(arr, dtype=UPDATE_DTYPE)[:count].copy()
