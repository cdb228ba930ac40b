"""TEST-ONLY wrapper of liblaunch_cpu.so: the host build of the step
(tests/soa_cpu) with the paged rbe_launch on top (launch_cpu.cpp), and
optionally a host tier under the cold log (host_pool_bytes).

As tests/collect_cpu/collect.py does, the variant library gets a copy of
tests/soa_cpu/soa.py of its own, loaded under another name and pointed at the
variant through SOA_LIB, so the soa module the other tests use is not touched.
"""
import ctypes as C
import importlib.util
import os

import soa_cpu.soa as _plain
from dragonboat_amd.engine import make_config

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("launch_cpu._soa_variant", _plain.__file__)
soa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(soa)
_typed = False


def lib():
    """liblaunch_cpu.so with soa.lib()'s signatures and the new ones."""
    global _typed
    if not _typed:
        p = os.path.join(_HERE, "liblaunch_cpu.so")
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
        L.lc_create.restype = C.c_void_p
        L.lc_create.argtypes = [C.c_void_p]
        L.lc_launch.restype = C.c_int
        L.lc_launch.argtypes = [C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lc_tier_stats.argtypes = [C.c_void_p, u64p]
        L.lc_chain.restype = C.c_uint32
        L.lc_chain.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), u64p, C.c_uint32]
        L.lc_mflags.restype = C.c_uint32
        L.lc_mflags.argtypes = [C.c_void_p, C.c_uint64]
        _typed = True
    return soa.lib()


class LaunchCpu(soa.SoaCpu):
    """SoaCpu on the variant library.  `paged` selects what launch() calls:
    lc_launch (the passes of rbe_launch.h, as the HIP engine) or the serial
    soa_launch.  host_pool_bytes gives the engine a host tier."""

    def __init__(self, paged=True, full_only=False, staged=0, **kw):
        L = lib()
        self.paged = paged
        self.cfg = make_config(**kw)
        self.h = L.lc_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("lc_create failed")
        ng = C.c_uint64()
        L.soa_local_groups(self.h, C.byref(ng), None)
        self.n_groups = ng.value
        self.n_rep = self.n_groups * self.cfg.n_replicas
        L.soa_set_full_only(self.h, int(full_only))
        L.soa_set_staged(self.h, int(staged))

    def _input(self, name, *args):
        if name == "launch" and self.paged:
            return lib().lc_launch(self.h, *args)
        return getattr(lib(), "soa_" + name)(self.h, *args)

    def tier_stats(self):
        """Host pages in use / in total (Engine.cold_tier_stats' first two)."""
        out = (C.c_uint64 * 2)()
        lib().lc_tier_stats(self.h, out)
        return dict(host_pages_used=out[0], host_pages=out[1])

    def chain(self, replica, cap=64):
        """[(page id, page number)] of a replica's cold log from its head."""
        pages, pns = (C.c_uint32 * cap)(), (C.c_uint64 * cap)()
        n = lib().lc_chain(self.h, replica, pages, pns, cap)
        assert n != 0xFFFFFFFF and n <= cap, f"broken chain of replica {replica}"
        return [(pages[i], pns[i]) for i in range(n)]

    def mflags(self, replica):
        return lib().lc_mflags(self.h, replica)

    def entries(self, replica, lo, hi):
        return [(d["index"], d["term"], d["type"], d["cmd"])
                for d in self.entry_records(replica, lo, hi)]
