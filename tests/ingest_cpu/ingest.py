"""TEST-ONLY wrapper of libingest_cpu.so: the host build of the step
(tests/soa_cpu) with the spilling inbound transport on top (ingest_cpu.cpp).

A variant build of the host library, loaded through a second copy of
tests/soa_cpu/soa.py as tests/collect_cpu/collect.py does, so the soa module
the other tests use is not touched.
"""
import ctypes as C
import importlib.util
import os

import soa_cpu.soa as _plain
from dragonboat_amd.engine import (RbeEntry, RbeMessage, RbeWireIngestStats, push_messages_call,
                                   wire_ingest_call)

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("ingest_cpu._soa_variant", _plain.__file__)
soa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(soa)
_typed = False


def lib():
    """libingest_cpu.so with soa.lib()'s signatures and the new ones."""
    global _typed
    if not _typed:
        p = os.path.join(_HERE, "libingest_cpu.so")
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
        L.soa_wire_ingest_spill.restype = C.c_int
        L.soa_wire_ingest_spill.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64,
                                            P(RbeWireIngestStats)]
        L.soa_push_messages_spill.restype = C.c_int
        L.soa_push_messages_spill.argtypes = [C.c_void_p, C.c_uint64, P(C.c_uint64),
                                              P(RbeMessage), P(RbeEntry), C.c_void_p]
        L.soa_spill_heap.restype = C.c_uint64
        L.soa_spill_heap.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
        L.soa_spill_used.restype = C.c_uint64
        L.soa_spill_used.argtypes = [C.c_void_p]
        _typed = True
    return soa.lib()


class IngestCpu(soa.SoaCpu):
    """SoaCpu on the variant library whose wire_ingest / push_messages spill
    past maxm / ecap (dragonboat_amd/csrc/rbe_ingest_spill.h)."""

    def __init__(self, **kw):
        lib()
        super().__init__(**kw)
        self.inbound_spill_bytes = 0  # what the inbound batches took of the spill heap

    def wire_ingest(self, data):
        before = lib().soa_spill_used(self.h)
        st = wire_ingest_call(lib().soa_wire_ingest_spill, self.h, data)
        self.inbound_spill_bytes += 16 * (lib().soa_spill_used(self.h) - before)
        return st

    def push_messages(self, groups, msgs, ents, cmds=None):
        before = lib().soa_spill_used(self.h)
        push_messages_call(lib().soa_push_messages_spill, self.h, groups, msgs, ents, cmds)
        self.inbound_spill_bytes += 16 * (lib().soa_spill_used(self.h) - before)

    def wire_ingest_parent(self, data):
        """The refusing form (rbe_ingest.h, as the HIP engine runs it)."""
        return wire_ingest_call(lib().soa_wire_ingest, self.h, data)

    def push_messages_parent(self, groups, msgs, ents, cmds=None):
        push_messages_call(lib().soa_push_messages, self.h, groups, msgs, ents, cmds)

    def spill_heap(self, par):
        """The bytes of the round spill heap of parity `par`."""
        n = lib().soa_spill_heap(self.h, par, None, 0)
        buf = C.create_string_buffer(max(1, n))
        lib().soa_spill_heap(self.h, par, buf, n)
        return buf.raw[:n]
