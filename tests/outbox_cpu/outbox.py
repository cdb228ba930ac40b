"""TEST-ONLY wrapper of liboutbox_cpu.so: the host build of the step
(tests/soa_cpu) with the spilling inbound transport (tests/ingest_cpu) and the
batched outbox on top (outbox_cpu.cpp).

A variant build of the host library, loaded through a second copy of
tests/soa_cpu/soa.py as tests/collect_cpu/collect.py does, so the soa module
the other tests use is not touched.
"""
import ctypes as C
import importlib.util
import os

import soa_cpu.soa as _plain
from dragonboat_amd.engine import (RbeEntry, RbeMessage, RbeOutboxList, outbox_list_call,
                                   push_messages_call)

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("outbox_cpu._soa_variant", _plain.__file__)
soa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(soa)
_typed = False


def lib():
    """liboutbox_cpu.so with soa.lib()'s signatures and the new ones."""
    global _typed
    if not _typed:
        p = os.path.join(_HERE, "liboutbox_cpu.so")
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
        L.soa_collect_outbox.restype = C.c_int
        L.soa_collect_outbox.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.c_int32, P(RbeOutboxList)]
        L.soa_outbox_extra_blocks.argtypes = [C.c_uint64]
        L.soa_push_messages_spill.restype = C.c_int
        L.soa_push_messages_spill.argtypes = [C.c_void_p, C.c_uint64, P(C.c_uint64),
                                              P(RbeMessage), P(RbeEntry), C.c_void_p]
        L.soa_spill_used.restype = C.c_uint64
        L.soa_spill_used.argtypes = [C.c_void_p]
        _typed = True
    return soa.lib()


class OutboxCpu(soa.SoaCpu):
    """SoaCpu on the variant library, with Engine.collect_outbox; push_messages
    spills past maxm / ecap as the HIP engine's does."""

    def __init__(self, **kw):
        lib()
        super().__init__(**kw)
        self.inbound_spill_bytes = 0  # what the inbound batches took of the spill heap

    def collect_outbox(self, first=0, count=None, remote_only=False, dst_rank=-1, cmds=True,
                       raw=False):
        count = self.n_rep - first if count is None else count
        return outbox_list_call(lib().soa_collect_outbox, "soa_collect_outbox", self.h, first,
                                count, remote_only, dst_rank, cmds, raw)

    def push_messages(self, groups, msgs, ents, cmds=None):
        before = lib().soa_spill_used(self.h)
        push_messages_call(lib().soa_push_messages_spill, self.h, groups, msgs, ents, cmds)
        self.inbound_spill_bytes += 16 * (lib().soa_spill_used(self.h) - before)
