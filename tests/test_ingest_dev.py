"""The device pipeline of the spilling inbound transport on the CPU tier.

rbe_wire_ingest and rbe_push_messages keep a list past maxm and entries past
ecap in the round spill heap (dragonboat_amd/csrc/rbe_ingest_spill.h).  The
bodies of the kernels that do it are RBE_HD lane functions (ingest_walk_lane,
ingest_share_gate, ingest_share_commit); tests/ingest_dev_cpu/ingest_dev_cpu.cpp
runs them as loops in the device's order of passes beside the host build of
tests/ingest_cpu, 4 x 3 over two engines with maxm = ecap = 1, and compares
planes, count rows, arenas, spill heaps and SpillCtl after every hop.  Built
here with the address and undefined-behaviour sanitizers, as
tests/test_fast_aux.py builds its program.  The GPU twin is
test_gpu_ingest_spill.py."""
import ctypes as C
import os
import re
import subprocess

from dragonboat_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_ingest_dev_cpu(tmp_path):
    """The alignment check is off: the host engine's planes are byte vectors
    and calloc'd blocks, not the 256-byte aligned device allocations."""
    exe = tmp_path / "ingest_dev_cpu"
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize=alignment", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(HERE, "ingest_dev_cpu", "ingest_dev_cpu.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "ingest_dev_cpu ok", out.stdout + out.stderr
    # frames and push, summary-word form and plain form: each run spilled inbound
    assert len(lines) == 5 and all(" ok: " in ln for ln in lines[:4]), out.stdout
    assert len({ln.split(" ok: ")[1] for ln in lines[:4]}) == 1, out.stdout  # the same figures
    assert not out.stderr, out.stderr  # (a recovered sanitizer report)


def test_inbound_spill_stats_is_exported():
    src = open(os.path.join(ROOT, "include", "rbe.h")).read()
    assert re.search(r"^int rbe_inbound_spill_stats\(rbe_engine\* e, uint64_t\* out", src, flags=re.M)
    assert "rbe_inbound_spill_stats" in E.EXPORTS
    assert hasattr(E.Engine, "inbound_spill_stats")
    assert isinstance(E.Engine.inbound_spill_bytes, property)
    if os.path.exists(E.LIB_PATH):
        lib = C.CDLL(E.LIB_PATH)
        assert hasattr(lib, "rbe_inbound_spill_stats")
        out = (C.c_uint64 * 3)()
        assert lib.rbe_inbound_spill_stats(None, out) == E.RBE_E_INVALID


def test_the_refusals_are_documented_as_a_short_share():
    """Both calls' RBE_E_NOMEM sentences speak of the share of the spill heap,
    and no longer of maxm / ecap as limits."""
    src = open(os.path.join(ROOT, "include", "rbe.h")).read()
    assert "list over cfg.maxm messages" not in src
    assert "list exceeds cfg.maxm" not in src
    assert len(re.findall(r"share\s+(?:is|was)\s+short", src)) >= 3
