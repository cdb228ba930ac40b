#!/usr/bin/env python3
"""Cost of a whole-engine checkpoint on one MI355X.

Two states, snapshots off, stepped until every replica has several cold pages:
  plain  --groups x 3, the built-in workload (a proposal per group per round)
  heap   the same with cfg.heap_bytes and, every --heap-every-th round, a 1 KiB
         proposal at every group's leader
On each, three calls on the same state, each the median of repeated calls
after a warm-up call:
  rbe_export_bytes + rbe_export_groups   (one blocking copy per page)
  rbe_export_groups_ex(0)                (the device gather, sizing + filling)
  rbe_export_groups_ex(RBE_EXPORT_HEAP)
and the heap section's size and GB/s.  --profile DIR runs the measurement once
more in a child process under `rocprofv3 --kernel-trace --stats` and prints the
kernel times of the page-copy (k_ck_pages) and record-copy (k_ck_records)
passes.  Prints one JSON line per state.
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()  # warm-up: buffers grown, code loaded
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def heap_section_at(snap):
    """Where the heap section starts: after the planes and the log section (rbe_snap.h)."""
    body = int.from_bytes(snap[64:72], "little")
    return ((96 + body + 15) & ~15) + int.from_bytes(snap[88:96], "little")


def measure(a, heap):
    from dragonboat_amd.engine import Engine
    kw = dict(n_groups=a.groups, n_replicas=3, ring=a.ring, wl_enabled=True, wl_start_round=30)
    if heap:
        kw.update(ext_inputs=True, heap_bytes=a.heap_bytes)
    eng = Engine(device=0, **kw)
    if heap:
        # on top of the workload, every --heap-every-th round a 1 KiB proposal
        # at every group's leader, marshalled with numpy (a Python list of
        # 100k batches a round would dominate the run)
        import ctypes as C

        import numpy as np
        done = 0
        while done < a.rounds:
            k = min(a.heap_every, a.rounds - done)
            eng.run(k)
            done += k
            if done < 30 or done >= a.rounds:
                continue
            lead = np.nonzero(eng.views_np()["role"] == 2)[0].astype(np.uint64)
            n = len(lead)
            if not n:
                continue
            one, typ = np.ones(n, np.uint32), np.zeros(n, np.uint32)
            lens = np.full(n, 1024, np.uint32)
            blob = np.random.default_rng(done).integers(0, 256, n * 1024, dtype=np.uint8)
            p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
            rc = eng.lib.rbe_push_proposals(eng.h, n, lead.ctypes.data_as(p64),
                                            one.ctypes.data_as(p32), typ.ctypes.data_as(p32),
                                            lens.ctypes.data_as(p32),
                                            blob.ctypes.data_as(C.POINTER(C.c_uint8)))
            assert rc == 0, f"rbe_push_proposals rc={rc}"
    else:
        eng.run(a.rounds)
    eng.sync()
    res = dict(state="heap" if heap else "plain", groups=a.groups, rounds=a.rounds, ring=a.ring)
    if a.old_reps:
        t, old = timed(lambda: eng.export_groups(), a.old_reps)
        res.update(old_s=t, bytes=len(old))
    t, new = timed(lambda: eng.export_groups(device=True), a.reps)
    res.update(ex0_s=t, bytes=len(new))
    if a.old_reps:
        res["identical"] = new == old
    body_log = heap_section_at(new)
    res["log_bytes"] = int.from_bytes(new[88:96], "little")
    res["pages"] = (res["log_bytes"] - 16 * 3 * a.groups) // 2064
    if heap:
        t, full = timed(lambda: eng.export_groups(heap=True), a.reps)
        sec = len(full) - body_log
        res.update(exheap_s=t, heap_section_bytes=sec,
                   heap_records=int.from_bytes(full[body_log + 8:body_log + 16], "little"),
                   heap_section_gbps=sec / max(t - res["ex0_s"], 1e-9) / 1e9)
    eng.close()
    print(json.dumps(res), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--groups", type=int, default=100000)
    p.add_argument("--rounds", type=int, default=300)
    p.add_argument("--ring", type=int, default=8)
    p.add_argument("--heap-bytes", type=int, default=2 << 30)
    p.add_argument("--heap-every", type=int, default=16)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--old-reps", type=int, default=1, help="0 skips the per-page export")
    p.add_argument("--states", default="plain,heap")
    p.add_argument("--profile", default="", help="directory for a rocprofv3 kernel trace")
    a = p.parse_args()
    for st in a.states.split(","):
        measure(a, st == "heap")
    if a.profile:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.profile, "-o", "run",
               "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--groups", str(a.groups), "--rounds", str(a.rounds), "--ring", str(a.ring),
               "--heap-bytes", str(a.heap_bytes), "--heap-every", str(a.heap_every), "--reps", "1", "--old-reps", "0",
               "--states", "heap" if "heap" in a.states else "plain"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        for f in glob.glob(os.path.join(a.profile, "**", "*kernel_stats.csv"), recursive=True):
            lines = open(f).read().splitlines()
            print(lines[0])
            for ln in lines[1:]:
                if "k_ck_" in ln:
                    print(ln)


if __name__ == "__main__":
    main()
