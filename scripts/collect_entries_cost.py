"""What the batched read of the Updates' entries costs (rbe_collect_entries,
DESIGN.md §5 "Outputs") next to what it replaces: on a C2-shaped engine
(every group appends every round) after a warm-up, per call and on the same
engine and round,
  rbe_collect_entries(RBE_ENTRIES_TO_SAVE), rbe_collect_entries(
  RBE_ENTRIES_COMMITTED), the same with RBE_ENTRIES_NO_CMDS, rbe_collect_step,
  and a loop of rbe_get_entries + rbe_get_entry_cmds over 1,000 of the listed
  replicas, scaled to all of them;
then a second, host-driven engine whose leaders take one 1 KiB Cmd per group
per round through the payload heap: the same calls and the GB/s of Cmd bytes
delivered.  Each figure is the median of `reps` calls timed with a host clock
(every call ends in a stream synchronisation), a fresh round before each.
RBE_COLLECT_STAGE=0 / 1 selects how k_ce_entries stores its 72-B records (a
lane each / staged in LDS and written as 16-B words); the script runs itself
once per form in a child process and prints one JSON line.
    python3 scripts/collect_entries_cost.py [groups] [reps]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

groups = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
WARM = 120


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(eng, push=None):
    from dragonboat_amd.engine import (RBE_ENTRIES_COMMITTED, RBE_ENTRIES_NO_CMDS,
                                       RBE_ENTRIES_TO_SAVE, RbeEntry, RbeEntryList, RbeStepOutputs)
    lib, h, n_rep = eng.lib, eng.h, eng.n_rep
    lst, so = RbeEntryList(), RbeStepOutputs()

    def collect(flags):
        rc = lib.rbe_collect_entries(h, 0, n_rep, flags, C.byref(lst))
        assert rc == 0, rc

    def step_outputs():
        rc = lib.rbe_collect_step(h, 0, n_rep, 0, C.byref(so))
        assert rc == 0, rc

    t = {k: [] for k in ("save", "committed", "save_no_cmds", "committed_no_cmds",
                         "collect_step")}
    shape = {}
    for _ in range(reps + 2):  # (the first two rounds size the buffers)
        if push:
            push()
        eng.step()
        eng.sync()
        for k, f in (("save", RBE_ENTRIES_TO_SAVE), ("committed", RBE_ENTRIES_COMMITTED),
                     ("save_no_cmds", RBE_ENTRIES_TO_SAVE | RBE_ENTRIES_NO_CMDS),
                     ("committed_no_cmds", RBE_ENTRIES_COMMITTED | RBE_ENTRIES_NO_CMDS)):
            t[k].append(timed(lambda: collect(f)))
            if k in ("save", "committed"):
                shape[k] = dict(replicas=lst.n, entries=lst.n_entries, cmd_bytes=lst.cmd_bytes)
        t["collect_step"].append(timed(step_outputs))
        shape["collect_step"] = dict(updates=so.n, messages=so.n_messages)
    out = {k + "_ms": med(v[2:]) for k, v in t.items()}
    out.update(shape)
    # the per-replica getters over 1,000 of the replicas the save list names
    collect(RBE_ENTRIES_TO_SAVE)
    n = min(1000, lst.n)
    ranges = [(lst.replica[i], lst.entries[lst.ent_off[i]].index,
               lst.entries[lst.ent_off[i + 1] - 1].index) for i in range(n)]
    buf, offs = C.create_string_buffer(1 << 20), (C.c_uint64 * 4096)()

    def loop():
        for r, lo, hi in ranges:
            arr = (RbeEntry * (hi - lo + 1))()
            assert lib.rbe_get_entries(h, r, lo, hi, arr) == 0
            assert lib.rbe_get_entry_cmds(h, r, lo, hi, buf, len(buf), offs) == 0

    if n:
        per = timed(loop) / n
        out.update(getters_ms_per_replica=per, getters_ms_scaled=per * lst.n)
    if out["save"]["cmd_bytes"]:
        out["save_cmd_gb_per_s"] = out["save"]["cmd_bytes"] / out["save_ms"] / 1e6
        out["committed_cmd_gb_per_s"] = out["committed"]["cmd_bytes"] / out["committed_ms"] / 1e6
    n_f, bits = eng.fault_summary()
    out["faults"] = n_f
    return out


def child():
    from dragonboat_amd.engine import Engine
    eng = Engine(device=0, n_groups=groups, n_replicas=3, wl_enabled=True, wl_start_round=30,
                 ring=64)
    eng.run(WARM)
    small = measure(eng)
    eng.close()
    # 1 KiB heap Cmds: a proposal per group per round at the group's leader
    import numpy as np
    g2 = max(1, groups // 4)
    eng = Engine(device=0, n_groups=g2, n_replicas=3, ext_inputs=True, ring=64,
                 heap_bytes=min(4 << 30, g2 * 1056 * 24))
    eng.run(40)
    role = np.array([v.role for v in eng.views()])
    leaders = [int(r) for r in np.flatnonzero(role == 2)]  # (oracle.LEADER)
    cmd = bytes(range(256)) * 4

    def push():
        eng.push_proposals(leaders, [[(0, cmd)]] * len(leaders))

    for _ in range(8):
        push()
        eng.step()
    big = measure(eng, push)
    big["groups"], big["leaders"] = g2, len(leaders)
    eng.close()
    print(json.dumps(dict(stage=os.environ.get("RBE_COLLECT_STAGE", "1"), inline=small,
                          heap_1k=big)))


if os.environ.get("COLLECT_COST_CHILD"):
    child()
else:
    res = {}
    for stage in ("1", "0", "1", "0"):  # alternating, two runs of each form
        env = dict(os.environ, COLLECT_COST_CHILD="1", RBE_COLLECT_STAGE=stage)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            sys.exit(p.returncode)
        res.setdefault("lds_staged" if stage == "1" else "direct", []).append(
            json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(groups=groups, reps=reps, **res)))
