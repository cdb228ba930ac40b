"""What the batched outbox costs (rbe_collect_outbox, DESIGN.md §5 "The
Updates' messages with their entries") next to what it replaces and next to
its sibling: on a C2-shaped engine (every group appends every round, one 16-B
entry per Replicate) after a warm-up, per call and on the same engine and
round,
  rbe_collect_outbox (whole Cmds), the same with RBE_ENTRIES_NO_CMDS,
  rbe_collect_entries(RBE_ENTRIES_TO_SAVE), which moves a comparable number of
  records, and a loop of rbe_get_outbox over 1,000 of the listed senders,
  scaled to all of them;
then a second, host-driven engine whose leaders take one 1 KiB Cmd per group
per round through the payload heap: the same calls and the GB/s of Cmd bytes
delivered.  Each figure is the median of `reps` calls timed with a host clock
(every call ends in a stream synchronisation), a fresh round before each.
RBE_COLLECT_STAGE=0 / 1 selects how the entries passes store their 72-B
records (a lane each / staged in LDS and written as 16-B words); the script
runs itself once per form in a child process, alternating, and prints one
JSON line.
    python3 scripts/collect_outbox_cost.py [groups] [reps]"""
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
    from dragonboat_amd.engine import (RBE_ENTRIES_NO_CMDS, RBE_ENTRIES_TO_SAVE, RbeEntry,
                                       RbeEntryList, RbeMessage, RbeOutboxList)
    lib, h, n_rep = eng.lib, eng.h, eng.n_rep
    ob, lst = RbeOutboxList(), RbeEntryList()

    def outbox(flags):
        rc = lib.rbe_collect_outbox(h, 0, n_rep, flags, -1, C.byref(ob))
        assert rc == 0, rc

    def save():
        rc = lib.rbe_collect_entries(h, 0, n_rep, RBE_ENTRIES_TO_SAVE, C.byref(lst))
        assert rc == 0, rc

    t = {k: [] for k in ("outbox", "outbox_no_cmds", "save")}
    shape = {}
    for _ in range(reps + 2):  # (the first two rounds size the buffers)
        if push:
            push()
        eng.step()
        eng.sync()
        t["outbox"].append(timed(lambda: outbox(0)))
        shape["outbox"] = dict(senders=ob.n, messages=ob.n_messages, entries=ob.n_entries,
                               cmd_bytes=ob.cmd_bytes)
        t["outbox_no_cmds"].append(timed(lambda: outbox(RBE_ENTRIES_NO_CMDS)))
        t["save"].append(timed(save))
        shape["save"] = dict(replicas=lst.n, entries=lst.n_entries, cmd_bytes=lst.cmd_bytes)
    out = {k + "_ms": med(v[2:]) for k, v in t.items()}
    out.update(shape)
    out["outbox_over_save"] = out["outbox_ms"] / out["save_ms"]
    # the per-replica call over 1,000 of the senders the list names
    outbox(0)
    n = min(1000, ob.n)
    senders = [ob.replica[i * (ob.n // n)] for i in range(n)] if n else []
    msgs, ents = (RbeMessage * 64)(), (RbeEntry * 256)()
    buf = C.create_string_buffer(1 << 20)
    nm, ne, nc = C.c_uint32(), C.c_uint32(), C.c_uint64()

    def loop():
        for r in senders:
            rc = lib.rbe_get_outbox(h, r, msgs, 64, C.byref(nm), ents, 256, C.byref(ne), buf,
                                    len(buf), C.byref(nc))
            assert rc == 0 and nm.value <= 64 and ne.value <= 256

    if n:
        per = timed(loop) / n
        out.update(get_outbox_ms_per_replica=per, get_outbox_ms_scaled=per * ob.n,
                   get_outbox_over_outbox=per * ob.n / out["outbox_ms"])
    if out["outbox"]["cmd_bytes"]:
        out["outbox_cmd_gb_per_s"] = out["outbox"]["cmd_bytes"] / out["outbox_ms"] / 1e6
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


if os.environ.get("OUTBOX_COST_CHILD"):
    child()
else:
    res = {}
    for stage in ("1", "0", "1", "0"):  # alternating, two runs of each form
        env = dict(os.environ, OUTBOX_COST_CHILD="1", RBE_COLLECT_STAGE=stage)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            sys.exit(p.returncode)
        res.setdefault("lds_staged" if stage == "1" else "direct", []).append(
            json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(groups=groups, reps=reps, **res)))
