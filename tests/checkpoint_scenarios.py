"""Self-contained checkpoints (rbe_export_groups_ex with RBE_EXPORT_HEAP, the
heap section of rbe_import_groups; dragonboat_amd/csrc/rbe_checkpoint.h): the
scenarios, shared by the host build (tests/test_checkpoint.py) and the HIP
engine (tests/test_gpu_checkpoint.py).  `mk(**kw)` builds an engine of the
tier under test; both have export_groups(heap=, device=), import_groups,
entry_cmds, collect_entry_ranges and the node inputs.

A source run is computed once per tier and shape and shared, unchanged, by the
scenarios that read it."""
import random
import re
import struct

import numpy as np

import oracle as O
from dragonboat_amd.engine import RBE_E_INVALID, RBE_E_NOMEM, RBE_E_STATE
from heap_util import check_logs, mixed_cmd
from input_util import apply_engine, apply_oracle, plan_round, run_driven
from parity_util import C2, C3, view_diff

HEAP_MAGIC = 0x3150414548454252  # "RBEHEAP1"
HEAP_HDR = 32  # the 32-B record header {Key, ClientID, SeriesID, RespondedTo}


def rc_of(fn, *a, **kw):
    """0, or the rc of the error the call raised."""
    try:
        fn(*a, **kw)
    except Exception as e:  # EngineError / SnapshotError / InputError of either tier
        rc = getattr(e, "rc", None)
        if rc is None:  # (an EngineError carries it in its text)
            m = re.search(r"rc=(-?\d+)", str(e))
            if not m:
                raise
            rc = int(m.group(1))
        return rc
    return 0


def heap_section_at(snap):
    """Where a heap section would start: after the planes and the log section."""
    body, = struct.unpack_from("<Q", snap, 64)
    log_bytes, = struct.unpack_from("<Q", snap, 88)
    return ((96 + body + 15) & ~15) + log_bytes


def parse_heap_section(snap):
    """(head, cap, [(pos, len)], [record bytes]) of a snapshot's heap section,
    or None when it has none."""
    at = heap_section_at(snap)
    if len(snap) < at + 32:
        return None
    magic, n, head, cap = struct.unpack_from("<QQQQ", snap, at)
    if magic != HEAP_MAGIC:
        return None
    rows = [struct.unpack_from("<QII", snap, at + 32 + 16 * i) for i in range(n)]
    assert all(pad == 0 for _, _, pad in rows)
    off = at + 32 + 16 * n
    recs = []
    for pos, ln, _ in rows:
        rb = (HEAP_HDR + ln + 15) & ~15
        recs.append(snap[off:off + rb])
        off += rb
    assert off == len(snap), "the section ends with its last record"
    return head, cap, [(p, l) for p, l, _ in rows], recs


def views_equal(a, b):
    av, bv = a.views(), b.views()
    return all(view_diff(av[i], bv[i]) is None for i in range(len(av)))


def whole_logs(eng):
    """collect_entry_ranges over every replica's whole log, as comparable bytes."""
    v = eng.views()
    reps = [r for r in range(eng.n_rep) if v[r].last_index]
    rep, eoff, ents, coff, cmds = eng.collect_entry_ranges(
        reps, [1] * len(reps), [v[r].last_index for r in reps])
    return rep, eoff, ents, coff, cmds


def logs_equal(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def read_each(eng):
    """Every replica's every index read alone: its Cmd bytes, or the rc."""
    v = eng.views()
    out = {}
    for r in range(eng.n_rep):
        for i in range(1, v[r].last_index + 1):
            try:
                out[r, i] = eng.entry_cmds(r, i, i)[0]
            except Exception as e:
                assert f"rc={RBE_E_STATE}" in str(e), e
                out[r, i] = RBE_E_STATE
    return out


def drive_on(engs, ref, rounds, seed, cmd, density, on_ops=None):
    """`rounds` more driven rounds (input_util.plan_round) with the same input
    at every engine of `engs` and at the oracle, every view compared each
    round.  A proposal batch fails at all engines or at none, and only with
    RBE_E_NOMEM; the oracle then gets none of the round's input either.  (The
    counters of a resumed engine restart at zero, so run_driven's closing
    comparison of them does not apply.)"""
    rng = random.Random(seed)
    n, n_rep = engs[0].cfg.n_replicas, engs[0].n_rep
    views = ref.views()
    for rnd in range(rounds):
        ops = plan_round(rng, n_rep, n, rnd, views, False, density, [0] * n_rep, cmd)
        if on_ops:
            on_ops(ops)
        rcs = [rc_of(apply_engine, e, ops) for e in engs]
        assert len(set(rcs)) == 1 and rcs[0] in (0, RBE_E_NOMEM), (rnd, rcs)
        if rcs[0] == 0:
            apply_oracle(ref, ops)
        for e in engs + [ref]:
            e.step()
        views = ref.views()
        for e in engs:
            ev = e.views()
            for i in range(n_rep):
                assert view_diff(ev[i], views[i]) is None, (rnd, i, view_diff(ev[i], views[i]))


# ---------------------------------------------------------------- 1. identity
def identity(mk, kw, rounds, tier_stats=False):
    """_ex(flags = 0) equals export_groups() byte for byte; returns the bytes."""
    eng = mk(**kw)
    eng.run(rounds)
    if tier_stats:
        assert eng.cold_tier_stats()["demoted"] > 0, "no page reached the host tier"
    old = eng.export_groups()
    assert old[88:96] != b"\0" * 8, "no cold log in the snapshot"
    new = eng.export_groups(device=True)
    assert new == old
    # a range, and a heap flag without a heap: no section
    assert eng.export_groups(3, 5, device=True) == eng.export_groups(3, 5)
    assert eng.export_groups(heap=True) == old
    eng.close()
    return old


TIER_KW = dict(dict(C2, n_groups=16), ring=8, pool_bytes=256 << 10, host_pool_bytes=2 << 20)
TIER_ROUNDS = 200


# ---------------------------------------------------------------- 2 - 4. resume
HEAP_KW = dict(C2, n_groups=8, ext_inputs=True, max_entry_size=0)
_SRC = {}


def heap_source(mk, tag):
    """The test_payload_heap shape after 150 driven rounds: everything the
    resume scenarios compare with, taken before the source engine is closed."""
    if tag not in _SRC:
        eng = mk(heap_bytes=64 << 20, ring=64, **HEAP_KW)
        ref = O.Harness(**HEAP_KW)
        pushed = set()

        def keep(ops):
            for kind, _, a in ops:
                if kind == "prop":
                    pushed.update(c for _, c in a if len(c) > 16)

        d = run_driven(eng, ref, 150, seed=5, cmd=mixed_cmd, on_ops=keep, density=0.25)
        assert d is None, f"first divergence {d}"
        s = dict(ref=ref, pushed=pushed, keep=keep, logs=whole_logs(eng),
                 plain=eng.export_groups(), snap=eng.export_groups(heap=True))
        assert eng.export_groups(device=True) == s["plain"]
        eng.close()
        _SRC[tag] = s
    return _SRC[tag]


def resume_fresh(mk, tag):
    s = heap_source(mk, tag)
    ref = s["ref"]  # (the only scenario that steps the shared oracle on)
    n = HEAP_KW["n_replicas"]
    # a plain export resumes with the logs pointing into an empty heap
    gap = mk(heap_bytes=64 << 20, ring=64, **HEAP_KW)
    gap.import_groups(s["plain"], resume=True)
    v = ref.views()
    bad = 0
    for r in range(gap.n_rep):
        if v[r].last_index:
            bad += rc_of(gap.entry_cmds, r, 1, v[r].last_index) == RBE_E_STATE
    assert bad > 0, "a plain export of a heap engine read back whole"
    gap.close()
    b = mk(heap_bytes=64 << 20, ring=64, **HEAP_KW)
    b.import_groups(s["snap"], resume=True)
    assert b.export_groups(heap=True) == s["snap"]
    assert check_logs(b, HEAP_KW["n_groups"], n, ref.views(), 64, s["pushed"]) > 50
    assert logs_equal(whole_logs(b), s["logs"])
    drive_on([b], ref, 40, 6, mixed_cmd, 0.25, on_ops=s["keep"])
    b.run(20)  # one stretch through the K-round path
    ref.run(20)
    ev, rv = b.views(), ref.views()
    for i in range(len(rv)):
        assert view_diff(ev[i], rv[i]) is None, (i, view_diff(ev[i], rv[i]))
    assert b.faults()[0] == 0
    assert check_logs(b, HEAP_KW["n_groups"], n, rv, 64, s["pushed"]) > 50
    b.close()


def section_shape(mk, tag):
    s = heap_source(mk, tag)
    head, cap, rows, recs = parse_heap_section(s["snap"])
    assert cap == 64 << 20 and rows
    for (p0, l0), (p1, _) in zip(rows, rows[1:]):
        assert p0 % 16 == 0 and p0 + ((HEAP_HDR + l0 + 15) & ~15) <= p1
    assert rows[-1][0] + HEAP_HDR + rows[-1][1] <= head
    # every log's heap Cmds: more references than records (each record once),
    # and each record's bytes are the source's read of its entry
    by_cmd = {}
    for (pos, ln), rec in zip(rows, recs):
        assert rec[HEAP_HDR + ln:] == b"\0" * (len(rec) - HEAP_HDR - ln), "bytes past the Cmd"
        assert rec[:HEAP_HDR] == b"\0" * HEAP_HDR  # (no session fields in this run)
        c = rec[HEAP_HDR:HEAP_HDR + ln]
        assert ln > 16 and c in s["pushed"], (pos, ln)
        by_cmd[c] = pos
    assert len(by_cmd) == len(rows)
    _, _, ents, coff, cmds = s["logs"]
    raw, refs = cmds.tobytes(), 0
    for j in np.nonzero(ents["cmd_len"] > 16)[0]:
        c = raw[int(coff[j]):int(coff[j]) + int(ents["cmd_len"][j])]
        assert c in by_cmd, f"entry {j} of the logs: its Cmd is in no record"
        refs += 1
    assert len(rows) < refs, (len(rows), refs)


# ---------------------------------------------------------------- 3. wrap and laps
LAPS_KW = dict(C2, n_groups=4, ext_inputs=True)


def wrap_and_laps(mk):
    a = mk(heap_bytes=256 << 10, **LAPS_KW)
    ref = O.Harness(**LAPS_KW)
    cmd = lambda rng: rng.randbytes(4000)  # noqa: E731
    d = run_driven(a, ref, 120, seed=9, cmd=cmd, density=0.3)
    assert d is None, f"first divergence {d}"
    snap = a.export_groups(heap=True)
    head, cap, rows, _ = parse_heap_section(snap)
    assert head > cap and rows[0][0] // cap != rows[-1][0] // cap, "the positions do not wrap"
    assert all(p + cap >= head for p, _ in rows)
    want = read_each(a)
    assert RBE_E_STATE in want.values() and any(isinstance(x, bytes) and len(x) == 4000
                                                for x in want.values())
    b = mk(heap_bytes=256 << 10, **LAPS_KW)
    b.import_groups(snap, resume=True)
    assert b.export_groups(heap=True) == snap
    assert read_each(b) == want
    # 30 more rounds with the same input at the source and the resumed engine:
    # a push fails at both or at neither, and both stay with the oracle
    drive_on([a, b], ref, 30, 10, cmd, 0.3)
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. in-flight forward
def inflight_forward(mk):
    kw = dict(C2, n_groups=2, ext_inputs=True)
    a = mk(heap_bytes=1 << 20, **kw)
    a.run(60)
    v = a.views()
    lead = [r for r in range(3) if v[r].role == O.LEADER]
    assert len(lead) == 1
    foll = (lead[0] + 1) % 3
    cmd = bytes(range(100))
    a.push_proposals([foll], [[(0, cmd)]])
    a.step()
    last = a.views()[lead[0]].last_index
    assert cmd not in a.entry_cmds(lead[0], max(1, last - 5), last), "already appended"
    snap = a.export_groups(heap=True)
    _, _, rows, recs = parse_heap_section(snap)
    assert any(r[HEAP_HDR:HEAP_HDR + ln] == cmd for (_, ln), r in zip(rows, recs))
    a.close()
    b = mk(heap_bytes=1 << 20, **kw)
    b.import_groups(snap, resume=True)
    b.step()
    b.step()
    last = b.views()[lead[0]].last_index
    assert cmd in b.entry_cmds(lead[0], max(1, last - 5), last)
    assert b.faults()[0] == 0
    b.close()


# ---------------------------------------------------------------- 6. hand-off
def handoff(mk):
    def driven(seed):
        e = mk(heap_bytes=64 << 20, ring=64, **HEAP_KW)
        ref = O.Harness(**HEAP_KW)
        assert run_driven(e, ref, 60, seed=seed, cmd=mixed_cmd, density=0.25) is None
        return e

    a, b = driven(5), driven(77)
    part = a.export_groups(2, 4, heap=True)
    assert parse_heap_section(part)[2], "no record in the range"
    assert len(parse_heap_section(part)[2]) < len(parse_heap_section(a.export_groups(heap=True))[2])
    before = a.export_groups(heap=True)
    a.import_groups(part)
    assert a.export_groups(heap=True) == before
    # another engine at the same round whose pushes differed holds other bytes
    mine = b.export_groups(heap=True)
    assert rc_of(b.import_groups, part) == RBE_E_STATE
    assert b.export_groups(heap=True) == mine
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. refusals
def refusals(mk, tag):
    s = heap_source(mk, tag)
    snap = s["snap"]
    at = heap_section_at(snap)
    head, cap, rows, _ = parse_heap_section(snap)
    assert len(rows) > 2

    def patched(off, fmt, *vals):
        b = bytearray(snap)
        struct.pack_into(fmt, b, at + off, *vals)
        return bytes(b)

    r0, r1 = snap[at + 32:at + 48], snap[at + 48:at + 64]
    swapped = bytearray(snap)
    swapped[at + 32:at + 64] = r1 + r0
    bad = {
        "truncated": snap[:-16],
        "cut in the table": snap[:at + 40],
        "swapped rows": bytes(swapped),
        "overlapping records": patched(48, "<Q", rows[0][0] + 16),
        "unaligned": patched(32, "<Q", rows[0][0] + 8),
        "a record past head": patched(16, "<Q", rows[-1][0] + 16),
        "a lap below head": patched(16, "<Q", rows[0][0] + cap + 16),
        "wrong cap": patched(24, "<Q", cap * 2),
        "trailing bytes": snap + b"\0" * 16,
    }
    b = mk(heap_bytes=64 << 20, ring=64, **HEAP_KW)
    b.run(3)
    before = b.export_groups(heap=True)
    for name, x in bad.items():
        assert rc_of(b.import_groups, x, resume=True) == RBE_E_INVALID, name
        assert b.export_groups(heap=True) == before, name
    # inputs staged since the last step
    b.push_proposals([0], [[(0, b"x" * 40)]])
    assert rc_of(b.import_groups, snap, resume=True) == RBE_E_STATE
    b.step()
    # trailing bytes without the magic are ignored, as before the section existed
    b.import_groups(s["plain"] + b"\x01" * 24, resume=True)
    b.import_groups(snap, resume=True)
    assert b.export_groups(heap=True) == snap
    # a short cap: RBE_E_NOMEM with the size set
    try:
        b.export_groups(cap=64, heap=True)
    except Exception as e:
        assert e.rc == RBE_E_NOMEM and e.bytes_needed == len(snap)
    else:
        raise AssertionError("a 64-byte buffer took the export")
    b.close()
