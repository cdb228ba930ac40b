"""The engine's scratch buffers across growth, reuse and re-creation
(dragonboat_amd/csrc/rbe_scratch.h): every batched reader is called on one
replica, then on the whole range, then on one replica again, and each result is
compared with the per-replica getters.

The engine has 256 C4 groups (768 replicas).  A one-replica call leaves a
reader's scratch under about 6 KiB (the 4096 bytes of slack and a few 256-byte
regions); the whole range's record arrays are tens of KiB (over a thousand
messages a round), so the second call outgrows the scratch after its count and
scan pass has written the block prefixes there: the growth that keeps a prefix.
The third call reuses the grown buffers.  A second engine created after the
first is closed repeats the whole-range calls."""
import numpy as np
import pytest

from collect_scenarios import by_replica
from parity_util import C4, view_diff

pytestmark = pytest.mark.gpu

KW = dict(C4, n_groups=256)
FIELDS = ("type", "reject", "to", "from_", "cluster_id", "term", "log_term", "log_index",
          "commit", "hint", "hint_high", "n_entries")


def _stepped(E, rounds=None):
    """(engine, rounds): stepped until one round's Updates carry messages,
    ReadyToReads, entries to save and entries to apply (or `rounds` rounds)."""
    eng = E.Engine(device=0, trace=True, **KW)
    for rnd in range(1, 301):
        eng.step()
        if rounds is not None:
            if rnd == rounds:
                return eng, rnd
            continue
        if rnd < 40:
            continue
        u = np.frombuffer(bytes(eng.updates()), E.UPDATE_DTYPE)
        u = u[(u["flags"] & E.UF_HAS_UPDATE) != 0]
        if (u["n_messages"].sum() > 500 and u["n_ready_to_read"].any() and
                (u["save_lo"] <= u["save_hi"]).any() and (u["apply_lo"] <= u["apply_hi"]).any()):
            return eng, rnd
    raise AssertionError("no round with messages, ReadyToReads and entries in 300")


def _reference(E, eng):
    """What the per-replica getters return for the last round, read once."""
    full = np.frombuffer(bytes(eng.updates()), E.UPDATE_DTYPE).copy()
    ref = dict(updates=full, has=(full["flags"] & E.UF_HAS_UPDATE) != 0, msgs=[], rtrs=[], ents={})
    for r in range(eng.n_rep):
        ref["msgs"].append([tuple(getattr(m, f) for f in FIELDS) for m in eng.messages(r)])
        ref["rtrs"].append([tuple(x) for x in eng.ready_to_reads(r)])
    for w, lo_f, hi_f in ((E.RBE_ENTRIES_TO_SAVE, "save_lo", "save_hi"),
                          (E.RBE_ENTRIES_COMMITTED, "apply_lo", "apply_hi")):
        ref["ents"][w] = {r: eng.entry_records(r, int(full[lo_f][r]), int(full[hi_f][r]))
                          for r in np.nonzero(ref["has"] & (full[lo_f] <= full[hi_f]))[0].tolist()}
    assert sum(map(len, ref["msgs"])) > 500 and any(ref["rtrs"])
    assert ref["ents"][E.RBE_ENTRIES_TO_SAVE] and ref["ents"][E.RBE_ENTRIES_COMMITTED]
    return ref


def _lists(ref, reps, off, msgs, roff, rtrs):
    """Messages and ReadyToReads of `reps`, as lists of offsets, against the getters."""
    assert off[0] == 0 and roff[0] == 0 and off[-1] == len(msgs) and roff[-1] == len(rtrs)
    for i, r in enumerate(reps):
        got = [tuple(m[f] for f in FIELDS) for m in msgs[off[i]:off[i + 1]]]
        assert got == ref["msgs"][r], (r, got, ref["msgs"][r])
        gr = [tuple(x) for x in rtrs[roff[i]:roff[i + 1]].tolist()]
        assert gr == ref["rtrs"][r], (r, gr, ref["rtrs"][r])


def _outputs(eng, ref, first, count):
    _lists(ref, range(first, first + count), *eng.collect_outputs(first, count))


def _updates(ref, first, count, rep, ups):
    want = np.nonzero(ref["has"][first:first + count])[0] + first
    assert rep.tolist() == want.tolist()
    assert ups.tobytes() == ref["updates"][want].tobytes()


def _step_lists(ref, first, count, got):
    rep, ups, moff, msgs, roff, rtrs = got
    _updates(ref, first, count, rep, ups)
    _lists(ref, [int(r) for r in rep], moff, msgs, roff, rtrs)
    for r in range(first, first + count):  # no outputs outside the listed replicas
        assert ref["has"][r] or not (ref["msgs"][r] or ref["rtrs"][r]), r


def _collect_step(eng, ref, first, count):
    _step_lists(ref, first, count, eng.collect_step(first, count))


def _collect_async(eng, ref, first, count):
    eng.collect_step_begin(first, count)
    _step_lists(ref, first, count, eng.collect_step_end())


def _collect_updates(eng, ref, first, count):
    _updates(ref, first, count, *eng.collect_updates(first, count))


def _collect_entries(eng, ref, first, count):
    for w, want in ref["ents"].items():
        got = by_replica(eng.collect_entries(first, count, which=w))
        assert got == {r: v for r, v in want.items() if first <= r < first + count}, w


READERS = (_outputs, _collect_step, _collect_async, _collect_updates, _collect_entries)


def _export(eng, other, first, count, resume=False):
    """Groups [first, first + count) of `eng` into `other`, whose views then equal eng's."""
    snap = eng.export_groups(first, count, heap=True)
    assert snap == eng.export_groups(first, count)  # (no heap: no section after the log's)
    other.import_groups(snap, resume=resume)
    n = KW["n_replicas"]
    av, bv = eng.views(first * n, count * n), other.views(first * n, count * n)
    for i in range(count * n):
        assert view_diff(av[i], bv[i]) is None, (first * n + i, view_diff(av[i], bv[i]))


def test_gpu_scratch_regrow_and_recreate(gpu_available):
    from dragonboat_amd import engine as E
    eng, rounds = _stepped(E)
    ref = _reference(E, eng)
    for reader in READERS:
        reader(eng, ref, 0, 1)          # sizes the scratch for one replica
        reader(eng, ref, 0, eng.n_rep)  # outgrows it after the count pass
        reader(eng, ref, 0, 1)          # reuses the grown buffers
    # the export, gathered on the device: the bytes the host's walk of the same
    # range writes, and importable.  Group 0 goes to a second engine at the same
    # round, then the whole engine into a fresh one (resume), then group 0 again
    other = E.Engine(device=0, trace=True, **KW)
    other.run(rounds)
    _export(eng, other, 0, 1)
    other.close()
    other = E.Engine(device=0, trace=True, **KW)
    _export(eng, other, 0, KW["n_groups"], resume=True)
    _export(eng, other, 0, 1)
    other.close()
    eng.close()
    # a fresh engine in the same process: the same round, whole-range calls
    eng, _ = _stepped(E, rounds)
    for reader in READERS:
        reader(eng, ref, 0, eng.n_rep)
    other = E.Engine(device=0, trace=True, **KW)
    _export(eng, other, 0, KW["n_groups"], resume=True)
    other.close()
    eng.close()
