"""The cold log's host tier on the CPU tier (cfg.host_pool_bytes;
dragonboat_amd/csrc/rbe_spill.h): a second tier of cold log pages under the
HBM page pool, filled by a demotion pass after each round (the plan relinks a
replica's chain onto host pages, the copy carries the entries and frees the
HBM pages).  tests/cold_tier_cpu is the host build of exactly those functions
over malloc'd tiers; here a Python model follows every operation.

Also two checks of the engine as it stands without the tier, through the host
build of the step (tests/soa_cpu): the small pools the GPU tests give a tiered
engine (test_gpu_cold_tier.py) do run out without it, and the small ring they
use is bit-exact with the default pool."""
import ctypes as C
import os
import random

import pytest

import oracle as O
from parity_util import C2, counters_match, run_lockstep
from soa_cpu.soa import SoaCpu
from test_spill import LONG_ISO

PAGE = 64  # kPageEnts
_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        p = os.path.join(_HERE, "cold_tier_cpu", "libcold_tier_cpu.so")
        if not os.path.exists(p):
            raise RuntimeError(f"{p} missing: run __graft_entry__.build()")
        L = C.CDLL(p)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        L.ct_create.restype = vp
        L.ct_create.argtypes = [u32, u32, u32, u32]
        L.ct_destroy.argtypes = [vp]
        L.ct_put.restype = C.c_int
        L.ct_put.argtypes = [vp, u32, u64, u64, u64, u32]
        L.ct_get.restype = C.c_int
        L.ct_get.argtypes = [vp, u32, u64, C.POINTER(u64)]
        L.ct_demote.restype = u32
        L.ct_demote.argtypes = [vp, C.POINTER(u64), u32, C.c_int]
        L.ct_release.argtypes = [vp, u32, u64, u32]
        L.ct_chain.restype = u32
        L.ct_chain.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u64), u32]
        L.ct_stats.argtypes = [vp, C.POINTER(u64)]
        _lib = L
    return _lib


ALL = (1 << 64) - 1


class Tiers:
    """The harness with its model: per replica {index: value} of every entry the
    chain holds and {page number: on the host} of its pages."""

    def __init__(self, pool_pages, host_pages, n_rep, mv_cap):
        self.h = lib().ct_create(pool_pages, host_pages, n_rep, mv_cap)
        self.pool_pages, self.host_pages, self.n, self.mv_cap = pool_pages, host_pages, n_rep, mv_cap
        self.ents = [dict() for _ in range(n_rep)]
        self.pages = [dict() for _ in range(n_rep)]
        self.last = [0] * n_rep
        self.commit = [0] * n_rep
        self.par = 0
        self.stamp = 0

    def close(self):
        lib().ct_destroy(self.h)

    def stats(self):
        out = (C.c_uint64 * 10)()
        lib().ct_stats(self.h, out)
        return dict(zip(("live", "hlive", "bump", "hbump", "demoted", "passes", "mv0", "mv1", "oom",
                         "hpool_first"), out))

    def chain(self, r):
        cap = self.pool_pages + self.host_pages
        pg, pn = (C.c_uint32 * cap)(), (C.c_uint64 * cap)()
        n = lib().ct_chain(self.h, r, pg, pn, cap)
        assert n != 0xFFFFFFFF, f"replica {r}: broken chain links"
        return [(pg[i], pn[i]) for i in range(n)]

    def model_live(self):
        return sum(1 for p in self.pages for host in p.values() if not host)

    def model_host(self):
        return sum(1 for p in self.pages for host in p.values() if host)

    # -- operations
    def put(self, r, idx, value):
        self.stamp += 1
        if not lib().ct_put(self.h, r, idx, self.stamp, value, self.par):
            return False
        self.ents[r][idx] = (self.stamp, value)
        self.pages[r].setdefault(idx // PAGE, False)  # (a new page is an HBM page)
        return True

    def append(self, r, value):
        if not self.put(r, self.last[r] + 1, value):
            return False
        self.last[r] += 1
        return True

    def demote(self, force=False):
        """One pass at the model's commit indexes, then the next round."""
        commit = (C.c_uint64 * self.n)(*self.commit)
        st = self.stats()
        moved = lib().ct_demote(self.h, commit, self.par, int(force))
        want = 0
        if force or st["live"] > self.pool_pages // 2:
            slots, free = self.mv_cap, self.host_pages - st["hlive"]
            for r in range(self.n):
                if not self.pages[r]:
                    continue
                tail = max(self.pages[r])
                for pn in sorted(self.pages[r]):
                    if pn == tail or (pn + 1) * PAGE - 1 > self.commit[r]:
                        break
                    if self.pages[r][pn]:
                        continue
                    if slots == 0:
                        break
                    slots -= 1
                    if free == 0:
                        break
                    free -= 1
                    self.pages[r][pn] = True
                    want += 1
        assert moved == want
        self.par ^= 1
        return moved

    def release(self, r, upto):
        lib().ct_release(self.h, r, upto, self.par)
        gone = [pn for pn in self.pages[r] if upto == ALL or (pn + 1) * PAGE - 1 <= upto]
        # (cold_release frees from the head while pages lie wholly at or below upto)
        for pn in gone:
            del self.pages[r][pn]
        self.ents[r] = {i: v for i, v in self.ents[r].items() if i // PAGE in self.pages[r]}

    # -- the checks after every operation
    def check(self):
        out = (C.c_uint64 * 3)()
        for r in range(self.n):
            for idx, (stamp, value) in self.ents[r].items():
                assert lib().ct_get(self.h, r, idx, out), (r, idx)
                assert (out[0], out[1], out[2]) == (stamp, value, value ^ ALL), (r, idx)
            ch = self.chain(r)
            assert [pn for _, pn in ch] == sorted(self.pages[r]), r
            first = self.stats()["hpool_first"]
            for i, (page, pn) in enumerate(ch):
                on_host = bool(first) and page >= first
                assert on_host == self.pages[r][pn], (r, pn)
                if on_host:
                    assert i + 1 < len(ch), f"replica {r}: the tail page is on the host"
                    assert (pn + 1) * PAGE - 1 <= self.commit[r], \
                        f"replica {r}: uncommitted page {pn} is on the host"
        st = self.stats()
        assert st["live"] == self.model_live()
        assert st["hlive"] == self.model_host()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_random_operations(seed):
    """Appends, rewrites from an index on (into demoted pages too), demotion
    passes at rising commit indexes (above and below the half-pool mark),
    compaction to a marker and whole releases, in a seeded random order: after
    each one every entry reads back, both tiers' counts equal the model's, and
    only committed pages below a tail are on the host."""
    rng = random.Random(seed)
    t = Tiers(pool_pages=40, host_pages=80, n_rep=3, mv_cap=12)
    rewrote_host = 0
    for _ in range(700):
        r = rng.randrange(t.n)
        k = rng.randrange(100)
        if k < 55:
            for _ in range(rng.randrange(1, 50)):
                if not t.append(r, rng.getrandbits(40)):
                    break
        elif k < 70 and t.ents[r]:
            c = rng.choice(sorted(t.ents[r]))
            for i in range(c, min(c + rng.randrange(1, 40), t.last[r] + 1)):
                if i not in t.ents[r]:
                    break
                rewrote_host += t.pages[r][i // PAGE]
                assert t.put(r, i, rng.getrandbits(40))
        elif k < 88:
            for q in range(t.n):
                t.commit[q] += rng.randrange(t.last[q] - t.commit[q] + 1)
            t.demote(force=rng.random() < 0.5)
        elif k < 96:
            t.release(r, rng.randrange(t.last[r] + 1))
        else:
            t.release(r, ALL)
        t.check()
    st = t.stats()
    assert st["demoted"] > 0 and st["passes"] > 0 and rewrote_host > 0
    for r in range(t.n):
        t.release(r, ALL)
    t.check()
    st = t.stats()
    assert st["live"] == 0 and st["hlive"] == 0
    t.close()


def test_freed_pages_are_reused():
    """After a whole release both tiers are empty, and the same load again and
    again lives on the freed pages of both: 31 HBM pages serve three loads of
    20, the bump counter never leaves the end of the pool, and the host bump
    counter does not move after the first load."""
    t = Tiers(pool_pages=32, host_pages=32, n_rep=2, mv_cap=64)

    def load():
        for r in range(t.n):
            for _ in range(10 * PAGE if t.last[r] else 10 * PAGE - 1):  # (ten pages: index 0 is unused)
                assert t.append(r, t.last[r] * 7 + r)
            t.commit[r] = t.last[r]
        assert t.demote() == 2 * 9  # (live 20 > 16: every page but the two tails)
        t.check()

    load()
    st0 = t.stats()
    assert (st0["live"], st0["hlive"], st0["bump"]) == (2, 18, 21)
    for cycle in range(2):
        for r in range(t.n):
            t.release(r, ALL)
        t.check()
        st = t.stats()
        assert st["live"] == 0 and st["hlive"] == 0
        # the 18 HBM pages each demotion freed are in the free-id ring, which
        # the bump counter runs on into once the pool's own pages are spent;
        # the 18 host pages came back to the host tier's stack
        load()
        st1 = t.stats()
        assert (st1["live"], st1["hlive"], st1["oom"]) == (2, 18, 0)
        assert st1["bump"] <= 32 and st1["hbump"] == st0["hbump"]
    assert st1["bump"] == 32  # (spent: every page since came out of the ring or a stack)
    t.close()


def test_full_host_tier_stops_the_plan():
    """A full host tier: the plan stops with every chain whole, the pages it
    could not move stay in HBM, and a later pass moves them once host pages
    come back."""
    t = Tiers(pool_pages=32, host_pages=4, n_rep=2, mv_cap=64)
    for r in range(t.n):
        for _ in range(6 * PAGE - 1):  # (six pages each)
            assert t.append(r, r + 1)
        t.commit[r] = t.last[r]
    assert t.demote(force=True) == 4  # replica 0's first four pages
    t.check()
    assert t.stats()["hlive"] == 4 and t.stats()["live"] == 8
    assert t.demote(force=True) == 0  # full: nothing moves, nothing breaks
    t.check()
    t.release(0, 3 * PAGE - 1)  # compaction gives three host pages back
    t.check()
    assert t.stats()["hlive"] == 1
    assert t.demote(force=True) == 3
    t.check()
    assert t.stats()["hlive"] == 4
    t.close()


def test_full_move_list_stops_the_plan():
    """A full move list: the plan stops with the chain whole and the rest
    waits for the next pass."""
    t = Tiers(pool_pages=32, host_pages=32, n_rep=2, mv_cap=3)
    for r in range(t.n):
        for _ in range(5 * PAGE - 1):  # (five pages each)
            assert t.append(r, r + 1)
        t.commit[r] = t.last[r]
    moved = []
    for _ in range(4):
        moved.append(t.demote(force=True))
        t.check()
    assert moved == [3, 3, 2, 0]
    assert t.stats()["live"] == 2 and t.stats()["hlive"] == 8
    assert t.stats()["passes"] == 3 and t.stats()["demoted"] == 8
    t.close()


@pytest.mark.parametrize("n_rep, pool_pages", [(48, 128), (80, 256)])
def test_logs_in_step_live_on_the_free_id_ring(n_rep, pool_pages):
    """Every replica evicts one entry per round, all logs the same length (the
    C2 shape): once the bump counter is spent the pool lives on what demotion
    frees.  A page freed after a round of one parity must serve the very next
    round, whatever its parity, which a per-parity free stack does not: the
    copy gives the page ids to a ring that the spent bump counter runs on
    into (pool_alloc, pool_fa_settle)."""
    t = Tiers(pool_pages=pool_pages, host_pages=16 * n_rep, n_rep=n_rep, mv_cap=pool_pages)
    peak, spent_at = 0, None
    for rnd in range(1, 620):
        for r in range(n_rep):
            assert lib().ct_put(t.h, r, rnd, 1, rnd, t.par), f"round {rnd}: the pool ran out"
            t.commit[r] = max(0, rnd - 2)
        peak = max(peak, t.stats()["live"])
        lib().ct_demote(t.h, (C.c_uint64 * n_rep)(*t.commit), t.par, 0)
        t.par ^= 1
        bump = t.stats()["bump"]
        if spent_at is None and bump == pool_pages:
            spent_at = rnd
        if spent_at is not None:  # it stays at the end of the pool between rounds
            assert bump == pool_pages, rnd
    st = t.stats()
    assert st["oom"] == 0 and peak <= 2 * n_rep
    assert st["live"] + st["hlive"] == n_rep * (619 // PAGE + 1)
    # the pool's own pages were spent early: the later ~7 pages per replica all
    # came out of the ring
    assert spent_at is not None and spent_at <= 3 * PAGE
    t.close()


def test_no_tier_no_demotion():
    """host_pages = 0: no page id is a host page and a pass moves nothing."""
    t = Tiers(pool_pages=16, host_pages=0, n_rep=1, mv_cap=8)
    for _ in range(5 * PAGE - 1):
        assert t.append(0, 9)
    t.commit[0] = t.last[0]
    assert t.demote(force=True) == 0
    t.check()
    assert t.stats()["live"] == 5 and t.stats()["hlive"] == 0
    t.close()


# ------------------------------------------------------------------ the engine without the tier
C2_SMALL = dict(C2, n_groups=16)


@pytest.mark.parametrize("name, kw, pool_bytes, by_round", [
    ("c2", C2_SMALL, 256 << 10, 180),
    ("long_iso", dict(LONG_ISO, check_quorum=False), 512 << 10, 225),
])
def test_small_pool_runs_out_without_the_tier(name, kw, pool_bytes, by_round):
    """The shapes of test_gpu_cold_tier.py are not vacuous: with
    host_pool_bytes = 0 their small pools are exhausted (measured on the host
    build: by rounds 180 and 225)."""
    eng = SoaCpu(trace=True, ring=8, pool_bytes=pool_bytes, host_pool_bytes=0, **kw)
    eng.run(by_round)
    assert eng.spill_stats()["oom"] & 1, "the page pool never ran out"


@pytest.mark.parametrize("name, kw", [
    ("c2", C2_SMALL),
    ("long_iso_cq", dict(LONG_ISO, check_quorum=True)),
    ("long_iso", dict(LONG_ISO, check_quorum=False)),
])
def test_ring8_default_pool_bit_exact(name, kw):
    """ring = 8 with the default pool stays bit-exact with the oracle for the
    620 rounds the GPU tests run."""
    eng, ref = SoaCpu(trace=True, ring=8, **kw), O.Harness(trace=True, **kw)
    d = run_lockstep(eng, ref, 620, every=1)
    assert d is None, f"first divergence {d}"
    n, bits = eng.faults()
    assert n == 0, f"faults {bits:#x}"
    assert not counters_match(eng.counters(), ref.counters())
    assert eng.spill_stats()["oom"] == 0
