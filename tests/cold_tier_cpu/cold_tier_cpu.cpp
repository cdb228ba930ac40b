// TEST-ONLY host build of the cold log and its host tier (dragonboat_amd/csrc/
// rbe_spill.h): the page pool, a replica's chain, and the demotion plan and
// copy that the HIP engine runs after a round (k_cold_demote_plan /
// k_cold_demote_copy call the same RBE_HD functions).  A small C API over
// malloc'd tiers for tests/test_cold_tier.py; with -DCOLD_TIER_MAIN a
// stand-alone program that runs a seeded random sequence against a std::map
// model (for a sanitizer build).  Never linked into the product.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../dragonboat_amd/csrc/rbe_step.h"  // (defines RBE_HD, includes rbe_spill.h)

using namespace rbe;

namespace {

// the tiers' fields the templates of rbe_spill.h read (as SpillP / SpillC)
struct CtP {
  Ent* pool;
  PoolMeta* pmeta;
  SpillCtl* sctl;
};
struct CtC {
  u32 pool_pages, host_pages;
};
struct Ct {
  CtP P;
  CtC C;
  std::vector<ColdRef> cold;
  std::vector<ColdMove> mv;
};

}  // namespace

extern "C" {

// pool_pages HBM pages (page 0 is the null page), host_pages of host tier
// (0 = no tier), n_rep chains, a move list of mv_cap slots
void* ct_create(uint32_t pool_pages, uint32_t host_pages, uint32_t n_rep, uint32_t mv_cap) {
  Ct* t = new Ct();
  t->C.pool_pages = pool_pages;
  t->C.host_pages = host_pages;
  t->P.pool = (Ent*)calloc((size_t)pool_pages * kPageEnts, sizeof(Ent));
  t->P.pmeta = (PoolMeta*)calloc((size_t)pool_pages + host_pages, sizeof(PoolMeta));
  SpillCtl* s = (SpillCtl*)aligned_alloc(alignof(SpillCtl), sizeof(SpillCtl));
  memset(s, 0, sizeof(SpillCtl));
  s->bump = 1;
  t->P.sctl = s;
  if (host_pages) {  // the tier's constants, as rbe_create sets them
    u32 ring = 64;
    while (ring < pool_pages) ring <<= 1;
    s->hpool = (Ent*)calloc((size_t)host_pages * kPageEnts, sizeof(Ent));
    s->fa = (u32*)calloc(ring, sizeof(u32));
    s->hpool_first = pool_pages;
    s->hpool_pages = host_pages;
    s->fa_mask = ring - 1;
  }
  ColdRef z;
  z.head = z.tail = 0;
  z.tail_pn = 0;
  t->cold.assign(n_rep, z);
  ColdMove m0;
  m0.src = m0.dst = 0;
  t->mv.assign(mv_cap, m0);
  return t;
}

void ct_destroy(void* h) {
  Ct* t = (Ct*)h;
  free(t->P.pool);
  free(t->P.pmeta);
  free(t->P.sctl->hpool);
  free(t->P.sctl->fa);
  free(t->P.sctl);
  delete t;
}

// cold_put of entry idx = (term, lo) in a round of parity par; 0 when the pool is full
int ct_put(void* h, uint32_t r, uint64_t idx, uint64_t term, uint64_t lo, uint32_t par) {
  Ct* t = (Ct*)h;
  Ent e;
  memset(&e, 0, sizeof(e));
  e.term = term;
  e.lo = lo;
  e.hi = ~lo;
  e.len = 16;
  return cold_put(t->P, t->C, t->cold[r], idx, e, par) ? 1 : 0;
}

// cold_get: out = {term, lo, hi}; 0 when the chain does not hold the page
int ct_get(void* h, uint32_t r, uint64_t idx, uint64_t* out) {
  Ct* t = (Ct*)h;
  Ent e;
  if (!cold_get(t->P, t->cold[r], idx, &e)) return 0;
  out[0] = e.term;
  out[1] = e.lo;
  out[2] = e.hi;
  return 1;
}

// One demotion pass after a round of parity par, as launch_step queues it:
// the plan for every replica (commit[r] its commit index) unless at most half
// the pool is in use (and `force` is 0), then the copy of the planned moves.
// Returns the pages moved.
uint32_t ct_demote(void* h, const uint64_t* commit, uint32_t par, int force) {
  Ct* t = (Ct*)h;
  SpillCtl* s = t->P.sctl;
  s->mv_n[par ^ 1u] = 0;
  pool_fa_settle(s, t->C.pool_pages);
  u32 moved = 0;
  if (force || s->live > t->C.pool_pages / 2)
    for (size_t r = 0; r < t->cold.size(); r++)
      moved += cold_demote_plan(t->P, t->C, t->cold[r], commit[r], par, t->mv.data(),
                                (u32)t->mv.size());
  const u32 n = cold_move_count(s, par, (u32)t->mv.size());
  for (u32 i = 0; i < n; i++) {
    const ColdMove x = t->mv[i];
    if (!x.dst) continue;
    for (u32 j = 0; j < kPageEnts; j++) cold_demote_ent(t->P, x, j);
    cold_demote_done(t->P, x);
  }
  cold_demote_account(s);
  return moved;
}

// cold_release: pages wholly at or below upto (~0: the whole chain)
void ct_release(void* h, uint32_t r, uint64_t upto, uint32_t par) {
  Ct* t = (Ct*)h;
  cold_release(t->P, t->cold[r], upto, par);
}

// replica r's chain from the head: page ids and page numbers, at most cap;
// returns its length
uint32_t ct_chain(void* h, uint32_t r, uint32_t* pages, uint64_t* pns, uint32_t cap) {
  Ct* t = (Ct*)h;
  u32 n = 0;
  u32 prev = 0;
  for (u32 p = t->cold[r].head; p; p = t->P.pmeta[p].next) {
    if (t->P.pmeta[p].prev != prev) return ~0u;  // (a broken back link)
    if (n < cap) {
      pages[n] = p;
      pns[n] = t->P.pmeta[p].pn;
    }
    n++;
    prev = p;
  }
  if (prev != t->cold[r].tail) return ~0u;
  return n;
}

// live, hlive, bump, hbump, demoted, passes, mv_n[0], mv_n[1], oom, hpool_first
void ct_stats(void* h, uint64_t* out) {
  Ct* t = (Ct*)h;
  const SpillCtl& s = *t->P.sctl;
  out[0] = s.live;
  out[1] = s.hlive;
  out[2] = s.bump;
  out[3] = s.hbump;
  out[4] = s.demoted;
  out[5] = s.passes;
  out[6] = s.mv_n[0];
  out[7] = s.mv_n[1];
  out[8] = s.oom;
  out[9] = s.hpool_first;
}

}  // extern "C"

#if defined(COLD_TIER_MAIN)
// A seeded random run against a model: appends, rewrites below the tail (into
// demoted pages too), demotion passes, partial and whole releases
int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1;
  const int ops = argc > 2 ? atoi(argv[2]) : 20000;
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&](uint64_t n) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x % n;
  };
  const uint32_t R = 3;
  void* h = ct_create(48, 96, R, 16);
  std::map<uint64_t, uint64_t> model[R];
  uint64_t last[R] = {0, 0, 0}, commit[R] = {0, 0, 0};
  uint32_t par = 0;
  auto fail = [&](const char* what, int op) {
    fprintf(stderr, "cold_tier_cpu: %s at op %d (seed %llu)\n", what, op,
            (unsigned long long)seed);
    return 1;
  };
  for (int op = 0; op < ops; op++) {
    const uint32_t r = (uint32_t)rnd(R);
    const uint64_t k = rnd(100);
    if (k < 60) {  // append a few
      for (uint64_t n = 1 + rnd(40); n; n--) {
        const uint64_t v = rnd(1ull << 40);
        if (!ct_put(h, r, last[r] + 1, op + 1, v, par)) break;
        model[r][++last[r]] = v;
      }
    } else if (k < 75 && last[r] > 1) {  // rewrite from c on
      const uint64_t c = 1 + rnd(last[r]);
      if (model[r].count(c)) {
        const uint64_t n = 1 + rnd(30);
        for (uint64_t i = c; i < c + n && i <= last[r]; i++) {
          if (!model[r].count(i)) break;
          const uint64_t v = rnd(1ull << 40);
          if (!ct_put(h, r, i, op + 1, v, par)) return fail("rewrite refused", op);
          model[r][i] = v;
        }
      }
    } else if (k < 90) {  // a demotion pass, then the next round
      for (uint32_t q = 0; q < R; q++) commit[q] += rnd(last[q] - commit[q] + 1);
      ct_demote(h, commit, par, (int)rnd(2));
      par ^= 1u;
    } else if (k < 97) {  // compaction
      const uint64_t upto = rnd(last[r] + 1);
      ct_release(h, r, upto, par);
      for (auto it = model[r].begin(); it != model[r].end();)
        it = (it->first / kPageEnts + 1) * kPageEnts - 1 <= upto ? model[r].erase(it) : ++it;
    } else {  // a restored snapshot: everything goes
      ct_release(h, r, ~0ull, par);
      model[r].clear();
    }
    uint64_t pages = 0;
    for (uint32_t q = 0; q < R; q++) {
      uint64_t pn_last = ~0ull;
      for (const auto& kv : model[q]) {
        uint64_t out[3];
        if (!ct_get(h, q, kv.first, out) || out[1] != kv.second) return fail("read mismatch", op);
        if (kv.first / kPageEnts != pn_last) pages++;
        pn_last = kv.first / kPageEnts;
      }
    }
    uint64_t st[10];
    ct_stats(h, st);
    if (st[0] + st[1] != pages) return fail("page count mismatch", op);
  }
  for (uint32_t q = 0; q < R; q++) ct_release(h, q, ~0ull, par);
  uint64_t st[10];
  ct_stats(h, st);
  if (st[0] || st[1]) return fail("pages left after release", ops);
  printf("cold_tier_cpu ok: %d ops, demoted %llu pages in %llu passes\n", ops,
         (unsigned long long)st[4], (unsigned long long)st[5]);
  ct_destroy(h);
  return 0;
}
#endif
