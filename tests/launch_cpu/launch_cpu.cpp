// TEST-ONLY host build of the paged rbe_launch: the host build of the step
// (tests/soa_cpu/soa_cpu.cpp, included unchanged) plus the passes of
// dragonboat_amd/csrc/rbe_launch_kernels.h as plain loops over the same RBE_HD
// functions (dragonboat_amd/csrc/rbe_launch.h), run on the planes of a
// SoaEngine.  lc_create can give the engine a host tier (cfg.host_pool_bytes):
// calloc'd pages the host build's steps read through the same pool_ent; no
// demotion runs here.  tests/launch_cpu/launch.py loads it; with
// -DLAUNCH_CPU_MAIN a stand-alone program that launches boundary shapes both
// ways (for a sanitizer build).  Never linked into the product.
#include "../soa_cpu/soa_cpu.cpp"

#include "../../dragonboat_amd/csrc/rbe_launch.h"

extern "C" {

// soa_create, and with cfg.host_pool_bytes the tier's constants as rbe_create
// sets them: pmeta over both page ranges, the free-id ring, hpool
void* lc_create(const rbe_config* cfg) {
  SoaEngine* e = (SoaEngine*)soa_create(cfg);
  if (!e || !e->C.host_pages) return e;
  const Params& C = e->C;
  SpillCtl* s = e->P.sctl;
  u64 ring = 64;
  while (ring < C.pool_pages) ring <<= 1;
  e->P.pmeta = calloc_t<PoolMeta>(e, (u64)C.pool_pages + C.host_pages);  // (none in use yet)
  s->hpool = calloc_t<Ent>(e, (u64)C.host_pages * kPageEnts);
  s->fa = calloc_t<u32>(e, ring);
  s->hpool_first = C.pool_pages;
  s->hpool_pages = C.host_pages;
  s->fa_mask = (u32)(ring - 1);
  return e;
}

// rbe_launch as rbe_engine.hip runs it: the parent's sequence when no launched
// replica has an entry below its ring, else release / alloc / fill / relaunch
int lc_launch(void* h, uint64_t n, const uint64_t* replica, const rbe_launch_state* st_ids,
              const rbe_entry* ents, const uint8_t* cmd) {
  SoaEngine* e = (SoaEngine*)h;
  std::vector<rbe_launch_state> stv;  // votes as internal ids
  if (!e->hin.map_votes(n, replica, st_ids, stv)) return RBE_E_INVALID;
  const rbe_launch_state* st = stv.data();
  if (n && replica) {
    std::vector<u64> v(replica, replica + n);
    std::sort(v.begin(), v.end());
    if (std::adjacent_find(v.begin(), v.end()) != v.end()) return RBE_E_INVALID;
  }
  std::vector<u64> terms;
  std::vector<Body> bodies;
  int rc = launch_rows(e->C, e->hin.heap, n, replica, st, ents, cmd, terms, bodies);
  if (rc || n == 0) return rc;
  std::vector<LaunchPg> pg;
  std::vector<u32> page_off;
  const u64 np = launch_plan(e->C, n, st, bodies.data(), pg, page_off);
  if (np > 0xFFFFFFF0ull) return RBE_E_NOMEM;
  const Planes& P = e->P;
  const Params& C = e->C;
  const u32 ppar = (e->round & 1u) ^ 1u, par = ppar ^ 1u;
  std::vector<u32> ids(np);
  if (np) {
    for (u64 i = 0; i < n; i++) spill_replica_release(P, C, replica[i], par);  // k_launch_release
    for (u64 p = 0; p < np; p++) {                                             // k_launch_alloc
      const u64 i = launch_page_owner(page_off.data(), n, (u32)p);
      ids[p] = launch_page_alloc(P, C, (u32)p + 1u == page_off[i + 1]);
    }
    for (u64 p = 0; p < np; p++) {  // k_launch_fill
      const u64 i = launch_page_owner(page_off.data(), n, (u32)p);
      const LaunchPg& x = pg[i];
      const u32 j = (u32)p - page_off[i];
      const u32* rid = ids.data() + page_off[i];
      if (!launch_ids_ok(rid, x.pages)) continue;
      for (u32 l = 0; l < kPageEnts; l++)
        *pool_ent(P, rid[j], l) = launch_slot(x, terms.data(), bodies.data(), x.first / kPageEnts + j, l);
      P.pmeta[rid[j]] = launch_meta(x, rid, j);
    }
  }
  u64 off = 0;
  for (u64 i = 0; i < n; i++) {  // k_relaunch
    const rbe_launch_state& x = st[i];
    const u32 nr = np && x.n_entries > C.ring ? C.ring : x.n_entries;
    const u64* t = terms.data() + off + (x.n_entries - nr);
    const Body* b = bodies.data() + off + (x.n_entries - nr);
    with_n(C.n, [&](auto NN) {
      relaunch_replica<decltype(NN)::value>(P, C, replica[i], x.term, x.vote, x.commit,
                                            x.last_index, nr, t, b, ppar, e->tclk, x.marker,
                                            x.marker_term, x.snapshot_index, x.snapshot_term,
                                            x.removed);
    });
    if (np) launch_install(P, replica[i], pg[i], ids.data() + page_off[i], par);
    P.gwake[replica[i] / C.n] = GW_AWAKE;
    off += x.n_entries;
  }
  e->scan_at = e->round;  // as rbe_launch: the next round scans every group
  return RBE_OK;
}

// rbe_cold_tier_stats' first two words: host pages in use / in total
void lc_tier_stats(void* h, uint64_t* out) {
  SoaEngine* e = (SoaEngine*)h;
  out[0] = e->P.sctl->hlive;
  out[1] = e->P.sctl->hpool_pages;
}

// Replica r's cold chain from the head: page ids and page numbers, at most
// cap; returns its length, ~0 on a broken link
uint32_t lc_chain(void* h, uint64_t r, uint32_t* pages, uint64_t* pns, uint32_t cap) {
  SoaEngine* e = (SoaEngine*)h;
  const ColdRef cr = e->P.cold[r];
  u32 n = 0, prev = 0;
  for (u32 p = cr.head; p; p = e->P.pmeta[p].next) {
    if (e->P.pmeta[p].prev != prev) return ~0u;
    if (n < cap) {
      pages[n] = p;
      pns[n] = e->P.pmeta[p].pn;
    }
    n++;
    prev = p;
  }
  if (prev != cr.tail || (n && e->P.pmeta[prev].pn != cr.tail_pn)) return ~0u;
  return n;
}

// Core::mflags of replica r (MB_ROLES | MB_CC_IN_LOG)
uint32_t lc_mflags(void* h, uint64_t r) { return ((SoaEngine*)h)->P.core[r].mflags; }

}  // extern "C"

#ifdef LAUNCH_CPU_MAIN
// Boundary shapes of the cold range launched through lc_launch and through
// the serial soa_launch, in one batch and one per batch: equal entries over
// the whole handed range and equal page counts; then a tiered engine too
// small for the batch, where exhaustion must leave nothing behind.
#include <cstdio>
namespace {
struct Shape {
  u64 last;
  u32 n;
};
rbe_config base_cfg() {
  rbe_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = RBE_ABI_VERSION;
  cfg.n_groups = 4;
  cfg.n_replicas = 3;
  cfg.election_rtt = 10;
  cfg.heartbeat_rtt = 1;
  cfg.ring = 8;
  cfg.seed = 0x1A0C4;
  return cfg;
}
void make_batch(const std::vector<u64>& reps, const std::vector<Shape>& sh,
                std::vector<rbe_launch_state>& st, std::vector<rbe_entry>& ents) {
  st.clear();
  ents.clear();
  for (size_t i = 0; i < reps.size(); i++) {
    rbe_launch_state s;
    memset(&s, 0, sizeof(s));
    s.term = 3;
    s.commit = sh[i].last;
    s.last_index = sh[i].last;
    s.n_entries = sh[i].n;
    st.push_back(s);
    for (u64 idx = sh[i].last - sh[i].n + 1; idx <= sh[i].last; idx++) {
      rbe_entry en;
      memset(&en, 0, sizeof(en));
      en.index = idx;
      en.term = 1 + (idx > 50) + (idx > 120);
      en.cmd_len = 8;
      const u64 v = idx * 1000003ull + reps[i];
      memcpy(en.cmd, &v, 8);
      ents.push_back(en);
    }
  }
}
int same_logs(void* a, void* b, const std::vector<u64>& reps, const std::vector<Shape>& sh) {
  for (size_t i = 0; i < reps.size(); i++) {
    const u64 lo = sh[i].last - sh[i].n + 1;
    std::vector<rbe_entry> x(sh[i].n), y(sh[i].n);
    if (soa_get_entries(a, reps[i], lo, sh[i].last, x.data())) return 1;
    if (soa_get_entries(b, reps[i], lo, sh[i].last, y.data())) return 2;
    if (memcmp(x.data(), y.data(), sizeof(rbe_entry) * sh[i].n)) return 3;
    for (u32 q = 0; q < sh[i].n; q++)
      if (x[q].index != lo + q || x[q].term != 1u + (lo + q > 50) + (lo + q > 120)) return 4;
  }
  return 0;
}
}  // namespace

int main() {
  // n == ring, ring + 1, last cold = 0 / 63 (mod 64), first cold = 63 / 0
  // (mod 64), a page filled at neither end, three pages
  const std::vector<Shape> sh = {{8, 8},     {9, 9},     {72, 72},    {135, 100}, {200, 138},
                                 {200, 137}, {120, 50},  {190, 190},  {8, 8}};
  std::vector<u64> reps = {11, 3, 7, 0, 9, 5, 2, 10, 4};  // (not in ascending order)
  const rbe_config cfg = base_cfg();
  std::vector<rbe_launch_state> st;
  std::vector<rbe_entry> ents;
  u64 checked = 0;
  for (int one = 0; one < 2; one++) {
    void* a = lc_create(&cfg);
    void* b = lc_create(&cfg);
    if (!a || !b) return 2;
    soa_run(a, 3);
    soa_run(b, 3);
    if (!one) {
      make_batch(reps, sh, st, ents);
      if (lc_launch(a, reps.size(), reps.data(), st.data(), ents.data(), nullptr)) return 3;
      if (soa_launch(b, reps.size(), reps.data(), st.data(), ents.data(), nullptr)) return 4;
    } else {
      for (size_t i = 0; i < reps.size(); i++) {
        make_batch({reps[i]}, {sh[i]}, st, ents);
        if (lc_launch(a, 1, &reps[i], st.data(), ents.data(), nullptr)) return 5;
        if (soa_launch(b, 1, &reps[i], st.data(), ents.data(), nullptr)) return 6;
      }
    }
    const int d = same_logs(a, b, reps, sh);
    if (d) return 10 + d;
    u64 sa[5], sb[5];
    soa_spill_stats(a, sa);
    soa_spill_stats(b, sb);
    if (sa[0] != sb[0] || sa[4] || sb[4]) return 20;
    // a second launch of the same batch reuses what the first one's release returns
    make_batch(reps, sh, st, ents);
    if (lc_launch(a, reps.size(), reps.data(), st.data(), ents.data(), nullptr)) return 21;
    soa_spill_stats(a, sb);
    if (sa[0] != sb[0] || same_logs(a, b, reps, sh)) return 22;
    soa_run(a, 5);
    checked += ents.size();
    soa_destroy(a);
    soa_destroy(b);
  }
  // a 7-page pool over a 6-page tier: 12 replicas of 3 pages each do not fit
  rbe_config small = base_cfg();
  small.pool_bytes = 8 * 2048;
  small.host_pool_bytes = 6 * 2048;
  void* t = lc_create(&small);
  if (!t) return 30;
  std::vector<Shape> s3(12, Shape{200, 136});
  std::vector<u64> all(12);
  for (u64 r = 0; r < 12; r++) all[r] = r;
  make_batch(all, s3, st, ents);
  if (lc_launch(t, 12, all.data(), st.data(), ents.data(), nullptr)) return 31;
  u64 nf = 0, pages = 0;
  for (u64 r = 0; r < 12; r++) {
    u32 pgs[8];
    u64 pns[8];
    const u32 len = lc_chain(t, r, pgs, pns, 8);
    if (len == ~0u) return 32;
    std::vector<rbe_entry> x(136);
    const int rc = soa_get_entries(t, r, 65, 200, x.data());
    if (len == 0) {
      nf++;
      if (!rc) return 33;  // (the cold part is gone)
    } else {
      if (len != 3 || rc) return 34;
      pages += len;
    }
  }
  u64 ss[5], ts[2];
  soa_spill_stats(t, ss);
  lc_tier_stats(t, ts);
  if (!nf || nf == 12 || ss[0] + ts[0] != pages || !(ss[4] & 1)) return 35;
  soa_destroy(t);
  printf("launch_cpu ok: %llu entries launched both ways, %llu of 12 replicas refused by a "
         "13-page engine, %llu pages held by the others\n",
         (unsigned long long)checked, (unsigned long long)nf, (unsigned long long)pages);
  return 0;
}
#endif
