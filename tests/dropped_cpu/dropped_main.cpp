// TEST-ONLY stand-alone program over the host build of rbe_collect_dropped
// (dropped_cpu.cpp), for a build with -fsanitize=address,undefined
// (__graft_entry__.build() builds it, tests/test_dropped_collect.py runs it as
// a child process; nothing is loaded into Python under a sanitizer).
//
// 16 groups of 3 with host-pushed proposal batches and ReadIndexes at every
// replica, leader transfers and isolations, and every capacity minimal (maxm =
// ecap = dri_cap = 1), so forwarded entries and the contexts of a double
// append live in the round spill heap next to the dropped-entry lists.  The
// passes run over whole 256-lane blocks — 48 replicas in a block of 256 — with
// entry and context grids three blocks larger than the totals need.  Every
// round the lists of the whole engine and of an inner range are compared with
// soa_get_dropped, entry for entry, Cmd byte for byte, context for context,
// and the passes every call made must follow from its three totals alone.
#include "dropped_cpu.cpp"

#include <cstdio>

namespace {

u64 g_rng = 0x9E3779B97F4A7C15ull;
u64 rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

struct Want {
  std::vector<rbe_entry> e;
  std::vector<u8> c;
  std::vector<rbe_system_ctx> x;
};

int one_replica(void* h, u64 r, Want& w) {
  uint32_t ne = 0, nx = 0;
  uint64_t nc = 0;
  if (soa_get_dropped(h, r, nullptr, 0, &ne, nullptr, 0, &nc, nullptr, 0, &nx)) return 1;
  w.e.assign(ne + 1, rbe_entry{});
  w.x.assign(nx + 1, rbe_system_ctx{});
  uint64_t bytes = 0;
  for (int pass = 0; pass < 2; pass++) {  // the first sizes the Cmd buffer
    w.c.assign(bytes + 1, 0);
    if (soa_get_dropped(h, r, w.e.data(), ne, &ne, w.c.data(), bytes, &nc, w.x.data(), nx, &nx))
      return 1;
    bytes = nc;
  }
  w.e.resize(ne);
  w.x.resize(nx);
  w.c.resize(bytes);
  return 0;
}

// the list of [first, first + count) against the per-replica calls
int compare(void* h, u64 first, u64 count, bool cmds, u64* ents, u64* ctxs, u64* longest) {
  rbe_dropped_list l;
  if (soa_collect_dropped(h, first, count, cmds ? 0 : RBE_ENTRIES_NO_CMDS, &l)) return 10;
  // the passes follow the totals alone, never the lists' lengths: 3, one more
  // each for entries, contexts and Cmd bytes when there are any, 3 for the Cmd
  // offsets; at most 9 (5 without Cmds)
  const uint32_t want = 3u + (l.n_entries ? 1u : 0u) + (l.n_read_indexes ? 1u : 0u) +
                        (cmds ? 3u + (l.cmd_bytes ? 1u : 0u) : 0u);
  if (soa_dropped_passes() != want || want > (cmds ? 9u : 5u)) return 9;
  u64 i = 0, ej = 0, xj = 0;
  for (u64 r = first; r < first + count; r++) {
    Want w;
    if (one_replica(h, r, w)) return 11;
    if (w.e.empty() && w.x.empty()) continue;
    if (i >= l.n || l.replica[i] != r || l.ent_off[i] != ej || l.ri_off[i] != xj) return 12;
    if (w.e.size() > *longest) *longest = w.e.size();
    u64 co = 0;
    for (const rbe_entry& e : w.e) {
      if (ej >= l.n_entries || e.index != 0) return 15;
      if (memcmp(&e, &l.entries[ej], sizeof(rbe_entry))) return 16;
      const u64 len = e.cmd_len;
      if (cmds) {
        if (l.cmd_off[ej] % 16 || l.cmd_off[ej + 1] - l.cmd_off[ej] != ((len + 15) & ~15ull))
          return 17;
        if (len && memcmp(w.c.data() + co, l.cmds + l.cmd_off[ej], len)) return 18;
        for (u64 p = l.cmd_off[ej] + len; p < l.cmd_off[ej + 1]; p++)
          if (l.cmds[p]) return 19;
      }
      co += len;
      ej++;
    }
    for (const rbe_system_ctx& x : w.x) {
      if (xj >= l.n_read_indexes || memcmp(&x, &l.read_indexes[xj], sizeof(x))) return 20;
      xj++;
    }
    i++;
  }
  if (i != l.n || ej != l.n_entries || xj != l.n_read_indexes || l.ent_off[l.n] != ej ||
      l.ri_off[l.n] != xj)
    return 21;
  if (cmds ? l.cmd_off[ej] != l.cmd_bytes : (l.cmd_off || l.cmds)) return 22;
  *ents += ej;
  *ctxs += xj;
  return 0;
}

}  // namespace

int run(void* h);
int lapped(void* h);

int main() {
  rbe_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = RBE_ABI_VERSION;
  cfg.n_groups = 16;
  cfg.n_replicas = 3;
  cfg.election_rtt = 10;
  cfg.heartbeat_rtt = 1;
  cfg.trace = 1;
  cfg.cid_base = 1;
  cfg.cid_stride = 1;
  cfg.seed = 12345;
  cfg.ext_inputs = 1;
  cfg.iso_period = 40;
  cfg.iso_len = 20;
  cfg.iso_mod = 1;
  cfg.xfer_mod = 1;
  cfg.cc_mod = 1;
  cfg.maxm = cfg.ecap = cfg.dri_cap = 1;
  cfg.heap_bytes = 1 << 20;
  void* h = soa_create(&cfg);
  if (!h) return 2;
  int rc = run(h);
  soa_destroy(h);
  if (rc) return rc;
  // A lapped record, here by moving the host's head a lap ahead
  // (tests/dropped_scenarios.py lapped_record reaches it with pushes, through
  // a forwarded Propose).  The call that succeeded is then
  // refused whole, with *out zeroed, with and without Cmds.
  cfg.iso_period = 0;
  h = soa_create(&cfg);
  if (!h) return 2;
  rc = lapped(h);
  soa_destroy(h);
  if (!rc) printf("dropped_main ok: a lapped record is refused\n");
  return rc;
}

int lapped(void* h) {
  if (soa_set_drop_lists(h)) return 2;
  const uint64_t r = 0;
  const uint32_t n = 1, type = 0, len = 100;
  const std::vector<u8> cmd(len, 0x5A);
  if (soa_push_proposals(h, 1, &r, &n, &type, &len, cmd.data())) return 3;
  soa_run(h, 1);
  rbe_dropped_list l, zero;
  memset(&zero, 0, sizeof(zero));
  if (soa_collect_dropped(h, 0, 48, 0, &l) || l.n != 1 || l.n_entries != 1 ||
      l.entries[0].cmd_len != len || memcmp(l.cmds, cmd.data(), len))
    return 40;
  HostHeap& hp = ((SoaEngine*)h)->hin.heap;
  hp.head += hp.cap;
  hp.flushed = hp.head;
  hp.stage.clear();
  for (uint32_t flags : {0u, (uint32_t)RBE_ENTRIES_NO_CMDS})
    if (soa_collect_dropped(h, 0, 48, flags, &l) != RBE_E_STATE || memcmp(&l, &zero, sizeof(l)))
      return 41;
  if (soa_collect_dropped(h, 3, 45, 0, &l) || l.n != 0) return 42;  // a range without it is served
  return 0;
}

int run(void* h) {
  if (soa_set_drop_lists(h)) return 2;
  const u64 R = 48;
  soa_dropped_extra_blocks(3);
  u64 ents = 0, ctxs = 0, longest = 0;
  for (int round = 0; round < 120; round++) {
    for (u64 r = 0; r < R; r++) {
      if (rnd() % 3 == 0) {  // a batch of 1-3 proposals, Cmds of 0-99 bytes (the heap past 16)
        uint32_t n = 1 + rnd() % 3, type[3] = {0, 0, 0}, len[3];
        std::vector<u8> cmd;
        for (uint32_t j = 0; j < n; j++) {
          len[j] = rnd() % 5 ? rnd() % 17 : rnd() % 100;
          for (uint32_t b = 0; b < len[j]; b++) cmd.push_back((u8)rnd());
        }
        cmd.push_back(0);
        if (soa_push_proposals(h, 1, &r, &n, type, len, cmd.data())) return 3;
      }
      if (rnd() % 3 == 0) {
        const uint64_t lo = ((u64)(round + 1) << 32) | r, hi = rnd();
        if (soa_push_read_index(h, 1, &r, &lo, &hi)) return 4;
      }
      if (round > 30 && rnd() % 40 == 0) {
        const uint64_t to = 1 + rnd() % 3;
        if (soa_request_leader_transfer(h, 1, &r, &to)) return 5;
      }
    }
    soa_run(h, 1);
    for (int cmds = 0; cmds < 2; cmds++) {
      int rc = compare(h, 0, R, cmds != 0, &ents, &ctxs, &longest);
      if (!rc) rc = compare(h, 5, R - 11, cmds != 0, &ents, &ctxs, &longest);
      if (rc) {
        printf("dropped_main: round %d cmds %d: mismatch %d\n", round, cmds, rc);
        return rc;
      }
    }
  }
  uint64_t st[5];
  soa_spill_stats(h, st);
  uint64_t nf = 0;
  const uint32_t bits = soa_faults(h, &nf);
  printf("dropped_main ok: %llu dropped entries, %llu dropped ReadIndexes over 120 rounds, "
         "longest list %llu, spill peak %llu B, faults %llu (%#x)\n",
         (unsigned long long)ents, (unsigned long long)ctxs, (unsigned long long)longest,
         (unsigned long long)st[2], (unsigned long long)nf, bits);
  // a run that never drops proves nothing
  return ents > 100 && ctxs > 100 && longest > 1 && st[2] > 0 && st[4] == 0 && nf == 0 ? 0 : 30;
}
