// TEST-ONLY host build of rbe_collect_entries / rbe_collect_entry_ranges: the
// host build of the step (tests/soa_cpu/soa_cpu.cpp, included unchanged) plus
// the passes of dragonboat_amd/csrc/rbe_collect_kernels.h as plain loops over
// the same RBE_HD functions (dragonboat_amd/csrc/rbe_collect.h), run on the
// planes of a SoaEngine.  tests/collect_cpu/collect.py loads it; with
// -DCOLLECT_CPU_MAIN a stand-alone program that runs a small engine and reads
// its logs back both ways (for a sanitizer build).  Never linked into the
// product.
#include "../soa_cpu/soa_cpu.cpp"

#include "../../dragonboat_amd/csrc/rbe_collect.h"

namespace {

// one set of buffers per source (save, committed, ranges), shared by every
// engine of the process: a list is valid until the next call of its source
struct CeBuf {
  std::vector<u64> rep, ent_off, lo_at, cmd_off, src;
  std::vector<rbe_entry> ents;
  std::vector<u8> cmds;
};
CeBuf g_ce[3];

int collect(SoaEngine* e, const CeSrc& s, bool cmds, u32 slot, rbe_entry_list* out) {
  CeBuf& B = g_ce[slot];
  B = CeBuf();
  // records still staged for the next step go to the heap now, as ce_collect
  // uploads them (run_round writes the same bytes again)
  const HostHeap& hp = e->hin.heap;
  for (u64 p = hp.flushed; hp.cap && p < hp.head; p++) e->heap[p % hp.cap] = hp.stage[p - hp.flushed];
  const u8* heap = e->heap.empty() ? nullptr : e->heap.data();
  u32 err = 0;
  u64 ne = 0;
  for (u64 i = 0; i < s.count; i++) {  // k_ce_count / k_ce_ranges
    u64 r, lo;
    const u64 cnt = collect_range(e->P, e->C, s, i, &r, &lo, &err);
    if (!cnt) continue;
    B.rep.push_back(r);
    B.ent_off.push_back(ne);
    B.lo_at.push_back(lo);
    ne += cnt;
  }
  B.ent_off.push_back(ne);
  if (err) return collect_rc(err);
  const u64 n = B.rep.size();
  B.ents.resize(ne);
  B.src.resize(ne);
  B.cmd_off.assign(ne + 1, 0);
  for (u64 j = 0; j < ne; j++) {  // k_ce_entries, then the Cmd offsets
    const u64 sl = collect_slot_of(B.ent_off.data(), n, j);
    CeEnt x;
    err |= collect_entry(e->P, e->C, heap, hp.head, B.rep[sl], B.lo_at[sl] + (j - B.ent_off[sl]), &x);
    B.ents[j] = x.e;
    B.src[j] = x.src;
    B.cmd_off[j + 1] = B.cmd_off[j] + x.plen;
  }
  if (err) return collect_rc(err);
  if (cmds) {  // k_ce_cmds
    B.cmds.assign(B.cmd_off[ne], 0);
    for (u64 j = 0; j < ne; j++) {
      u32 words = ce_padded(B.ents[j].cmd_len) >> 4;
      if (B.src[j] == kCeInline && words > 1) words = 1;
      for (u32 w = 0; w < words; w++) {
        const CeWord v = collect_cmd_word(heap, B.ents[j], B.src[j], w);
        memcpy(B.cmds.data() + B.cmd_off[j] + 16ull * w, &v, 16);
      }
    }
  }
  out->n = n;
  out->n_entries = ne;
  out->replica = B.rep.data();
  out->ent_off = B.ent_off.data();
  out->entries = B.ents.data();
  if (cmds) {
    out->cmd_bytes = B.cmd_off[ne];
    out->cmd_off = B.cmd_off.data();
    out->cmds = B.cmds.data();
  }
  return RBE_OK;
}

}  // namespace

extern "C" {

int soa_collect_entries(void* h, uint64_t first, uint64_t count, uint32_t flags,
                        rbe_entry_list* out) {
  SoaEngine* e = (SoaEngine*)h;
  const uint32_t which = flags & (RBE_ENTRIES_TO_SAVE | RBE_ENTRIES_COMMITTED);
  if (!e || !out || count == 0 || first >= e->C.n_rep || count > e->C.n_rep - first ||
      (flags & ~(RBE_ENTRIES_TO_SAVE | RBE_ENTRIES_COMMITTED | RBE_ENTRIES_NO_CMDS)) ||
      (which != RBE_ENTRIES_TO_SAVE && which != RBE_ENTRIES_COMMITTED))
    return RBE_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->first = first;
  out->count = count;
  // (before the first step no Upd record is of round - 1: the lists come out empty)
  const CeSrc s{first, count, e->round, which, nullptr, nullptr, nullptr};
  const int rc = collect(e, s, !(flags & RBE_ENTRIES_NO_CMDS),
                         which == RBE_ENTRIES_TO_SAVE ? 0u : 1u, out);
  if (rc) memset(out, 0, sizeof(*out));
  return rc;
}

int soa_collect_entry_ranges(void* h, uint64_t n, const uint64_t* replica, const uint64_t* lo,
                             const uint64_t* hi, uint32_t flags, rbe_entry_list* out) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !out || (flags & ~RBE_ENTRIES_NO_CMDS) || (n && (!replica || !lo || !hi)))
    return RBE_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->count = n;
  const CeSrc s{0, n, e->round, 0, replica, lo, hi};
  const int rc = collect(e, s, !(flags & RBE_ENTRIES_NO_CMDS), 2u, out);
  if (rc) memset(out, 0, sizeof(*out));
  return rc;
}

// rbe_get_updates: the last round's Updates (rbe_host.h update_view), which
// the tests compare the lists' ranges with
int soa_get_updates(void* h, uint64_t first, uint64_t count, rbe_update* out) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !out || first >= e->C.n_rep || count > e->C.n_rep - first) return RBE_E_INVALID;
  for (u64 i = 0; i < count; i++) {
    const u64 r = first + i;
    update_view(e->P.upd[r], e->P.core[r], e->P.hot[r], e->round, out[i]);
  }
  return RBE_OK;
}

}  // extern "C"

#ifdef COLLECT_CPU_MAIN
// A small engine with the built-in workload and a ring of 8, so the logs reach
// into the cold log: every replica's whole log read through
// soa_collect_entry_ranges equals soa_get_entries + soa_get_entry_cmds, and
// each round's EntriesToSave list is consistent with its offsets.
#include <cstdio>
int main() {
  rbe_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = RBE_ABI_VERSION;
  cfg.n_groups = 6;
  cfg.n_replicas = 3;
  cfg.election_rtt = 10;
  cfg.heartbeat_rtt = 1;
  cfg.ring = 8;
  cfg.seed = 0x5EEDD8A6;
  cfg.wl_enabled = 1;
  cfg.wl_start_round = 30;
  void* h = soa_create(&cfg);
  if (!h) return 2;
  const u64 R = 18;
  u64 saved = 0;
  for (int round = 0; round < 150; round++) {
    soa_run(h, 1);
    rbe_entry_list l;
    if (soa_collect_entries(h, 0, R, RBE_ENTRIES_TO_SAVE, &l)) return 3;
    if (l.ent_off[l.n] != l.n_entries || l.cmd_off[l.n_entries] != l.cmd_bytes) return 4;
    saved += l.n_entries;
  }
  std::vector<rbe_replica_view> v(R);
  soa_views(h, v.data());
  std::vector<u64> rep, lo, hi;
  for (u64 r = 0; r < R; r++)
    if (v[r].last_index) {
      rep.push_back(r);
      lo.push_back(1);
      hi.push_back(v[r].last_index);
    }
  rbe_entry_list l;
  if (soa_collect_entry_ranges(h, rep.size(), rep.data(), lo.data(), hi.data(), 0, &l)) return 5;
  u64 checked = 0;
  for (u64 i = 0; i < l.n; i++) {
    const u64 n = hi[i];
    std::vector<rbe_entry> one(n);
    std::vector<u64> off(n + 1);
    std::vector<u8> cmd(16 * n + 16);
    if (soa_get_entries(h, rep[i], 1, n, one.data())) return 6;
    if (soa_get_entry_cmds(h, rep[i], 1, n, cmd.data(), cmd.size(), off.data())) return 7;
    for (u64 j = 0; j < n; j++, checked++) {
      const u64 at = l.ent_off[i] + j;
      if (memcmp(&one[j], &l.entries[at], sizeof(rbe_entry))) return 8;
      if (memcmp(cmd.data() + off[j], l.cmds + l.cmd_off[at], one[j].cmd_len)) return 9;
    }
  }
  soa_destroy(h);
  printf("collect_cpu ok: %llu entries saved over 150 rounds, %llu read back both ways\n",
         (unsigned long long)saved, (unsigned long long)checked);
  return checked && saved ? 0 : 10;
}
#endif
