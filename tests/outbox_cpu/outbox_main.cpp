// TEST-ONLY stand-alone program over the host build of rbe_collect_outbox
// (outbox_cpu.cpp), for a build with -fsanitize=address,undefined
// (tests/test_outbox_collect.py builds and runs it; nothing is loaded into
// Python under a sanitizer).
//
// The MIXED-shaped workload (5 replicas, CheckQuorum, Quiesce, reads and
// proposals, isolations) with every capacity minimal (maxm = ecap = 1, ring
// 8): message lists and catch-up entries live in the round spill heap, where
// index math over spilled blocks has gone wrong before (DESIGN.md §10,
// "Inbound spill").  The passes run over whole 256-lane blocks — 60 replicas
// in a block of 256, so most lanes lie past the range — with an entries grid
// three blocks larger than the totals need.  Every round the lists of the
// whole engine and of an inner range are compared with outbox_messages
// (soa_get_outbox), message for message, entry for entry, Cmd byte for byte.
#include "outbox_cpu.cpp"

#include <cstdio>

namespace {

struct Want {
  std::vector<rbe_message> m;
  std::vector<rbe_entry> e;
  std::vector<u8> c;
};

int one_sender(void* h, u64 r, Want& w) {
  uint32_t nm = 0, ne = 0;
  uint64_t nc = 0;
  if (soa_get_outbox(h, r, nullptr, 0, &nm, nullptr, 0, &ne, nullptr, 0, &nc)) return 1;
  w.m.assign(nm + 1, rbe_message{});
  w.e.assign(ne + 1, rbe_entry{});
  uint64_t bytes = 0;
  for (int pass = 0; pass < 2; pass++) {  // the first sizes the Cmd buffer
    w.c.assign(bytes + 1, 0);
    if (soa_get_outbox(h, r, w.m.data(), nm, &nm, w.e.data(), ne, &ne, w.c.data(), bytes, &nc))
      return 1;
    bytes = nc;
  }
  w.m.resize(nm);
  w.e.resize(ne);
  w.c.resize(bytes);
  return 0;
}

// the list of [first, first + count) against the per-sender calls
int compare(void* h, u64 first, u64 count, bool cmds, u64* msgs, u64* ents, u64* longest_list,
            u64* longest_ents) {
  rbe_outbox_list l;
  if (soa_collect_outbox(h, first, count, cmds ? 0 : RBE_ENTRIES_NO_CMDS, -1, &l)) return 10;
  u64 i = 0, mj = 0, ej = 0;
  for (u64 r = first; r < first + count; r++) {
    Want w;
    if (one_sender(h, r, w)) return 11;
    if (w.m.empty()) continue;
    if (i >= l.n || l.replica[i] != r || l.msg_off[i] != mj) return 12;
    u64 ei = 0, co = 0, run = 0, to = 0;
    for (const rbe_message& m : w.m) {
      if (mj >= l.n_messages || l.ent_off[mj] != ej) return 13;
      if (memcmp(&m, &l.messages[mj], sizeof(m))) return 14;
      if (m.type != 21) {  // (the Quiesce notice is not in the list)
        run = m.to == to ? run + 1 : 1;
        to = m.to;
      }
      if (run > *longest_list) *longest_list = run;
      if (m.n_entries > *longest_ents) *longest_ents = m.n_entries;
      for (u32 k = 0; k < m.n_entries; k++, ei++, ej++) {
        if (ej >= l.n_entries || ei >= w.e.size()) return 15;
        if (memcmp(&w.e[ei], &l.entries[ej], sizeof(rbe_entry))) return 16;
        const u64 len = w.e[ei].cmd_len;
        if (cmds) {
          if (l.cmd_off[ej] % 16 || l.cmd_off[ej + 1] - l.cmd_off[ej] != ((len + 15) & ~15ull))
            return 17;
          if (len && memcmp(w.c.data() + co, l.cmds + l.cmd_off[ej], len)) return 18;
          for (u64 p = l.cmd_off[ej] + len; p < l.cmd_off[ej + 1]; p++)
            if (l.cmds[p]) return 19;
        }
        co += len;
      }
      mj++;
    }
    if (ei != w.e.size()) return 20;
    i++;
  }
  if (i != l.n || mj != l.n_messages || ej != l.n_entries || l.msg_off[l.n] != mj ||
      l.ent_off[mj] != ej)
    return 21;
  if (cmds ? l.cmd_off[ej] != l.cmd_bytes : (l.cmd_off || l.cmds)) return 22;
  *msgs += mj;
  *ents += ej;
  return 0;
}

}  // namespace

int main() {
  rbe_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = RBE_ABI_VERSION;
  cfg.n_groups = 12;
  cfg.n_replicas = 5;
  cfg.election_rtt = 10;
  cfg.heartbeat_rtt = 1;
  cfg.check_quorum = 1;
  cfg.quiesce = 1;
  cfg.trace = 1;
  cfg.cid_base = 1;
  cfg.cid_stride = 1;
  cfg.seed = 12345;
  cfg.wl_enabled = 1;
  cfg.wl_start_round = 25;
  cfg.wl_active_mod = 2;
  cfg.wl_read_permille = 500;
  cfg.iso_period = 37;
  cfg.iso_len = 20;
  cfg.iso_mod = 2;
  cfg.xfer_mod = 1;
  cfg.cc_mod = 1;
  cfg.maxm = cfg.ecap = cfg.rtr_cap = cfg.dri_cap = cfg.rq_cap = 1;
  cfg.ring = 8;
  void* h = soa_create(&cfg);
  if (!h) return 2;
  const u64 R = 60;
  soa_outbox_extra_blocks(3);
  u64 msgs = 0, ents = 0, longest_list = 0, longest_ents = 0;
  for (int round = 0; round < 120; round++) {
    soa_run(h, 1);
    for (int cmds = 0; cmds < 2; cmds++) {
      int rc = compare(h, 0, R, cmds != 0, &msgs, &ents, &longest_list, &longest_ents);
      if (!rc) rc = compare(h, 6, R - 12, cmds != 0, &msgs, &ents, &longest_list, &longest_ents);
      if (rc) {
        printf("outbox_main: round %d cmds %d: mismatch %d\n", round, cmds, rc);
        return rc;
      }
    }
  }
  uint64_t st[5];
  soa_spill_stats(h, st);
  uint64_t nf = 0;
  const uint32_t bits = soa_faults(h, &nf);
  soa_destroy(h);
  printf("outbox_main ok: %llu messages, %llu entries over 120 rounds, longest list %llu, "
         "most entries in a message %llu, spill peak %llu B, faults %llu (%#x)\n",
         (unsigned long long)msgs, (unsigned long long)ents, (unsigned long long)longest_list,
         (unsigned long long)longest_ents, (unsigned long long)st[2], (unsigned long long)nf, bits);
  // a run that never spills proves nothing
  return longest_list > 1 && longest_ents > 1 && st[2] > 0 && st[4] == 0 && nf == 0 ? 0 : 30;
}
