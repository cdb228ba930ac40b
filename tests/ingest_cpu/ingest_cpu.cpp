// TEST-ONLY host build of the spilling inbound transport: the host build of
// the step (tests/soa_cpu/soa_cpu.cpp, included unchanged) plus
// rbe_wire_ingest / rbe_push_messages with a list past maxm and a message's
// entries past ecap going to the round spill heap
// (dragonboat_amd/csrc/rbe_ingest_spill.h ingest_sender_spill, rbe_xchg.h
// messages_to_records with a reservation).  RBE_HD functions as plain loops, in the passes
// a device pipeline would run; the granules are placed by one rule
// (this engine's share, from SpillCtl::used of the last round's parity, an
// exclusive scan of the runs' needs in sorted order), so the host build leaves
// the bytes a device pass would.  tests/ingest_cpu/ingest.py loads it; with
// -DINGEST_CPU_MAIN a stand-alone program that runs two small engines with
// every message capacity at 1 over frames and over the raftpb-form calls (for
// a sanitizer build).  Never linked into the product.
#include "../soa_cpu/soa_cpu.cpp"

#include "../../dragonboat_amd/csrc/rbe_ingest_spill.h"

namespace {

// the free part of this engine's share of the spill heap of parity `par`
struct Share {
  u64 first, used, avail;
};
Share share_of(const SoaEngine* e, u32 par) {
  const u64 share = spill_share(e->C);
  const u64 used = e->P.sctl->used[par];
  Share s;
  s.first = e->C.rep_world > 1 ? share * e->C.rep_rank : 0;
  s.used = used;
  s.avail = used < share ? share - used : 0;
  return s;
}
// the granules are taken (after every reader of the base)
void share_take(SoaEngine* e, u32 par, u64 total) {
  SpillCtl* s = e->P.sctl;
  s->used[par] += total;
  if (total && s->peak[par] < s->used[par]) s->peak[par] = s->used[par];
}

// soa_ingest_t of soa_cpu.cpp with the spilling checks and walks
template <int N>
int ingest_spill_t(SoaEngine* e, const uint8_t* d, uint64_t bytes, uint64_t* st) {
  const Params& C = e->C;
  u32 table[256];
  for (u32 i = 0; i < 256; i++) table[i] = crc_table_entry(i);
  std::vector<std::pair<u64, u64>> pos;  // message bodies
  for (u64 i = 0; i < bytes;) {
    if (bytes - i < kWireHeader || d[i] != 0xAE || d[i + 1] != 0x7D) return RBE_E_CORRUPT;
    u64 size = 0;
    for (int b = 0; b < 8; b++) size = (size << 8) | d[i + 4 + b];
    if (size == 0 || size > bytes - i - kWireHeader) return RBE_E_CORRUPT;
    u8 hb[18];
    memcpy(hb, d + i + 2, 18);
    const u32 inc = ((u32)hb[10] << 24) | ((u32)hb[11] << 16) | ((u32)hb[12] << 8) | hb[13];
    const u32 pc = ((u32)hb[14] << 24) | ((u32)hb[15] << 16) | ((u32)hb[16] << 8) | hb[17];
    hb[10] = hb[11] = hb[12] = hb[13] = 0;
    const u64 off = i + kWireHeader;
    if (crc32_update(0, hb, 18, table) != inc || (((u32)hb[0] << 8) | hb[1]) != kWireMethod ||
        crc32_update(0, d + off, size, table) != pc)
      return RBE_E_CORRUPT;
    WireRd rd{d + off, size, 0, false};
    while (rd.i < size && !rd.bad) {
      const u64 tag = rd.varint();
      const u32 fn = (u32)(tag >> 3), wt = (u32)(tag & 7);
      if (fn == 1 && wt == 2) {
        const u64 l = rd.varint();
        if (rd.bad || l > size - rd.i) return RBE_E_CORRUPT;
        pos.emplace_back(off + rd.i, l);
        rd.i += l;
      } else {
        rd.skip(wt);
      }
    }
    if (rd.bad) return RBE_E_CORRUPT;
    st[0]++;
    i = off + size;
  }
  const u64 tm = pos.size();
  std::vector<u64> ent0(tm + 1, 0), cmd0(tm + 1, 0);
  for (u64 j = 0; j < tm; j++) {
    WireRd rd{d, pos[j].first + pos[j].second, pos[j].first, false};
    u64 cb = 0;
    const u32 ne = wire_message_get(rd, pos[j].first + pos[j].second, nullptr, nullptr, nullptr, &cb);
    if (rd.bad) return RBE_E_CORRUPT;
    ent0[j + 1] = ent0[j] + ne;
    cmd0[j + 1] = cmd0[j] + cb;
  }
  std::vector<rbe_message> msgs(tm);
  std::vector<rbe_entry> ents(ent0[tm] + 1);
  std::vector<u8> cmd(cmd0[tm] + 1);
  for (u64 j = 0; j < tm; j++) {
    WireRd rd{d, pos[j].first + pos[j].second, pos[j].first, false};
    u64 cb = cmd0[j];
    wire_message_get(rd, pos[j].first + pos[j].second, &msgs[j], ents.data() + ent0[j], cmd.data(),
                     &cb);
  }
  st[1] = tm;
  st[3] = ent0[tm];
  st[4] = cmd0[tm];
  if (!tm) return RBE_OK;
  if (tm > 0x7FFFFFFFull) return RBE_E_NOMEM;
  HostHeap& H = e->hin.heap;
  std::vector<u64> key(tm), hb(tm);
  u32 err = 0;
  for (u64 j = 0; j < tm; j++) {  // lane per message
    u32 x = 0;
    ingest_ids<N>(C, e->hin.id_table(), msgs[j]);
    key[j] = ingest_check<N>(C, H.cap, msgs[j], ents.data() + ent0[j], &x, &hb[j], true);
    err |= x;
    if (!x && key[j] == ing_drop_key(C)) st[2]++;
  }
  if (err & ING_INVALID) return RBE_E_INVALID;
  if (err & ING_NOMEM) return RBE_E_NOMEM;
  std::vector<u32> sidx(tm);
  for (u64 j = 0; j < tm; j++) sidx[j] = (u32)j;
  std::stable_sort(sidx.begin(), sidx.end(), [&](u32 a, u32 b) { return key[a] < key[b]; });
  std::vector<u64> skey(tm), hs(tm), sn(tm, 0);
  u64 need = 0;
  for (u64 p = 0; p < tm; p++) {
    skey[p] = key[sidx[p]];
    hs[p] = need;
    need += hb[sidx[p]];
  }
  const u32 par = (e->round - 1) & 1u;
  // the checking walk: each run's granule need, then their exclusive scan
  for (u64 p = 0; p < tm; p++) {
    if (!ingest_run_start(C, skey.data(), p)) continue;
    const u64 q = ingest_run_end(C, skey.data(), p, tm);
    err |= ingest_sender_spill<N, false>(e->P, C, par, e->round, skey.data(), sidx.data(), p, q,
                                   msgs.data(), ents.data(), ent0.data(), cmd0.data(), cmd.data(),
                                   nullptr, H.cap, 0, hs.data(), &sn[p], 0);
  }
  if (err) return RBE_E_NOMEM;
  u64 stot = 0;
  for (u64 p = 0; p < tm; p++) {
    const u64 x = sn[p];
    sn[p] = stot;
    stot += x;
  }
  const Share sh = share_of(e, par);
  if (stot > sh.avail) return RBE_E_NOMEM;  // nothing written, no exhaustion flag
  st[5] = need;
  u64 base = 0;
  if (need) {
    for (u64 p = H.flushed; p < H.head; p++) e->heap[p % H.cap] = H.stage[p - H.flushed];
    const u64 skip = H.head % H.cap + need > H.cap ? H.cap - H.head % H.cap : 0;
    const int rc = H.room(need + skip);
    if (rc) return rc;
    if (H.flushed < H.round_lo) H.round_lo = H.flushed;
    H.stage.clear();
    base = H.head + skip;
    H.head = base + need;
    H.flushed = H.head;
    e->heap_head = H.head;
  }
  for (u64 p = 0; p < tm; p++) {  // the writing walk
    if (!ingest_run_start(C, skey.data(), p)) continue;
    const u64 q = ingest_run_end(C, skey.data(), p, tm);
    ingest_sender_spill<N, true>(e->P, C, par, e->round, skey.data(), sidx.data(), p, q, msgs.data(),
                           ents.data(), ent0.data(), cmd0.data(), cmd.data(), e->heap.data(), H.cap,
                                 base, hs.data(), nullptr, sh.first + sh.used + sn[p]);
  }
  share_take(e, par, stot);
  return RBE_OK;
}

template <int N>
int push_spill_t(SoaEngine* e, uint64_t n, const uint64_t* group, const rbe_message* msgs,
                 const rbe_entry* ents, const uint8_t* cmd) {
  std::vector<XCnt> c;
  std::vector<XMsg> m;
  std::vector<XEnt> x;
  const u32 par = (e->round - 1) & 1u;
  const Share sh = share_of(e, par);
  XSpillRes sp{sh.first + sh.used, sh.avail, 0};
  const int rc = messages_to_records<N>(e->C, e->hin.heap, e->round, n, group, msgs, ents, cmd, c,
                                        m, x, e->hin.id_table(), &sp);
  if (rc) return rc;
  soa_xchg_unpack_t<N>(e, c.data(), c.size(), m.data(), m.size(), x.data(), x.size());
  share_take(e, par, sp.total);
  return RBE_OK;
}

}  // namespace

extern "C" {

int soa_wire_ingest_spill(void* h, const uint8_t* data, uint64_t bytes, uint64_t* stats6) {
  SoaEngine* e = (SoaEngine*)h;
  memset(stats6, 0, 6 * sizeof(u64));
  if (e->round == 0) return RBE_E_INVALID;
  if (e->C.rep_world <= 1) return RBE_E_STATE;
  return with_n(e->C.n, [&](auto NN) {
    return ingest_spill_t<decltype(NN)::value>(e, data, bytes, stats6);
  });
}

int soa_push_messages_spill(void* h, uint64_t n, const uint64_t* group, const rbe_message* msgs,
                            const rbe_entry* ents, const uint8_t* cmd) {
  SoaEngine* e = (SoaEngine*)h;
  if (e->round == 0) return RBE_E_INVALID;
  if (e->C.rep_world <= 1) return RBE_E_STATE;
  return with_n(e->C.n, [&](auto NN) {
    return push_spill_t<decltype(NN)::value>(e, n, group, msgs, ents, cmd);
  });
}

// granules of the round spill heap of the last round's parity that are taken
// (SpillCtl::used): what an inbound batch adds is what it spilled
uint64_t soa_spill_used(void* h) {
  SoaEngine* e = (SoaEngine*)h;
  return e->round ? e->P.sctl->used[(e->round - 1) & 1u] : 0;
}

// the bytes of the round spill heap of parity `par` (both shares), for the
// tests that compare what push and frames leave there
uint64_t soa_spill_heap(void* h, uint32_t par, uint8_t* out, uint64_t cap) {
  SoaEngine* e = (SoaEngine*)h;
  const u64 n = e->C.spill_units * 16;
  if (out) memcpy(out, e->P.spill[par & 1u], n < cap ? n : cap);
  return n;
}

}  // extern "C"

#ifdef INGEST_CPU_MAIN
// Two engines (rep_world = 2) of 4 x 3 with the isolation schedule and every
// message capacity at 1, first over frames, then over the raftpb-form calls:
// every hop spills lists and entries inbound.  For a sanitizer build.
#include <cstdio>
static int run_pair(bool wire) {
  void* h[2];
  for (u32 r = 0; r < 2; r++) {
    rbe_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = RBE_ABI_VERSION;
    cfg.n_groups = 4;
    cfg.n_replicas = 3;
    cfg.election_rtt = 10;
    cfg.heartbeat_rtt = 1;
    cfg.seed = 0x5EEDD8A6;
    cfg.wl_enabled = 1;
    cfg.wl_start_round = 20;
    cfg.iso_period = 40;
    cfg.iso_len = 20;
    cfg.iso_mod = 1;
    cfg.maxm = 1;
    cfg.ecap = 1;
    cfg.ring = 8;
    cfg.cid_base = 1;
    cfg.cid_stride = 1;
    cfg.rep_world = 2;
    cfg.rep_rank = r;
    if (!(h[r] = soa_create(&cfg))) return 2;
  }
  std::vector<u8> buf(4 << 20);
  std::vector<rbe_wire_frame> fr(64);
  std::vector<rbe_message> om(4096);
  std::vector<rbe_entry> oe(65536);
  std::vector<u8> oc(4 << 20);
  for (int round = 0; round < 130; round++) {
    u8 bits[2][4] = {{0}};
    u32 epoch = 0;
    for (u32 r = 0; r < 2; r++) soa_iso_leaders(h[r], bits[r], &epoch);
    if (epoch) {
      for (int g = 0; g < 4; g++) bits[0][g] |= bits[1][g];
      for (u32 r = 0; r < 2; r++) soa_set_iso_leaders(h[r], bits[0]);
    }
    for (u32 r = 0; r < 2; r++) soa_run(h[r], 1);
    for (u32 dst = 0; dst < 2; dst++) {
      void* src = h[dst ^ 1u];
      if (wire) {
        const char* addr[7] = {"", "", "", "", "", "", ""};
        u32 nf = 0;
        const int64_t n = soa_wire_encode(src, 0, 0, 0, addr, buf.data(), buf.size(), fr.data(),
                                          &nf, (int32_t)dst);
        if (n < 0) return 3;
        u64 st[6];
        if (soa_wire_ingest_spill(h[dst], buf.data(), (u64)n, st)) return 4;
      } else {
        std::vector<u64> gs;
        std::vector<rbe_message> ms;
        std::vector<rbe_entry> es;
        std::vector<u8> cs;
        for (u64 rep = 0; rep < 12; rep++) {
          if ((rep / 3 + rep % 3) % 2 == dst) continue;  // sender not stepped by src
          u32 n = 0, ne = 0;
          u64 nc = 0;
          if (soa_get_outbox(src, rep, om.data(), (u32)om.size(), &n, oe.data(), (u32)oe.size(), &ne,
                             oc.data(), oc.size(), &nc))
            return 5;
          u32 ei = 0;
          u64 ci = 0;
          for (u32 i = 0; i < n; i++) {
            const bool take = (rep / 3 + (om[i].to - 1)) % 2 == dst;
            for (u32 j = 0; j < om[i].n_entries; j++, ei++) {
              if (take) {
                es.push_back(oe[ei]);
                cs.insert(cs.end(), oc.begin() + ci, oc.begin() + ci + oe[ei].cmd_len);
              }
              ci += oe[ei].cmd_len;
            }
            if (!take) continue;
            gs.push_back(rep / 3);
            ms.push_back(om[i]);
          }
        }
        cs.push_back(0);
        if (soa_push_messages_spill(h[dst], gs.size(), gs.data(), ms.data(), es.data(), cs.data()))
          return 6;
      }
    }
  }
  u64 committed = 0, peak = 0;
  for (u32 r = 0; r < 2; r++) {
    u64 nfaulty = 0, st[5];
    soa_faults(h[r], &nfaulty);
    if (nfaulty) return 7;
    soa_spill_stats(h[r], st);
    if (st[4]) return 8;
    peak += st[2];
    std::vector<rbe_replica_view> v(12);
    soa_views(h[r], v.data());
    for (u64 i = 0; i < 12; i++)
      if ((i / 3 + i % 3) % 2 == r) committed += v[i].committed;
    soa_destroy(h[r]);
  }
  printf("ingest_cpu %s ok: committed %llu, spill peaks %llu bytes\n", wire ? "frames" : "push",
         (unsigned long long)committed, (unsigned long long)peak);
  return committed > 100 && peak ? 0 : 9;
}
int main() {
  const int a = run_pair(true);
  return a ? a : run_pair(false);
}
#endif
