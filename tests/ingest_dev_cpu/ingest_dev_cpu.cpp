// TEST-ONLY stand-alone program: the device pipeline of the spilling inbound
// transport (rbe_engine.hip rbe_wire_ingest / rbe_push_messages) as host loops
// over the lane functions its kernels call (dragonboat_amd/csrc/
// rbe_ingest_spill.h ingest_walk_lane, ingest_share_gate, ingest_share_commit),
// beside the host build of tests/ingest_cpu (included unchanged), for a
// sanitizer build (tests/test_ingest_dev.py).
//
// Two pairs of engines (rep_world = 2) of 4 x 3 with the isolation schedule
// 40 / 20 and maxm = ecap = 1 step 100 rounds in lockstep.  Pair A takes every
// hop through ingest_spill_t / push_spill_t; pair B through the passes the
// device runs, in their order: keys (lane per message), stable sort, heap-byte
// scan, checking walk (lane per sorted position, the need array), the needs'
// scan in 256-lane blocks (k_scan_blocks / k_scan_top / k_scan_add), the share
// gate, the gated writing walk, the commit.  Even rounds launch for exactly the
// batch's messages (the exact path), odd rounds for a capacity above it with
// drop keys behind the batch (the no-read-back path).  After every hop the
// message planes, count rows, arenas, spill heaps and SpillCtl words of B must
// equal A's byte for byte.  Each run is made with the next round's step in the
// summary-word form (staged = 4) and in the plain form, over frames and over
// the raftpb-form call.
#include "../ingest_cpu/ingest_cpu.cpp"

#include <cstdio>

namespace {

// k_scan_blocks / k_scan_top / k_scan_add: exclusive scan of v[0, n) in place,
// top[nbk] = the total
void scan_dev(std::vector<u64>& v, u64 n, std::vector<u64>& top) {
  const u64 nbk = (n + 255) / 256;
  top.assign(nbk + 1, 0);
  for (u64 b = 0; b < nbk; b++) {
    u64 t = 0;
    for (u64 j = b * 256; j < n && j < (b + 1) * 256; j++) {
      const u64 x = v[j];
      v[j] = t;
      t += x;
    }
    top[b] = t;
  }
  u64 carry = 0;
  for (u64 b = 0; b < nbk; b++) {
    const u64 x = top[b];
    top[b] = carry;
    carry += x;
  }
  top[nbk] = carry;
  for (u64 j = 0; j < n; j++) v[j] += top[j / 256];
}

// rbe_wire_ingest's device passes for a stream ingest_spill_t has accepted or
// refused (the frames' checks are not repeated).  `cap_form`: launch for a
// capacity above the batch, as the no-read-back path does.  *took: granules.
template <int N>
int dev_ingest_t(SoaEngine* e, const uint8_t* d, uint64_t bytes, bool cap_form, u64* took) {
  const Params& C = e->C;
  *took = 0;
  std::vector<std::pair<u64, u64>> pos;
  for (u64 i = 0; i < bytes;) {
    if (bytes - i < kWireHeader) return RBE_E_CORRUPT;
    u64 size = 0;
    for (int b = 0; b < 8; b++) size = (size << 8) | d[i + 4 + b];
    if (size == 0 || size > bytes - i - kWireHeader) return RBE_E_CORRUPT;
    const u64 off = i + kWireHeader;
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
    i = off + size;
  }
  const u64 tm = pos.size();
  if (!tm) return RBE_OK;
  const u64 nm = cap_form ? tm + tm / 4 + 1024 : tm;  // note_ingest_caps
  std::vector<u64> ent0(nm + 1, 0), cmd0(nm + 1, 0);
  for (u64 j = 0; j < tm; j++) {
    WireRd rd{d, pos[j].first + pos[j].second, pos[j].first, false};
    u64 cb = 0;
    const u32 ne = wire_message_get(rd, pos[j].first + pos[j].second, nullptr, nullptr, nullptr, &cb);
    if (rd.bad) return RBE_E_CORRUPT;
    ent0[j + 1] = ent0[j] + ne;
    cmd0[j + 1] = cmd0[j] + cb;
  }
  for (u64 j = tm; j < nm; j++) ent0[j + 1] = ent0[tm], cmd0[j + 1] = cmd0[tm];
  // exactly sized: a sanitizer sees any index past the records
  std::vector<rbe_message> msgs(nm);
  std::vector<rbe_entry> ents(ent0[tm] + 1);
  std::vector<u8> cmd(cmd0[tm] + 1);
  for (u64 j = 0; j < tm; j++) {
    WireRd rd{d, pos[j].first + pos[j].second, pos[j].first, false};
    u64 cb = cmd0[j];
    wire_message_get(rd, pos[j].first + pos[j].second, &msgs[j], ents.data() + ent0[j], cmd.data(),
                     &cb);
  }
  HostHeap& H = e->hin.heap;
  // k_ing_key: lane per launched message
  std::vector<u64> key(nm), hb(nm);
  std::vector<u32> idx(nm);
  u32 gate[2] = {0, 0};  // [0] the ingest checks, [1] the decode's flags
  for (u64 j = 0; j < nm; j++) {
    idx[j] = (u32)j;
    if (j >= tm) {
      key[j] = ing_drop_key(C);
      hb[j] = 0;
      continue;
    }
    u32 x = 0;
    ingest_ids<N>(C, e->hin.id_table(), msgs[j]);
    key[j] = ingest_check<N>(C, H.cap, msgs[j], ents.data() + ent0[j], &x, &hb[j], true);
    gate[0] |= x;
  }
  // the stable pair sort, k_ing_gather, the heap bytes' scan
  std::vector<u32> sidx(idx);
  std::stable_sort(sidx.begin(), sidx.end(), [&](u32 a, u32 b) { return key[a] < key[b]; });
  std::vector<u64> skey(nm), hs(nm), top, sn(nm, ~0ull), stop;
  for (u64 p = 0; p < nm; p++) {
    skey[p] = key[sidx[p]];
    hs[p] = hb[sidx[p]];
  }
  scan_dev(hs, nm, top);
  const u32 par = (e->round - 1) & 1u;
  const u64 lanes = (nm + 255) / 256 * 256;  // whole blocks are launched
  // checking walk, lane per sorted position
  for (u64 p = 0; p < lanes; p++)
    ingest_walk_lane<N, false>(e->P, C, par, e->round, skey.data(), sidx.data(), p, nm, msgs.data(),
                               ents.data(), ent0.data(), cmd0.data(), cmd.data(), nullptr, H.cap, 0,
                               hs.data(), sn.data(), nullptr, nullptr);
  scan_dev(sn, nm, stop);
  u64 ctl[IC_WORDS] = {0, 0, 0, 0};
  ingest_share_gate(C, e->P.sctl, par, stop[(nm + 255) / 256], ctl, &gate[0]);
  if (gate[0] & ING_INVALID) return RBE_E_INVALID;
  if (gate[0] & ING_NOMEM) return RBE_E_NOMEM;
  if (!cap_form) {  // the exact path's host check of the read-back words
    const u64 share = spill_share(C);
    const bool refuse = ctl[IC_TOTAL] > (ctl[IC_USED] < share ? share - ctl[IC_USED] : 0);
    if (refuse != ((gate[0] & ING_SHARE) != 0)) return 100;
  }
  if (top[(nm + 255) / 256]) return 101;  // (no payload heap in these runs)
  // the gated writing walk and the gated commit run whatever the gate says
  for (u64 p = 0; p < lanes; p++)
    ingest_walk_lane<N, true>(e->P, C, par, e->round, skey.data(), sidx.data(), p, nm, msgs.data(),
                              ents.data(), ent0.data(), cmd0.data(), cmd.data(), e->heap.data(), H.cap,
                              0, hs.data(), sn.data(), ctl, gate);
  ingest_share_commit(e->P.sctl, par, stop[(nm + 255) / 256], gate);
  if (gate[0] & ING_SHARE) return RBE_E_NOMEM;
  *took = ctl[IC_TOTAL];
  return RBE_OK;
}

// rbe_push_messages' device form: the host reads `used`, reserves, scatters
// the records, and the commit lane takes the total
template <int N>
int dev_push_t(SoaEngine* e, uint64_t n, const uint64_t* group, const rbe_message* msgs,
               const rbe_entry* ents, const uint8_t* cmd, u64* took) {
  std::vector<XCnt> c;
  std::vector<XMsg> m;
  std::vector<XEnt> x;
  *took = 0;
  const u32 par = (e->round - 1) & 1u;
  const u64 used = e->P.sctl->used[par], share = spill_share(e->C);
  XSpillRes sp{share * e->C.rep_rank + used, used < share ? share - used : 0, 0};
  const int rc = messages_to_records<N>(e->C, e->hin.heap, e->round, n, group, msgs, ents, cmd, c,
                                        m, x, e->hin.id_table(), &sp);
  if (rc) return rc;
  soa_xchg_unpack_t<N>(e, c.data(), c.size(), m.data(), m.size(), x.data(), x.size());
  if (sp.total) ingest_share_commit(e->P.sctl, par, sp.total, nullptr);
  *took = sp.total;
  return RBE_OK;
}

void* make_engine(u32 rank, int staged) {
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
  cfg.rep_rank = rank;
  void* h = soa_create(&cfg);
  if (h) soa_set_staged(h, staged);
  return h;
}

// what an inbound batch may have written, and the words that place it
bool same_inbox(const SoaEngine* a, const SoaEngine* b) {
  const Params& C = a->C;
  const u64 G = C.n_groups, N = C.n, R = C.n_rep;
  if (memcmp(a->P.msgs[0], b->P.msgs[0], 2 * G * N * N * C.maxm * sizeof(Msg))) return false;
  if (memcmp(a->P.cnt[0], b->P.cnt[0], 2 * R * sizeof(CntRow))) return false;
  if (memcmp(a->P.arena[0], b->P.arena[0], 2 * R * C.ecap * sizeof(Ent))) return false;
  if (memcmp(a->P.spill[0], b->P.spill[0], 2 * C.spill_units * 16)) return false;
  if (memcmp(a->P.gwake, b->P.gwake, G)) return false;
  const SpillCtl *x = a->P.sctl, *y = b->P.sctl;
  return x->used[0] == y->used[0] && x->used[1] == y->used[1] && x->peak[0] == y->peak[0] &&
         x->peak[1] == y->peak[1] && x->oom == y->oom;
}

// the hop's batch for engine dst out of engine src, in raftpb form
int gather_push(void* src, u32 dst, std::vector<u64>& gs, std::vector<rbe_message>& ms,
                std::vector<rbe_entry>& es, std::vector<u8>& cs) {
  static std::vector<rbe_message> om(4096);
  static std::vector<rbe_entry> oe(65536);
  static std::vector<u8> oc(4 << 20);
  for (u64 rep = 0; rep < 12; rep++) {
    if ((rep / 3 + rep % 3) % 2 == dst) continue;  // sender not stepped by src
    u32 n = 0, ne = 0;
    u64 nc = 0;
    if (soa_get_outbox(src, rep, om.data(), (u32)om.size(), &n, oe.data(), (u32)oe.size(), &ne,
                       oc.data(), oc.size(), &nc))
      return 1;
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
  return 0;
}

int run_pairs(bool wire, int staged) {
  void *a[2], *b[2];
  for (u32 r = 0; r < 2; r++)
    if (!(a[r] = make_engine(r, staged)) || !(b[r] = make_engine(r, staged))) return 2;
  std::vector<u8> buf(4 << 20), buf2(4 << 20);
  std::vector<rbe_wire_frame> fr(64);
  u64 took_total = 0, hops = 0;
  for (int round = 0; round < 100; round++) {
    for (void** h : {a, b}) {
      u8 bits[2][4] = {{0}};
      u32 epoch = 0;
      for (u32 r = 0; r < 2; r++) soa_iso_leaders(h[r], bits[r], &epoch);
      if (epoch) {
        for (int g = 0; g < 4; g++) bits[0][g] |= bits[1][g];
        for (u32 r = 0; r < 2; r++) soa_set_iso_leaders(h[r], bits[0]);
      }
      for (u32 r = 0; r < 2; r++) soa_run(h[r], 1);
    }
    for (u32 dst = 0; dst < 2; dst++) {
      u64 took = 0;
      int ra, rb;
      if (wire) {
        const char* addr[7] = {"", "", "", "", "", "", ""};
        u32 nf = 0;
        const int64_t n = soa_wire_encode(a[dst ^ 1u], 0, 0, 0, addr, buf.data(), buf.size(),
                                          fr.data(), &nf, (int32_t)dst);
        const int64_t n2 = soa_wire_encode(b[dst ^ 1u], 0, 0, 0, addr, buf2.data(), buf2.size(),
                                           fr.data(), &nf, (int32_t)dst);
        if (n < 0 || n != n2 || memcmp(buf.data(), buf2.data(), (size_t)n)) return 3;
        // exactly sized, so that a read past the stream is seen
        std::vector<u8> stream(buf.begin(), buf.begin() + n);
        u64 st[6];
        ra = soa_wire_ingest_spill(a[dst], stream.data(), (u64)n, st);
        rb = with_n(3, [&](auto NN) {
          return dev_ingest_t<decltype(NN)::value>((SoaEngine*)b[dst], stream.data(), (u64)n,
                                                   (round & 1) != 0, &took);
        });
      } else {
        std::vector<u64> gs, gs2;
        std::vector<rbe_message> ms, ms2;
        std::vector<rbe_entry> es, es2;
        std::vector<u8> cs, cs2;
        if (gather_push(a[dst ^ 1u], dst, gs, ms, es, cs) ||
            gather_push(b[dst ^ 1u], dst, gs2, ms2, es2, cs2))
          return 5;
        if (gs != gs2 || cs != cs2 || ms.size() != ms2.size() || es.size() != es2.size()) return 5;
        ra = soa_push_messages_spill(a[dst], gs.size(), gs.data(), ms.data(), es.data(), cs.data());
        rb = with_n(3, [&](auto NN) {
          return dev_push_t<decltype(NN)::value>((SoaEngine*)b[dst], gs2.size(), gs2.data(),
                                                 ms2.data(), es2.data(), cs2.data(), &took);
        });
      }
      if (ra || rb) {
        fprintf(stderr, "round %d dst %u: host build %d, device passes %d\n", round, dst, ra, rb);
        return 4;
      }
      if (!same_inbox((SoaEngine*)a[dst], (SoaEngine*)b[dst])) {
        fprintf(stderr, "round %d dst %u: the device passes left other bytes\n", round, dst);
        return 6;
      }
      took_total += took;
      hops += took != 0;
    }
  }
  u64 committed = 0, peak = 0;
  for (u32 r = 0; r < 2; r++) {
    std::vector<rbe_replica_view> va(12), vb(12);
    soa_views(a[r], va.data());
    soa_views(b[r], vb.data());
    for (void* h : {a[r], b[r]}) {
      u64 nfaulty = 0, st[5];
      soa_faults(h, &nfaulty);
      if (nfaulty) return 7;
      soa_spill_stats(h, st);
      if (st[4]) return 8;
      if (h == b[r]) peak += st[2];
    }
    for (u64 i = 0; i < 12; i++) {
      if ((i / 3 + i % 3) % 2 != r) continue;
      if (va[i].committed != vb[i].committed || va[i].term != vb[i].term ||
          va[i].digest != vb[i].digest)
        return 9;
      committed += vb[i].committed;
    }
    soa_destroy(a[r]);
    soa_destroy(b[r]);
  }
  printf("ingest_dev_cpu %s staged=%d ok: committed %llu, spill peaks %llu bytes, inbound %llu bytes "
         "in %llu hops\n", wire ? "frames" : "push", staged, (unsigned long long)committed,
         (unsigned long long)peak, (unsigned long long)(took_total * 16), (unsigned long long)hops);
  return committed > 50 && peak && took_total ? 0 : 10;
}

// the share gate and the commit at the edges of a share
int gate_edges() {
  Params C;
  memset(&C, 0, sizeof(C));
  C.rep_world = 2;
  C.rep_rank = 1;
  C.spill_units = 128;  // 64 granules per rank
  SpillCtl s;
  memset(&s, 0, sizeof(s));
  u64 ctl[IC_WORDS];
  u32 gate[2] = {0, 0};
  s.used[1] = 10;
  ingest_share_gate(C, &s, 1, 54, ctl, gate);  // exactly what is left
  if (gate[0] || ctl[IC_BASE] != 64 + 10 || ctl[IC_TOTAL] != 54 || ctl[IC_USED] != 10) return 1;
  ingest_share_gate(C, &s, 1, 55, ctl, gate);
  if (gate[0] != ING_SHARE) return 2;
  ingest_share_commit(&s, 1, 55, gate);  // gated: nothing moves
  if (s.used[1] != 10 || s.peak[1] != 0) return 3;
  gate[0] = 0;
  s.used[0] = 70;  // a round that ran out left `used` past the share
  ingest_share_gate(C, &s, 0, 0, ctl, gate);
  if (gate[0]) return 4;
  ingest_share_gate(C, &s, 0, 1, ctl, gate);
  if (gate[0] != ING_SHARE) return 5;
  gate[0] = 0;
  ingest_share_commit(&s, 1, 0, gate);  // an empty total raises no peak
  if (s.used[1] != 10 || s.peak[1] != 0) return 6;
  ingest_share_commit(&s, 1, 54, gate);
  if (s.used[1] != 64 || s.peak[1] != 64 || s.used[0] != 70 || s.peak[0] != 0 || s.oom) return 7;
  return 0;
}

}  // namespace

int main() {
  if (const int g = gate_edges()) {
    fprintf(stderr, "gate_edges: %d\n", g);
    return 20 + g;
  }
  for (int staged : {4, 0})
    for (bool wire : {true, false})
      if (const int rc = run_pairs(wire, staged)) return rc;
  printf("ingest_dev_cpu ok\n");
  return 0;
}
