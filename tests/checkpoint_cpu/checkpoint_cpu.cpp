// TEST-ONLY host build of rbe_export_groups_ex and of the heap section of
// rbe_import_groups: the host build of the step (tests/soa_cpu/soa_cpu.cpp,
// included unchanged, through tests/collect_cpu/collect_cpu.cpp for the batched
// entry reads the scenarios compare with) plus the passes of
// dragonboat_amd/csrc/rbe_checkpoint_kernels.h as plain loops over the same
// RBE_HD functions (dragonboat_amd/csrc/rbe_checkpoint.h), run on the planes of
// a SoaEngine.  tests/checkpoint_cpu/checkpoint.py loads it; with
// -DCHECKPOINT_CPU_MAIN a stand-alone program that runs a small heap engine,
// exports it with the heap section, resumes a fresh engine and reads its logs
// back (for a sanitizer build).  Never linked into the product.
#include "../collect_cpu/collect_cpu.cpp"

#include <algorithm>

#include "../../dragonboat_amd/csrc/rbe_checkpoint.h"

namespace {

// records still staged for the next step go to the heap now (ck_export's upload)
void upload_staged(SoaEngine* e) {
  const HostHeap& hp = e->hin.heap;
  for (u64 p = hp.flushed; hp.cap && p < hp.head; p++) e->heap[p % hp.cap] = hp.stage[p - hp.flushed];
}

// 16-B aligned bytes
struct Aligned {
  std::vector<u64> w;
  u8* p = nullptr;
  explicit Aligned(u64 bytes) : w(bytes / 8 + 4, 0) {
    p = (u8*)(((uintptr_t)w.data() + 15) & ~(uintptr_t)15);
  }
};

}  // namespace

extern "C" {

int soa_export_groups_ex(void* h, uint64_t first, uint64_t count, uint32_t flags, void* buf,
                         uint64_t cap, uint64_t* bytes) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !bytes || count == 0 || first >= e->C.n_groups || count > e->C.n_groups - first ||
      (flags & ~RBE_EXPORT_HEAP))
    return RBE_E_INVALID;
  const Planes& P = e->P;
  const Params& C = e->C;
  if (soa_range_spilled(e, first, count)) return RBE_E_STATE;
  const bool heap = (flags & RBE_EXPORT_HEAP) && C.heap_bytes;
  if (heap) upload_staged(e);
  const u64 head = e->hin.heap.head;
  const u64 body = snap_body_bytes(P, C, count), r0 = first * C.n, nr = count * C.n;
  // k_ck_count + the scan
  std::vector<u32> np(nr), nq(nr);
  std::vector<u64> pa(nr + 1, 0), ua(nr + 1, 0);
  for (u64 i = 0; i < nr; i++) {
    ck_replica_count(P, C, r0 + i, &np[i], &nq[i]);
    pa[i + 1] = pa[i] + np[i];
    ua[i + 1] = ua[i] + ck_rec_units(np[i], nq[i]);
  }
  const u64 n_pages = pa[nr], lb = ua[nr] * 16;
  Aligned log(lb);
  std::vector<CkPage> list(n_pages + 1);
  u32 err = 0;
  for (u64 i = 0; i < nr; i++)  // k_ck_replicas
    err |= ck_replica_write(P, C, r0 + i, (u32)i, np[i], nq[i], log.p, ua[i] * 16, list.data(), pa[i]);
  for (u64 q = 0; q < n_pages; q++) {  // k_ck_pages
    SnapPage* sp = (SnapPage*)(log.p + list[q].out);
    sp->pn = list[q].pn;
    sp->pad = 0;
    for (u32 j = 0; j < kPageEnts; j++) sp->e[j] = *pool_ent(P, list[q].page, j);
  }
  if (err) return RBE_E_STATE;
  std::vector<u8> sec;
  if (heap) {
    std::vector<std::pair<u64, u32>> refs;  // k_ck_refs
    u64 pos;
    u32 len;
    for (u64 q = 0; q < n_pages; q++) {
      const u64 r = r0 + list[q].rep;
      const SnapPage* sp = (const SnapPage*)(log.p + list[q].out);
      for (u32 j = 0; j < kPageEnts; j++)
        if (ck_held_page(C, ck_marker(P, C, r), P.core[r].last_index, list[q].pn * kPageEnts + j) &&
            ck_heap_ref(C, head, sp->e[j], &pos, &len))
          refs.push_back({pos, len});
    }
    for (u32 s = 0; s < C.ring; s++)
      for (u64 i = 0; i < nr; i++) {
        const u64 r = r0 + i;
        if (ck_ring_index(C, ck_marker(P, C, r), P.core[r].last_index, s) &&
            ck_heap_ref(C, head, ck_ring_ent(P, C, r, s), &pos, &len))
          refs.push_back({pos, len});
      }
    for (u64 i = 0; i < nr; i++) {
      const u32 n = ck_msg_refs(P, C, r0 + i, e->round, head, nullptr, nullptr);
      std::vector<u64> k(n + 1);
      std::vector<u32> v(n + 1);
      ck_msg_refs(P, C, r0 + i, e->round, head, k.data(), v.data());
      for (u32 j = 0; j < n; j++) refs.push_back({k[j], v[j]});
    }
    std::stable_sort(refs.begin(), refs.end(),
                     [](const auto& a, const auto& b) { return a.first < b.first; });  // dev_sort_pairs
    std::vector<SnapHeapRow> rows;  // k_ck_heads / k_ck_table
    std::vector<u64> rec_off;
    u64 units = 0;
    for (u64 i = 0; i < refs.size(); i++) {
      if (i && refs[i].first == refs[i - 1].first) {
        if (refs[i].second != refs[i - 1].second) return RBE_E_STATE;
        continue;
      }
      rows.push_back(SnapHeapRow{refs[i].first, refs[i].second, 0});
      rec_off.push_back(units);
      units += heap_rec_bytes(refs[i].second) / 16;
    }
    rec_off.push_back(units);
    const u64 o_recs = sizeof(SnapHeapHdr) + rows.size() * sizeof(SnapHeapRow);
    sec.assign(o_recs + units * 16, 0);
    const SnapHeapHdr hh{kSnapHeapMagic, rows.size(), head, C.heap_bytes};
    memcpy(sec.data(), &hh, sizeof(hh));
    if (!rows.empty()) memcpy(sec.data() + sizeof(hh), rows.data(), rows.size() * sizeof(SnapHeapRow));
    for (u64 j = 0; j < units; j++) {  // k_ck_records<CK_GATHER>
      const u64 s = ck_slot_of(rec_off.data(), rows.size(), j), w = j - rec_off[s];
      const CeWord v = ck_heap_word(e->heap.data(), C.heap_bytes, rows[s].pos, rows[s].len, w);
      memcpy(sec.data() + o_recs + 16 * j, &v, 16);
    }
  }
  const u64 total = snap_log_at(body) + lb + sec.size();
  *bytes = total;
  if (!buf || cap < total) return RBE_E_NOMEM;
  SnapHeader hd;
  snap_fill_header(C, RBE_ABI_VERSION, e->round, e->tclk, first, count, body, &hd);
  hd.log_bytes = lb;
  memcpy(buf, &hd, sizeof(hd));
  memset((u8*)buf + sizeof(hd) + body, 0, snap_log_at(body) - sizeof(hd) - body);
  if (lb) memcpy((u8*)buf + snap_log_at(body), log.p, lb);
  if (!sec.empty()) memcpy((u8*)buf + snap_log_at(body) + lb, sec.data(), sec.size());
  SnapPlane pl[kSnapPlanes];
  snap_planes(P, C, pl);
  u8* dst = (u8*)buf + sizeof(SnapHeader);
  for (int i = 0; i < kSnapPlanes && pl[i].rows; i++) {
    const u64 w = count * pl[i].group_bytes;
    for (u64 row = 0; row < pl[i].rows; row++, dst += w)
      memcpy(dst, pl[i].base + row * pl[i].pitch + first * pl[i].group_bytes, w);
  }
  return RBE_OK;
}

// rbe_import_groups with the heap section: its checks, and at a hand-off the
// comparison, before soa_import_groups changes anything; the scatter after it
int soa_import_groups_ck(void* h, const void* buf, uint64_t bytes, uint32_t flags) {
  SoaEngine* e = (SoaEngine*)h;
  SnapHeader hd;
  if (!e || !buf || bytes < sizeof(hd)) return RBE_E_INVALID;
  memcpy(&hd, buf, sizeof(hd));
  if (snap_check_header(e->C, RBE_ABI_VERSION, &hd, bytes) ||
      hd.body_bytes != snap_body_bytes(e->P, e->C, hd.count))
    return RBE_E_INVALID;
  const bool resume = (flags & RBE_IMPORT_RESUME) != 0;
  if (resume && (hd.first != 0 || hd.count != e->C.n_groups)) return RBE_E_INVALID;
  if (!resume && hd.round != e->round) return RBE_E_STATE;
  {
    std::vector<u64> rec_off(hd.count * e->C.n);
    if (snap_log_index(e->C, (const u8*)buf, rec_off.size(), rec_off.data())) return RBE_E_INVALID;
  }
  const u64 hs_at = snap_log_at(hd.body_bytes) + hd.log_bytes;
  const u8* hsec = (const u8*)buf + hs_at;
  if (!ck_heap_present(hsec, bytes - hs_at)) return soa_import_groups(h, buf, bytes, flags);
  SnapHeapHdr hh;
  memcpy(&hh, hsec, sizeof(hh));
  if (hh.n_records > (bytes - hs_at) / sizeof(SnapHeapRow)) return RBE_E_INVALID;
  std::vector<u64> off(hh.n_records + 1);
  u64 sb = 0;
  if (ck_heap_check(e->C.heap_bytes, hsec, bytes - hs_at, &sb, off.data())) return RBE_E_INVALID;
  if (resume && !e->hin.empty()) return RBE_E_STATE;
  HostHeap& hp = e->hin.heap;
  const u64 n = hh.n_records, units = off[n];
  std::vector<SnapHeapRow> rows(n + 1);
  if (n) memcpy(rows.data(), hsec + sizeof(hh), n * sizeof(SnapHeapRow));
  const u8* recs = hsec + sizeof(hh) + n * sizeof(SnapHeapRow);
  if (!resume) {  // k_ck_records<CK_COMPARE>
    for (u64 i = 0; i < n; i++)
      if (!hp.valid(rows[i].pos, (u64)kHeapHdr + rows[i].len)) return RBE_E_STATE;
    upload_staged(e);
    for (u64 j = 0; j < units; j++) {
      const u64 s = ck_slot_of(off.data(), n, j), w = j - off[s];
      const CeWord v = ck_heap_word(e->heap.data(), hp.cap, rows[s].pos, rows[s].len, w);
      if (memcmp(&v, recs + 16 * j, 16)) return RBE_E_STATE;
    }
  }
  const int rc = soa_import_groups(h, buf, bytes, flags);
  if (rc || !resume) return rc;
  for (u64 j = 0; j < units; j++) {  // k_ck_records<CK_SCATTER>
    const u64 s = ck_slot_of(off.data(), n, j), w = j - off[s];
    memcpy(e->heap.data() + rows[s].pos % hp.cap + 16 * w, recs + 16 * j, 16);
  }
  hp.stage.clear();
  hp.head = hp.flushed = hp.batch_lo = hh.head;
  hp.round_lo = ~0ull;
  hp.live_lo = 0;
  e->heap_head = hh.head;
  return RBE_OK;
}

}  // extern "C"

#ifdef CHECKPOINT_CPU_MAIN
// A small ext_inputs engine with a payload heap and a ring of 8 (so the logs
// reach into the cold log): proposals of 0-599 bytes at every replica for 80
// rounds; the export with the heap section resumes a fresh engine, whose every
// replica reads its whole log back as the source did, exports the same bytes
// again and keeps stepping.  The plain _ex export equals soa_export_groups.
#include <cstdio>
static int read_all(void* h, u64 R, std::vector<std::vector<u8>>& out, u64* n_heap) {
  std::vector<rbe_replica_view> v(R);
  soa_views(h, v.data());
  out.assign(R, {});
  for (u64 r = 0; r < R; r++) {
    const u64 n = v[r].last_index;
    if (!n) continue;
    std::vector<u64> off(n + 1);
    soa_get_entry_cmds(h, r, 1, n, nullptr, 0, off.data());
    out[r].assign(off[n] + 1, 0);
    if (soa_get_entry_cmds(h, r, 1, n, out[r].data(), off[n], off.data())) return 1;
    for (u64 j = 0; j < n; j++) *n_heap += off[j + 1] - off[j] > 16;
  }
  return 0;
}
int main() {
  rbe_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = RBE_ABI_VERSION;
  cfg.n_groups = 4;
  cfg.n_replicas = 3;
  cfg.election_rtt = 10;
  cfg.heartbeat_rtt = 1;
  cfg.ring = 8;
  cfg.seed = 0x5EEDD8A6;
  cfg.ext_inputs = 1;
  cfg.heap_bytes = 1 << 20;
  void* h = soa_create(&cfg);
  if (!h) return 2;
  const u64 R = 12;
  u64 x = 88172645463325252ull;
  for (int round = 0; round < 80; round++) {
    for (u64 r = 0; r < R; r++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      const u32 len = (u32)(x % 600), one = 1, type = 0;
      std::vector<u8> cmd(len + 1, (u8)(x >> 20));
      if (soa_push_proposals(h, 1, &r, &one, &type, &len, cmd.data())) return 3;
    }
    soa_run(h, 1);
  }
  u64 need = 0, need2 = 0;
  if (soa_export_groups_ex(h, 0, 4, 0, nullptr, 0, &need) != RBE_E_NOMEM) return 4;
  std::vector<u8> plain(need), old(soa_export_bytes(h, 0, 4));
  if (soa_export_groups_ex(h, 0, 4, 0, plain.data(), need, &need2) || need2 != need) return 5;
  if (soa_export_groups(h, 0, 4, old.data(), old.size()) || old != plain) return 6;
  if (soa_export_groups_ex(h, 0, 4, RBE_EXPORT_HEAP, nullptr, 0, &need) != RBE_E_NOMEM) return 7;
  std::vector<u8> snap(need);
  if (soa_export_groups_ex(h, 0, 4, RBE_EXPORT_HEAP, snap.data(), need, &need2)) return 8;
  std::vector<std::vector<u8>> a, b;
  u64 n_heap = 0, n2 = 0;
  if (read_all(h, R, a, &n_heap)) return 9;
  soa_destroy(h);
  void* g = soa_create(&cfg);
  if (!g) return 10;
  if (soa_import_groups_ck(g, snap.data(), snap.size(), RBE_IMPORT_RESUME)) return 11;
  if (read_all(g, R, b, &n2) || a != b) return 12;
  std::vector<u8> again(need);
  if (soa_export_groups_ex(g, 0, 4, RBE_EXPORT_HEAP, again.data(), need, &need2) || again != snap)
    return 13;
  snap[snap.size() - 1] ^= 1;  // a hand-off of other bytes is refused
  if (soa_import_groups_ck(g, snap.data(), snap.size(), 0) != RBE_E_STATE) return 14;
  if (soa_import_groups_ck(g, again.data(), again.size(), 0)) return 15;
  soa_run(g, 10);
  soa_destroy(g);
  printf("checkpoint_cpu ok: %llu bytes (%llu plain), %llu heap entries read back after the resume\n",
         (unsigned long long)snap.size(), (unsigned long long)plain.size(),
         (unsigned long long)n_heap);
  return n_heap ? 0 : 16;
}
#endif
