// TEST-ONLY host build of rbe_collect_dropped: the host build of the step with
// the batched outbox on top (tests/outbox_cpu/outbox_cpu.cpp, included
// unchanged, as that file includes its predecessors), cfg.drop_lists switched
// on after soa_create (soa_set_drop_lists: Params::drop_lists and the P.dent
// plane), plus the passes of dragonboat_amd/csrc/rbe_dropped_kernels.h as
// plain loops over the same RBE_HD functions (dragonboat_amd/csrc/
// rbe_dropped.h), in the device's pass order and over whole 256-lane blocks.
// soa_get_dropped is the per-replica getter, a plain walk of its own.
// tests/dropped_cpu/dropped.py loads it; tests/dropped_cpu/dropped_main.cpp is
// a stand-alone program over it for a sanitizer build.  Never linked into the
// product.
#include "../outbox_cpu/outbox_cpu.cpp"

#include "../../dragonboat_amd/csrc/rbe_dropped.h"

namespace {

constexpr u64 kDrBlock = 256;  // kBlock of the device passes

// one set of buffers, shared by every engine of the process: a list is valid
// until the next call
struct DrBuf {
  std::vector<u64> rep, ent_off, ri_off, cmd_off, src;
  std::vector<DrSrc> dsrc;
  std::vector<rbe_entry> ents;
  std::vector<rbe_system_ctx> ctx;
  std::vector<u32> plen;
  std::vector<u8> cmds;
};
DrBuf g_dr;
// blocks the entries and context passes run beyond what the totals need
u64 g_dr_extra_blocks = 0;
// passes the last call ran, counted where the device launches (a scan's three
// launches as one): count, scan and write always; the entries, context and Cmd
// copy passes only when their total is not 0; the Cmd sum, scan and offsets
// with Cmds.  At most 9 (5 without Cmds), whatever is listed.
u32 g_dr_passes = 0;

int dr_collect(SoaEngine* e, const DrArgs& a, bool cmds, rbe_dropped_list* out) {
  DrBuf& B = g_dr;
  B = DrBuf();
  g_dr_passes = 0;
  // records still staged for the next step go to the heap now, as
  // heap_upload_staged does (run_round writes the same bytes again)
  const HostHeap& hp = e->hin.heap;
  for (u64 p = hp.flushed; hp.cap && p < hp.head; p++) e->heap[p % hp.cap] = hp.stage[p - hp.flushed];
  const u8* heap = e->heap.empty() ? nullptr : e->heap.data();
  u32 err = 0;
  // k_dr_count: every lane of every block, those past the range included
  const u64 nb = (a.count + kDrBlock - 1) / kDrBlock, lanes = nb * kDrBlock;
  std::vector<u32> ne(lanes, 0), nr(lanes, 0);
  for (u64 i = 0; i < lanes; i++)
    if (i < a.count) dropped_view(e->P, e->C, a.first + i, a, &ne[i], &nr[i], nullptr, &err);
  g_dr_passes++;
  if (err) return collect_rc(err);
  // the scan: exclusive prefixes and the totals
  std::vector<u64> at(lanes + 1, 0), be(lanes + 1, 0), br(lanes + 1, 0);
  for (u64 i = 0; i < lanes; i++) {
    at[i + 1] = at[i] + ((ne[i] | nr[i]) ? 1 : 0);
    be[i + 1] = be[i] + ne[i];
    br[i + 1] = br[i] + nr[i];
  }
  g_dr_passes++;
  const u64 n = at[lanes], te = be[lanes], tr = br[lanes];
  // k_dr_write
  B.rep.assign(n, 0);
  B.ent_off.assign(n + 1, 0);
  B.ri_off.assign(n + 1, 0);
  B.dsrc.assign(n, DrSrc{});
  const DrOut oo{B.rep.data(), B.ent_off.data(), B.ri_off.data(), B.dsrc.data()};
  for (u64 i = 0; i < lanes; i++) {
    if (i == 0) {
      oo.ent_off[n] = te;
      oo.ri_off[n] = tr;
    }
    u32 e2 = 0, r2 = 0;
    if (i < a.count) dropped_view(e->P, e->C, a.first + i, a, &e2, &r2, nullptr, &err);
    if (e2 != ne[i] || r2 != nr[i]) abort();  // (the passes see one state)
    if (!(e2 | r2)) continue;
    dropped_write(e->P, e->C, a.first + i, a, at[i], be[i], br[i], oo, &err);
  }
  g_dr_passes++;
  // k_dr_entries: whole blocks, a grid that may be larger than the total
  const u64 nb2 = (te + kDrBlock - 1) / kDrBlock + g_dr_extra_blocks;
  B.ents.assign(te, rbe_entry{});
  B.plen.assign(te, 0);
  B.src.assign(te, kCeInline);
  for (u64 b = 0; b < nb2; b++)
    for (u64 base = b * kDrBlock; base < te; base += nb2 * kDrBlock)
      for (u64 t = 0; t < kDrBlock; t++) {
        const u64 j = base + t;
        if (j >= te) continue;
        CeEnt x;
        err |= dropped_entry(e->P, e->C, heap, hp.head, B.ent_off.data(), B.dsrc.data(), n, j, &x);
        B.ents[j] = x.e;
        B.plen[j] = x.plen;
        B.src[j] = x.src;
      }
  if (te) g_dr_passes++;  // (the device skips the launch when nothing is listed)
  // k_dr_ctx
  const u64 nb3 = (tr + kDrBlock - 1) / kDrBlock + g_dr_extra_blocks;
  B.ctx.assign(tr, rbe_system_ctx{});
  for (u64 b = 0; b < nb3; b++)
    for (u64 j = b * kDrBlock; j < tr; j += nb3 * kDrBlock)
      for (u64 t = 0; t < kDrBlock && j + t < tr; t++)
        B.ctx[j + t] = dropped_ctx(e->P, B.ri_off.data(), B.dsrc.data(), n, j + t);
  if (tr) g_dr_passes++;
  if (err) return collect_rc(err);
  if (cmds) {  // k_ce_cmd_sum / the scan / k_ce_cmd_off / k_ce_cmds
    B.cmd_off.assign(te + 1, 0);
    for (u64 j = 0; j < te; j++) B.cmd_off[j + 1] = B.cmd_off[j] + B.plen[j];
    g_dr_passes += 3;
    B.cmds.assign(B.cmd_off[te], 0);
    for (u64 j = 0; j < te; j++) {
      u32 words = ce_padded(B.ents[j].cmd_len) >> 4;
      if (B.src[j] == kCeInline && words > 1) words = 1;
      for (u32 w = 0; w < words; w++) {
        const CeWord v = collect_cmd_word(heap, B.ents[j], B.src[j], w);
        memcpy(B.cmds.data() + B.cmd_off[j] + 16ull * w, &v, 16);
      }
    }
    if (B.cmd_off[te]) g_dr_passes++;
  }
  out->n = n;
  out->n_entries = te;
  out->n_read_indexes = tr;
  out->replica = B.rep.data();
  out->ent_off = B.ent_off.data();
  out->entries = B.ents.data();
  out->ri_off = B.ri_off.data();
  out->read_indexes = B.ctx.data();
  if (cmds) {
    out->cmd_bytes = B.cmd_off[te];
    out->cmd_off = B.cmd_off.data();
    out->cmds = B.cmds.data();
  }
  return RBE_OK;
}

}  // namespace

extern "C" {

// cfg.drop_lists on the host build: before the first step
int soa_set_drop_lists(void* h) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || e->round != 0) return RBE_E_STATE;
  if (!e->P.dent) e->P.dent = alloc<DentRow>(e, e->C.n_rep);
  e->C.drop_lists = 1;
  return RBE_OK;
}

void soa_dropped_extra_blocks(uint64_t n) { g_dr_extra_blocks = n; }
uint32_t soa_dropped_passes(void) { return g_dr_passes; }

int soa_collect_dropped(void* h, uint64_t first, uint64_t count, uint32_t flags,
                        rbe_dropped_list* out) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !out || count == 0 || first >= e->C.n_rep || count > e->C.n_rep - first ||
      (flags & ~RBE_ENTRIES_NO_CMDS))
    return RBE_E_INVALID;
  if (!e->C.drop_lists) return RBE_E_STATE;
  memset(out, 0, sizeof(*out));
  out->first = first;
  out->count = count;
  static const uint64_t zero = 0;
  if (e->round == 0) {
    out->ent_off = out->ri_off = &zero;
    if (!(flags & RBE_ENTRIES_NO_CMDS)) out->cmd_off = &zero;
    return RBE_OK;
  }
  const DrArgs a{first, count, e->round};
  const int rc = dr_collect(e, a, !(flags & RBE_ENTRIES_NO_CMDS), out);
  if (rc) memset(out, 0, sizeof(*out));
  return rc;
}

// rbe_get_dropped on the host build: a walk of its own over the Upd, the
// P.dent row and the P.dri list (rbe_spill.h dri_list)
int soa_get_dropped(void* h, uint64_t replica, rbe_entry* ents, uint32_t ent_cap, uint32_t* n_ents,
                    uint8_t* cmd, uint64_t cmd_cap, uint64_t* cmd_bytes, rbe_system_ctx* ctx,
                    uint32_t ctx_cap, uint32_t* n_ctx) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !n_ents || !n_ctx || replica >= e->C.n_rep) return RBE_E_INVALID;
  if (!e->C.drop_lists) return RBE_E_STATE;
  *n_ents = *n_ctx = 0;
  if (cmd_bytes) *cmd_bytes = 0;
  if (e->round == 0 || !owns_replica(e->C, replica / e->C.n, (u32)(replica % e->C.n)))
    return RBE_OK;
  const Upd& u = e->P.upd[replica];
  if (u.round != e->round - 1 || !(u.flags & UF_RANGES)) return RBE_OK;
  const u32 par = u.round & 1u;
  const DropRI* dl = dri_list(e->P, e->C, replica, u.n_drop_ri, par);
  for (u32 i = 0; i < u.n_drop_ri && i < ctx_cap && ctx; i++) {
    ctx[i].low = dl[i].low;
    ctx[i].high = dl[i].high;
  }
  *n_ctx = u.n_drop_ri;
  const DentRow d = e->P.dent[replica];
  const u32 n = (u.n_drop_ent && d.round == u.round) ? d.n : 0;
  const Ent* en = spill_at<const Ent>(e->P, par, d.granule);
  auto rd = [e](u64 pos, u64 off, u64 len, u8* dst) { return soa_read_heap(e, pos, off, len, dst); };
  u64 nc = 0;
  for (u32 i = 0; i < n; i++) {
    const bool room_c = cmd && nc + en[i].len <= cmd_cap;
    rbe_entry tmp;
    rbe_entry* o = (ents && i < ent_cap) ? &ents[i] : &tmp;
    *o = rbe_entry{};
    const int rc = entry_out(en[i], o, room_c ? cmd + nc : nullptr, rd);
    if (rc) return rc;
    nc += en[i].len;
  }
  *n_ents = n;
  if (cmd_bytes) *cmd_bytes = nc;
  return RBE_OK;
}

// rbe_get_updates: the last round's Updates (rbe_host.h update_view), whose
// counts the tests compare the lists' lengths with
int soa_get_updates(void* h, uint64_t first, uint64_t count, rbe_update* out) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !out || first >= e->C.n_rep || count > e->C.n_rep - first) return RBE_E_INVALID;
  for (u64 i = 0; i < count; i++) {
    const u64 r = first + i;
    update_view(e->P.upd[r], e->P.core[r], e->P.hot[r], e->round, out[i]);
  }
  return RBE_OK;
}

// rbe_import_groups with cfg.drop_lists: the imported range's P.dent rows are zeroed
int soa_import_groups_dropped(void* h, const void* buf, uint64_t bytes, uint32_t flags) {
  SoaEngine* e = (SoaEngine*)h;
  const int rc = soa_import_groups(h, buf, bytes, flags);
  if (rc || !e->P.dent) return rc;
  SnapHeader hd;
  memcpy(&hd, buf, sizeof(hd));
  memset(e->P.dent + hd.first * e->C.n, 0, hd.count * e->C.n * sizeof(DentRow));
  return rc;
}

}  // extern "C"
