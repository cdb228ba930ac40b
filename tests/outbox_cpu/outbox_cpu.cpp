// TEST-ONLY host build of rbe_collect_outbox: the host build of the step
// (tests/soa_cpu/soa_cpu.cpp, included unchanged, through the variant with the
// spilling inbound transport, tests/ingest_cpu/ingest_cpu.cpp, which the
// replica-mode shapes need to deliver what they collect) plus the passes of
// dragonboat_amd/csrc/rbe_outbox_kernels.h as plain loops over the same RBE_HD
// functions (dragonboat_amd/csrc/rbe_outbox.h), in the device's pass order and
// over whole 256-lane blocks, run on the planes of a SoaEngine.
// tests/outbox_cpu/outbox.py loads it; tests/outbox_cpu/outbox_main.cpp is a
// stand-alone program over it for a sanitizer build.  Never linked into the
// product.
#include "../ingest_cpu/ingest_cpu.cpp"

#include "../../dragonboat_amd/csrc/rbe_outbox.h"

namespace {

constexpr u64 kObBlock = 256;  // kBlock of the device passes

// one set of buffers, shared by every engine of the process: a list is valid
// until the next call
struct ObBuf {
  std::vector<u64> rep, msg_off, ent_off, cmd_off, src;
  std::vector<rbe_message> msgs;
  std::vector<ObSrc> msrc;
  std::vector<rbe_entry> ents;
  std::vector<u32> plen;
  std::vector<u8> cmds;
};
ObBuf g_ob;
// blocks the entries pass runs beyond what the totals need (outbox_main.cpp: a
// grid larger than the totals, as the device's fixed grid is for a small call)
u64 g_ob_extra_blocks = 0;

int ob_collect(SoaEngine* e, const ObArgs& a, bool cmds, rbe_outbox_list* out) {
  ObBuf& B = g_ob;
  B = ObBuf();
  // records still staged for the next step go to the heap now, as
  // heap_upload_staged does (run_round writes the same bytes again)
  const HostHeap& hp = e->hin.heap;
  for (u64 p = hp.flushed; hp.cap && p < hp.head; p++) e->heap[p % hp.cap] = hp.stage[p - hp.flushed];
  const u8* heap = e->heap.empty() ? nullptr : e->heap.data();
  u32 err = 0;
  // k_ob_count: every lane of every block, those past the range included
  const u64 nb = (a.count + kObBlock - 1) / kObBlock, lanes = nb * kObBlock;
  std::vector<u32> nm(lanes, 0), ne(lanes, 0);
  for (u64 i = 0; i < lanes; i++)
    if (i < a.count) outbox_count(e->P, e->C, a.first + i, a, &nm[i], &ne[i], &err);
  if (err) return collect_rc(err);
  // the scan: exclusive prefixes and the totals
  std::vector<u64> at(lanes + 1, 0), bm(lanes + 1, 0), be(lanes + 1, 0);
  for (u64 i = 0; i < lanes; i++) {
    at[i + 1] = at[i] + (nm[i] ? 1 : 0);
    bm[i + 1] = bm[i] + nm[i];
    be[i + 1] = be[i] + ne[i];
  }
  const u64 n = at[lanes], tm = bm[lanes], te = be[lanes];
  // k_ob_msgs
  B.rep.assign(n, 0);
  B.msg_off.assign(n + 1, 0);
  B.msgs.assign(tm, rbe_message{});
  B.ent_off.assign(tm + 1, 0);
  B.msrc.assign(tm, ObSrc{});
  const ObOut oo{B.rep.data(), B.msg_off.data(), B.msgs.data(), B.ent_off.data(), B.msrc.data()};
  for (u64 i = 0; i < lanes; i++) {
    if (i == 0) {
      oo.msg_off[n] = tm;
      oo.ent_off[tm] = te;
    }
    u32 m2 = 0, e2 = 0;
    if (i < a.count) outbox_count(e->P, e->C, a.first + i, a, &m2, &e2, &err);
    if (m2 != nm[i] || e2 != ne[i]) abort();  // (the passes see one state)
    if (!m2) continue;
    outbox_write(e->P, e->C, a.first + i, a, at[i], bm[i], be[i], oo, &err);
  }
  // k_ob_entries: whole blocks, a grid that may be larger than the total
  const u64 nb2 = (te + kObBlock - 1) / kObBlock + g_ob_extra_blocks;
  B.ents.assign(te, rbe_entry{});
  B.plen.assign(te, 0);
  B.src.assign(te, kCeInline);
  for (u64 b = 0; b < nb2; b++)
    for (u64 base = b * kObBlock; base < te; base += nb2 * kObBlock)
      for (u64 t = 0; t < kObBlock; t++) {
        const u64 j = base + t;
        if (j >= te) continue;
        CeEnt x;
        err |= outbox_entry(e->P, e->C, heap, hp.head, B.ent_off.data(), B.msrc.data(), tm, j, &x);
        B.ents[j] = x.e;
        B.plen[j] = x.plen;
        B.src[j] = x.src;
      }
  if (err) return collect_rc(err);
  if (cmds) {  // k_ce_cmd_sum / k_ce_cmd_off / k_ce_cmds
    B.cmd_off.assign(te + 1, 0);
    for (u64 j = 0; j < te; j++) B.cmd_off[j + 1] = B.cmd_off[j] + B.plen[j];
    B.cmds.assign(B.cmd_off[te], 0);
    for (u64 j = 0; j < te; j++) {
      u32 words = ce_padded(B.ents[j].cmd_len) >> 4;
      if (B.src[j] == kCeInline && words > 1) words = 1;
      for (u32 w = 0; w < words; w++) {
        const CeWord v = collect_cmd_word(heap, B.ents[j], B.src[j], w);
        memcpy(B.cmds.data() + B.cmd_off[j] + 16ull * w, &v, 16);
      }
    }
  }
  out->n = n;
  out->n_messages = tm;
  out->n_entries = te;
  out->replica = B.rep.data();
  out->msg_off = B.msg_off.data();
  out->messages = B.msgs.data();
  out->ent_off = B.ent_off.data();
  out->entries = B.ents.data();
  if (cmds) {
    out->cmd_bytes = B.cmd_off[te];
    out->cmd_off = B.cmd_off.data();
    out->cmds = B.cmds.data();
  }
  return RBE_OK;
}

}  // namespace

extern "C" {

void soa_outbox_extra_blocks(uint64_t n) { g_ob_extra_blocks = n; }

int soa_collect_outbox(void* h, uint64_t first, uint64_t count, uint32_t flags, int32_t dst_rank,
                       rbe_outbox_list* out) {
  SoaEngine* e = (SoaEngine*)h;
  if (!e || !out || count == 0 || first >= e->C.n_rep || count > e->C.n_rep - first ||
      (flags & ~(RBE_COLLECT_REMOTE_MSGS | RBE_ENTRIES_NO_CMDS)) ||
      !outbox_rank_ok(e->C, dst_rank))
    return RBE_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->first = first;
  out->count = count;
  static const uint64_t zero = 0;
  if (e->round == 0) {
    out->msg_off = out->ent_off = &zero;
    if (!(flags & RBE_ENTRIES_NO_CMDS)) out->cmd_off = &zero;
    return RBE_OK;
  }
  const ObArgs a{first, count, e->round, (flags & RBE_COLLECT_REMOTE_MSGS) ? 1u : 0u, dst_rank};
  const int rc = ob_collect(e, a, !(flags & RBE_ENTRIES_NO_CMDS), out);
  if (rc) memset(out, 0, sizeof(*out));
  return rc;
}

}  // extern "C"
