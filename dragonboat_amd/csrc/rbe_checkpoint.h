// Self-contained checkpoints (rbe_export_groups_ex, include/rbe.h): the device
// gather of a snapshot's log section and the payload-heap section that follows
// it.  The per-replica, per-page and per-record logic, shared by the HIP
// kernels (rbe_checkpoint_kernels.h) and the host build of the CPU test tier
// (tests/checkpoint_cpu/checkpoint_cpu.cpp).
//
// The log section is the one rbe_snap.h snap_log_write produces, byte for byte:
// a replica's SnapLogRec, its cold log's pages in chain order, its pooled
// readIndex requests.  Here each chain is walked once by its replica's lane to
// list its pages; the pages themselves are copied a wave per page.
//
// The heap section, 16-B aligned after the log section:
//   SnapHeapHdr                       32 B
//   SnapHeapRow rows[n_records]       strictly ascending in pos
//   the records in row order, each heap_rec_bytes(len) bytes: the 32-B record
//   header and the Cmd, the bytes past the Cmd zero
// It carries every record a held log entry of the range refers to (ring, cold
// pages of either tier) or an entry of a Propose / Replicate the next round
// reads, once, when it is readable by collect_entry's rule (rbe_collect.h)
// against the host's heap head.
#pragma once
#include "rbe_collect.h"
#include "rbe_snap.h"

namespace rbe {

static constexpr u64 kSnapHeapMagic = 0x3150414548454252ull;  // "RBEHEAP1"
struct SnapHeapHdr {
  u64 magic, n_records, head, cap;
};
struct SnapHeapRow {
  u64 pos;
  u32 len, pad;
};
static_assert(sizeof(SnapHeapHdr) == 32 && sizeof(SnapHeapRow) == 16, "heap section layout");

// error word of a call
enum : u32 {
  CK_OVER = 1,      // totals past a buffer's capacity: nothing was written
  CK_CONFLICT = 2,  // two references to one position disagree on the length
  CK_CHAIN = 4,     // a chain changed between the count and the write
  CK_DIFF = 8       // compare mode: a record differs from the heap's bytes
};

// one page of the flat page list: page id `page` of replica r0 + `rep` holds
// page number pn and goes to byte `out` of the log section
struct CkPage {
  u64 pn, out;
  u32 page, rep;
};
static constexpr u64 kCkPageUnits = sizeof(SnapPage) / 16;  // 129
static_assert(sizeof(SnapPage) % 16 == 0 && sizeof(ReadReq) == 32 && sizeof(SnapLogRec) == 16,
              "the log section counts in 16-B units");

RBE_HD u64 ck_marker(const Planes& P, const Params& C, u64 r) {
  return C.snapshot_entries ? P.snp[r].marker : 0;
}
// pages of r's cold log and requests of its pooled readIndex queue.  A chain
// has at most `max_pages` pages (every page of both tiers), which bounds the
// walk over a broken one.
RBE_HD void ck_replica_count(const Planes& P, const Params& C, u64 r, u32* n_pages, u32* n_rq) {
  const ColdRef cr = P.cold[r];
  const u64 max_pages = (u64)C.pool_pages + C.host_pages;
  u32 n = 0;
  for (u32 p = cr.head; p && n < max_pages;) {
    n++;
    p = p == cr.tail ? 0u : P.pmeta[p].next;
  }
  *n_pages = n;
  *n_rq = P.core[r].rq_count == kRqExt ? rq_ext_load(P, C, r).n : 0u;
}
RBE_HD u64 ck_rec_units(u32 n_pages, u32 n_rq) { return 1 + n_pages * kCkPageUnits + 2ull * n_rq; }

// Replica r's record at byte `at` of the section `out`: its SnapLogRec, its
// pages into list[list_at ..] (their bytes are the page pass's), its pooled
// readIndex requests.  The counts are the ones the count pass saw; a chain of
// another length sets CK_CHAIN.
RBE_HD u32 ck_replica_write(const Planes& P, const Params& C, u64 r, u32 rep, u32 n_pages, u32 n_rq,
                            u8* out, u64 at, CkPage* list, u64 list_at) {
  SnapLogRec h = {};
  h.n_pages = n_pages;
  h.n_rq = n_rq;
  *(SnapLogRec*)(out + at) = h;
  at += sizeof(SnapLogRec);
  const ColdRef cr = P.cold[r];
  u32 n = 0;
  for (u32 p = cr.head; p && n < n_pages; n++) {
    const PoolMeta m = P.pmeta[p];
    CkPage x;
    x.pn = m.pn;
    x.out = at;
    x.page = p;
    x.rep = rep;
    list[list_at + n] = x;
    at += sizeof(SnapPage);
    p = p == cr.tail ? 0u : m.next;
  }
  u32 err = n == n_pages ? 0u : (u32)CK_CHAIN;
  if (n_rq) {
    const RqExt x = rq_ext_load(P, C, r);
    if (x.n != n_rq) return err | CK_CHAIN;
    u32 p = x.head, pos = x.off;
    for (u32 i = 0; i < n_rq; i++, pos++, at += sizeof(ReadReq)) {
      if (pos == kPageEnts) {
        p = P.pmeta[p].next;
        pos = 0;
      }
      *(ReadReq*)(out + at) = *(const ReadReq*)pool_ent(P, p, pos);
    }
  }
  return err;
}

// Whether entry x refers to a heap record a reader is served (collect_entry's
// rule with the host's head): its position and Cmd length
RBE_HD bool ck_heap_ref(const Params& C, u64 head, const Ent& x, u64* pos, u32* len) {
  if (!ent_heap(x.type) || !C.heap_bytes || x.hi > head || x.hi + C.heap_bytes < head) return false;
  const u64 at = x.hi % C.heap_bytes;
  if ((at & 15u) || at + heap_rec_bytes(x.len) > C.heap_bytes || x.hi + kHeapHdr + x.len > head)
    return false;
  *pos = x.hi;
  *len = x.len;
  return true;
}
// held indices: in pages above the compaction marker and at most last - ring,
// in the ring the window above that
RBE_HD bool ck_held_page(const Params& C, u64 marker, u64 last, u64 idx) {
  return idx > marker && last >= C.ring && idx <= last - C.ring;
}
// the index ring slot s of a log ending at `last` holds (0: none)
RBE_HD u64 ck_ring_index(const Params& C, u64 marker, u64 last, u32 s) {
  const u64 back = (last - s) & (u64)(C.ring - 1);
  if (back >= last) return 0;
  const u64 idx = last - back;
  return idx > marker ? idx : 0;
}
RBE_HD Ent ck_ring_ent(const Planes& P, const Params& C, u64 r, u32 s) {
  const u64 at = (u64)s * C.n_rep + r;
  const Body b = P.pay_ring[at];
  Ent e;
  e.term = P.term_ring[at];
  e.type = b.type;
  e.len = b.len;
  e.lo = b.lo;
  e.hi = b.hi;
  return e;
}
// The heap references of the entries of the Proposes and Replicates replica r
// sent in round `round` - 1 (the lists the next round reads, heap_low_group's):
// their number, written to pos / len unless null.  Lists and entries in the
// round spill heap are skipped: an export with any is refused before this.
RBE_HD u32 ck_msg_refs(const Planes& P, const Params& C, u64 r, u32 round, u64 head, u64* pos,
                       u32* len) {
  if (round == 0) return 0;
  const u32 par = (round - 1u) & 1u, k = (u32)(r % C.n);
  const CntRow row = P.cnt[par][r];
  u32 n = 0;
  for (u32 d = 0; d < C.n; d++) {
    const u32 w = row_word(row, d, k, round);
    if (w & kCntSpill) continue;
    const ListView lv = list_view(P, C, par, r * C.n + d, w);
    for (u32 i = 0; i < lv.n() && i < C.maxm; i++) {
      const Msg m = lv.at(i);
      if ((m.type != M_Propose && m.type != M_Replicate) || (m.pad0 & kMsgXEnt)) continue;
      if ((u64)m.ent_off + m.n_ent > C.ecap) continue;
      const Ent* es = &P.arena[par][r * C.ecap + m.ent_off];
      for (u32 j = 0; j < m.n_ent; j++) {
        u64 p;
        u32 l;
        if (!ck_heap_ref(C, head, es[j], &p, &l)) continue;
        if (pos) {
          pos[n] = p;
          len[n] = l;
        }
        n++;
      }
    }
  }
  return n;
}

// 16-B word w of the record {pos, len} as the section carries it: the heap's
// bytes, zero at and past the end of the Cmd
RBE_HD CeWord ck_mask_word(CeWord v, u32 len, u64 w) {
  const u64 valid = (u64)kHeapHdr + len, b = 16 * w;
  const u64 left = valid > b ? valid - b : 0;
  if (left < 8) v.a &= left ? (1ull << (8 * left)) - 1 : 0ull;
  if (left <= 8) v.b = 0;
  else if (left < 16) v.b &= (1ull << (8 * (left - 8))) - 1;
  return v;
}
RBE_HD CeWord ck_heap_word(const u8* heap, u64 cap, u64 pos, u32 len, u64 w) {
  const u64* p = (const u64*)(heap + pos % cap) + 2 * w;
  CeWord v;
  v.a = p[0];
  v.b = p[1];
  return ck_mask_word(v, len, w);
}
// the record of word j: the last s with off[s] <= j (off[0 .. n], ascending, in words)
RBE_HD u64 ck_slot_of(const u64* off, u64 n, u64 j) { return collect_slot_of(off, n, j); }

// A heap section of `avail` bytes checked whole against a heap of `cap` bytes
// before anything of a snapshot is imported: 0 and its size in *bytes, or -1
// (no room for what the header announces, a table not strictly ascending, an
// unaligned position, a record across the ring end, past the head or more than
// a lap below it, overlapping records, a size mismatch, another heap's cap).
// rec_off (n_records + 1 words, in 16-B units from the first record) is filled
// for the scatter / compare pass.
inline int ck_heap_check(u64 cap, const u8* sec, u64 avail, u64* bytes, u64* rec_off) {
  SnapHeapHdr h;
  if (avail < sizeof(h)) return -1;
  memcpy(&h, sec, sizeof(h));
  if (h.magic != kSnapHeapMagic || h.cap != cap || cap == 0) return -1;
  if (h.n_records > (avail - sizeof(h)) / sizeof(SnapHeapRow)) return -1;
  u64 units = 0, prev_end = 0;
  for (u64 i = 0; i < h.n_records; i++) {
    SnapHeapRow x;
    memcpy(&x, sec + sizeof(h) + i * sizeof(x), sizeof(x));
    const u64 rb = heap_rec_bytes(x.len), at = x.pos % cap;
    if (x.pad || (at & 15u) || at + rb > cap) return -1;
    if (x.pos > h.head || x.pos + kHeapHdr + x.len > h.head || x.pos + cap < h.head) return -1;
    if (i && x.pos < prev_end) return -1;  // not ascending, or overlapping
    prev_end = x.pos + rb;
    if (rec_off) rec_off[i] = units;
    units += rb / 16;
  }
  // (records within one lap that do not overlap in position do not overlap in the ring)
  if (h.n_records && prev_end > h.head + 15) return -1;
  if (rec_off) rec_off[h.n_records] = units;
  const u64 need = sizeof(h) + h.n_records * sizeof(SnapHeapRow) + units * 16;
  if (need != avail) return -1;
  *bytes = need;
  return 0;
}
// whether a heap section starts at `sec` (trailing bytes without the magic are ignored)
inline bool ck_heap_present(const u8* sec, u64 avail) {
  u64 m = 0;
  if (avail < sizeof(SnapHeapHdr)) return false;
  memcpy(&m, sec, sizeof(m));
  return m == kSnapHeapMagic;
}

}  // namespace rbe
