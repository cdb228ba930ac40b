// Batched read of log entries and their Cmds for many replicas
// (rbe_collect_entries / rbe_collect_entry_ranges, include/rbe.h): the
// per-range and per-entry logic, shared by the HIP kernels
// (rbe_collect_kernels.h) and the host build of the CPU test tier
// (tests/collect_cpu/collect_cpu.cpp).
//
// A call lists ranges — the EntriesToSave or CommittedEntries range of each
// replica's last Update, or (replica, lo, hi) triples the host names — and
// then reads every entry of every range: the ring, a cold page in HBM or a
// host-tier page (rbe_spill.h log_ent_at), plus the payload-heap record of an
// ET_HEAP entry.  A range or entry that cannot be served sets a bit of the
// call's error word; nothing is dereferenced for it.
#pragma once
#include "rbe_host.h"
#include "rbe_xchg.h"

namespace rbe {

// error word of a call (the host turns it into RBE_E_*)
enum : u32 {
  CE_BAD_RANGE = 1,  // ranges form: lo == 0, hi < lo, hi above the last index, replica out of range
  CE_MISSING = 2,    // log_ent_at failed: compacted, or below what a launch handed over
  CE_LAPPED = 4,     // the entry's heap record was overwritten by a later lap
  CE_OVER = 8        // totals past a buffer's capacity: nothing was written
};
// The block sums and their scan (launch_scan) count in 32 bits: a call lists
// fewer than 2^32 entries and, in 16-B units, less than 64 GiB of Cmd bytes.
// (2^32 records alone are 288 GiB.)  Sums past that would wrap; no pass writes
// past the capacities it was launched with even then.
inline int collect_rc(u32 err) {
  if (err & CE_BAD_RANGE) return RBE_E_INVALID;
  if (err & (CE_MISSING | CE_LAPPED)) return RBE_E_STATE;  // as rbe_get_entries: ErrCompacted
  return err ? RBE_E_STATE : RBE_OK;
}

// Where the ranges come from.  rep == null: the Update form, range i is the
// `which` range of replica first + i's Update of round `round` - 1; else the
// ranges form, range i is [lo[i], hi[i]] of rep[i].
struct CeSrc {
  u64 first, count;
  u32 round, which;
  const u64 *rep, *lo, *hi;
};

// Range i of a call: its replica, first index and entry count (0: not listed).
// An Update's range is taken by the rule update_view uses (Upd::round ==
// round - 1 and UF_RANGES); a replica another rank steps has no Update.
RBE_HD u64 collect_range(const Planes& P, const Params& C, const CeSrc& s, u64 i, u64* r,
                         u64* lo, u32* err) {
  if (s.rep) {
    const u64 x = s.rep[i], a = s.lo[i], b = s.hi[i];
    *r = x;
    *lo = a;
    if (x >= C.n_rep || a == 0 || b < a || b > P.core[x].last_index) {
      *err |= CE_BAD_RANGE;
      return 0;
    }
    return b - a + 1;
  }
  const u64 x = s.first + i;
  *r = x;
  *lo = 0;
  if (C.rep_world > 1 && owner_of<1>(C, x / C.n, (u32)(x % C.n)) != C.rep_rank) return 0;
  const Upd* u = P.upd + x;
  if (!(s.round > 0 && u->round == s.round - 1) || !(u->flags & UF_RANGES)) return 0;
  const bool save = (s.which & RBE_ENTRIES_TO_SAVE) != 0;
  const u64 a = save ? u->save_lo : u->apply_lo, b = save ? u->save_hi : u->apply_hi;
  if (a > b) return 0;
  *lo = a;
  // an Update never names an entry its log does not have; a record that does
  // is refused here, so the totals stay within what the logs hold
  if (a == 0 || b > P.core[x].last_index) {
    *err |= CE_MISSING;
    return 0;
  }
  return b - a + 1;
}

// What the entries pass keeps of one entry besides its record: the padded
// Cmd length (a multiple of 16, 0 for an empty Cmd) and where a heap Cmd's
// bytes start in the heap (kCeInline for a Cmd of at most 16 bytes: it is the
// record's cmd field, whether the entry is inline or a heap record)
static constexpr u64 kCeInline = ~0ull;
struct CeEnt {
  rbe_entry e;
  u64 src;
  u32 plen;
};
RBE_HD u32 ce_padded(u32 len) { return (len + 15u) & ~15u; }

// Entry idx of replica r as rbe_host.h entry_out fills it: Index, Term, type
// without ET_HEAP, cmd_len, the first 16 Cmd bytes, and the session fields
// from the heap record's header (records are 16-B aligned and never wrap).
// Every load happens before the caller's first store.  Returns CE_* bits; the
// record is zero then.  `heap_head` is the host's next free heap position
// (HostHeap::head), the one rbe_engine.hip read_heap judges a record by: the
// caller has put every record below it into `heap` (ce_collect uploads the
// ones still staged for the next step, e.g. those of an rbe_launch), and a
// record a lap below it has been overwritten (rbe_step.h heap_lapped's rule
// with that head).
//
// collect_ent_record is the Ent → record half, shared with the batched outbox
// (rbe_outbox.h), whose entries come from a sender's arena row or the round
// spill heap and carry the Index their message gives them.
RBE_HD u32 collect_ent_record(const Params& C, const u8* heap, u64 heap_head, const Ent& x, u64 idx,
                              CeEnt* out) {
  CeEnt o;
  o.e = rbe_entry{};
  o.src = kCeInline;
  o.plen = 0;
  *out = o;
  o.e.index = idx;
  o.e.term = x.term;
  o.e.type = ent_type(x.type);
  o.e.cmd_len = x.len;
  o.plen = ce_padded(x.len);
  u64 w0 = x.lo, w1 = x.hi;
  if (ent_heap(x.type)) {
    if (!heap || !C.heap_bytes || x.hi + C.heap_bytes < heap_head) return CE_LAPPED;
    const u64 at = x.hi % C.heap_bytes;
    if ((at & 15u) || at + kHeapHdr + o.plen > C.heap_bytes ||
        x.hi + kHeapHdr + x.len > heap_head)
      return CE_LAPPED;  // no such record
    const u64* rec = (const u64*)(heap + at);
    o.e.key = rec[0];
    o.e.client_id = rec[1];
    o.e.series_id = rec[2];
    o.e.responded_to = rec[3];
    w0 = w1 = 0;
    if (x.len) {  // the first min(len, 16) Cmd bytes, the rest zero
      w0 = rec[4];
      w1 = rec[5];
      if (x.len < 8) w0 &= (1ull << (8 * x.len)) - 1;
      if (x.len <= 8) w1 = 0;
      else if (x.len < 16) w1 &= (1ull << (8 * (x.len - 8))) - 1;
    }
    if (x.len > 16) o.src = at + kHeapHdr;  // (a shorter Cmd is whole in the record)
  }
  for (u32 b = 0; b < 8; b++) {
    o.e.cmd[b] = (u8)(w0 >> (8 * b));
    o.e.cmd[8 + b] = (u8)(w1 >> (8 * b));
  }
  *out = o;
  return 0;
}
RBE_HD u32 collect_entry(const Planes& P, const Params& C, const u8* heap, u64 heap_head, u64 r,
                         u64 idx, CeEnt* out) {
  Ent x;
  if (!log_ent_at(P, C, r, P.core[r].last_index, idx, &x)) {
    CeEnt o;
    o.e = rbe_entry{};
    o.src = kCeInline;
    o.plen = 0;
    *out = o;
    return CE_MISSING;
  }
  return collect_ent_record(C, heap, heap_head, x, idx, out);
}

// 16-B word w of an entry's padded Cmd: from the record's cmd field (inline)
// or the heap, with the bytes at and past cmd_len zero
struct CeWord {
  u64 a, b;
};
RBE_HD CeWord collect_cmd_word(const u8* heap, const rbe_entry& e, u64 src, u32 w) {
  CeWord v;
  if (src == kCeInline) {
    v.a = v.b = 0;
    for (u32 i = 0; i < 8; i++) {
      v.a |= (u64)e.cmd[i] << (8 * i);
      v.b |= (u64)e.cmd[8 + i] << (8 * i);
    }
  } else {
    const u64* p = (const u64*)(heap + src) + 2ull * w;
    v.a = p[0];
    v.b = p[1];
  }
  const u32 left = e.cmd_len - 16u * w;  // bytes of this word that belong to the Cmd (>= 1)
  if (left < 8) v.a &= (1ull << (8 * left)) - 1;
  if (left <= 8) v.b = 0;
  else if (left < 16) v.b &= (1ull << (8 * (left - 8))) - 1;
  return v;
}

// the slot of entry j in ent_off[0 .. n] (ascending, ent_off[n] > j): the
// last s with ent_off[s] <= j
RBE_HD u64 collect_slot_of(const u64* ent_off, u64 n, u64 j) {
  u64 lo = 0, hi = n;  // ent_off[lo] <= j < ent_off[hi]
  while (hi - lo > 1) {
    const u64 mid = (lo + hi) / 2;
    if (ent_off[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace rbe
