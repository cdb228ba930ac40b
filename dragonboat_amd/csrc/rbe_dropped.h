// Batched dropped lists (rbe_collect_dropped, include/rbe.h): the
// Update.DroppedEntries and Update.DroppedReadIndexes of many replicas' last
// step, what a node completes as dropped (node.go:925-941).  The per-replica,
// per-entry and per-context logic, shared by the HIP kernels
// (rbe_dropped_kernels.h) and the host build of the CPU test tier
// (tests/dropped_cpu/dropped_cpu.cpp).
//
// A replica contributes the lists of its Update by the rule collect_range uses
// (Upd::round == round - 1 and UF_RANGES; a replica another rank steps has
// none).  Its dropped entries are the Ent records its P.dent row names in the
// round spill heap (cfg.drop_lists, rbe_spill.h dent_put_o), its dropped
// ReadIndex contexts the P.dri plane list or, past dri_cap, the block its slot
// 0 names.  Everything read out of the spill heap is bounds-checked first: a
// row or header whose block does not lie inside the heap sets CE_MISSING in
// the call's error word and nothing of it is dereferenced.
#pragma once
#include "rbe_collect.h"

namespace rbe {

struct DrArgs {
  u64 first, count;  // the replica range
  u32 round;         // the round that reads the lists (the engine's round)
};

// Where a listed replica's lists are: the entries' first granule in the round
// spill heap of parity `par`; the contexts' first granule there (ri_spill), or
// their first index in P.dri
struct DrSrc {
  u64 ent_at, ri_at;
  u32 par, ri_spill;
};

// Replica r's lists: the counts and, with `s`, where they are.  Nothing of a
// block that fails its check is counted.
RBE_HD void dropped_view(const Planes& P, const Params& C, u64 r, const DrArgs& a, u32* ne,
                         u32* nri, DrSrc* s, u32* err) {
  *ne = *nri = 0;
  const u64 g = r / C.n;
  const u32 k = (u32)(r % C.n);
  if (a.round == 0 || !owns_replica(C, g, k)) return;
  const Upd u = P.upd[r];
  if (u.round != a.round - 1 || !(u.flags & UF_RANGES)) return;
  const u32 par = u.round & 1u;
  DrSrc x;
  x.ent_at = x.ri_at = 0;
  x.par = par;
  x.ri_spill = 0;
  u32 n_ent = 0, n_ri = u.n_drop_ri;
  if (n_ri <= C.dri_cap) {
    x.ri_at = r * C.dri_cap;
  } else {  // the list moved to the spill heap: slot 0 = {granule, capacity}
    const DropRI h = P.dri[r * C.dri_cap];
    if (h.low > C.spill_units || (u64)n_ri * (sizeof(DropRI) / 16) > C.spill_units - h.low ||
        h.high < n_ri) {
      *err |= CE_MISSING;
      n_ri = 0;
    }
    x.ri_at = h.low;
    x.ri_spill = 1;
  }
  if (u.n_drop_ent && P.dent) {
    const DentRow d = P.dent[r];
    // (a row of another round is stale: an imported or relaunched replica's,
    // zeroed, lists nothing until its next step)
    if (d.round == u.round && d.n) {
      if (d.granule > C.spill_units || d.n > d.cap ||
          (u64)d.cap * (sizeof(Ent) / 16) > C.spill_units - d.granule) {
        *err |= CE_MISSING;
      } else {
        n_ent = d.n;
        x.ent_at = d.granule;
      }
    }
  }
  *ne = n_ent;
  *nri = n_ri;
  if (s) *s = x;
}

// the regions the write pass fills
struct DrOut {
  u64* replica;  // n
  u64* ent_off;  // n + 1
  u64* ri_off;   // n + 1
  DrSrc* src;    // n
};
// lane r of the write pass: listed replica number `at`, whose entries start at
// `be` and whose contexts start at `br`
RBE_HD void dropped_write(const Planes& P, const Params& C, u64 r, const DrArgs& a, u64 at, u64 be,
                          u64 br, const DrOut& o, u32* err) {
  u32 ne, nri;
  DrSrc s;
  dropped_view(P, C, r, a, &ne, &nri, &s, err);
  o.replica[at] = r;
  o.ent_off[at] = be;
  o.ri_off[at] = br;
  o.src[at] = s;
}

// Entry j of the call: its replica by binary search in ent_off[0 .. n], the
// Ent from the list's block, and the record half of rbe_collect.h with Index 0
// (a dropped proposal carries none).  Every load happens before the caller's
// first store.
RBE_HD u32 dropped_entry(const Planes& P, const Params& C, const u8* heap, u64 heap_head,
                         const u64* ent_off, const DrSrc* src, u64 n, u64 j, CeEnt* out) {
  const u64 sl = collect_slot_of(ent_off, n, j);
  const DrSrc s = src[sl];
  const Ent x = spill_at<const Ent>(P, s.par & 1u, s.ent_at)[j - ent_off[sl]];
  return collect_ent_record(C, heap, heap_head, x, 0, out);
}

// context j of the call
RBE_HD rbe_system_ctx dropped_ctx(const Planes& P, const u64* ri_off, const DrSrc* src, u64 n,
                                  u64 j) {
  const u64 sl = collect_slot_of(ri_off, n, j);
  const DrSrc s = src[sl];
  const u64 q = j - ri_off[sl];
  const DropRI x = s.ri_spill ? spill_at<const DropRI>(P, s.par & 1u, s.ri_at)[q] : P.dri[s.ri_at + q];
  rbe_system_ctx c;
  c.low = x.low;
  c.high = x.high;
  return c;
}

}  // namespace rbe
