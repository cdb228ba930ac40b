// rbe_launch.h — the cold part of an rbe_launch, a page at a time.
//
// A launch hands a replica its whole LogDB; what lies below the ring goes into
// the replica's cold log (rbe_spill.h).  The host knows every launched
// replica's cold range before anything runs, so the pages are planned there
// (launch_plan) and built in passes over pages instead of one cold_put per
// entry on the replica's lane:
//
//   release  a lane per replica   the old chain and readIndex pages go back
//   alloc    a lane per page      an id per page into ids[] (0: both tiers full)
//   fill     a wave per page      64 slots and the PoolMeta record
//   install  a lane per replica   after relaunch_replica over the ring rows:
//                                 the chain's ColdRef, or the undo
//
// The per-page and per-slot logic is here, shared by the HIP kernels
// (rbe_launch_kernels.h) and the host build of the CPU test tier
// (tests/launch_cpu/launch_cpu.cpp).  Placement follows the import's rule
// (rbe_snap.h snap_log_rebuild): with a host tier every page but a replica's
// last goes to a host page (an HBM page when the tier is full); the last page
// is the chain's tail and always an HBM page (ColdRef, rbe_types.h).
#pragma once
#include "rbe_host.h"
#include "rbe_step.h"

namespace rbe {

// One launched replica's cold range (parallel to the batch's launch records):
// entries [first, last] of its LogDB lie below the ring, in `pages` pages; `row`
// is the row of entry `first` in the batch's terms / bodies arrays.
struct LaunchPg {
  u64 first, last, row;
  u32 pages;
  u32 cc;  // a ConfigChange among them (MB_CC_IN_LOG)
};

// The plan of a batch: pg[i] for each replica and the exclusive prefix
// page_off[0 .. n] of the page counts.  Returns the page total.
inline u64 launch_plan(const Params& C, u64 n, const rbe_launch_state* st, const Body* bodies,
                       std::vector<LaunchPg>& pg, std::vector<u32>& page_off) {
  pg.assign(n, LaunchPg{0, 0, 0, 0, 0});
  page_off.assign(n + 1, 0);
  u64 row = 0, total = 0;
  for (u64 i = 0; i < n; i++) {
    const rbe_launch_state& x = st[i];
    LaunchPg& p = pg[i];
    if (x.n_entries > C.ring) {
      p.first = x.last_index - x.n_entries + 1;
      p.last = x.last_index - C.ring;
      p.row = row;
      p.pages = (u32)(p.last / kPageEnts - p.first / kPageEnts + 1);
      if (C.membership)
        for (u64 q = 0; q < x.n_entries - C.ring; q++)
          if (ent_type(bodies[row + q].type) == E_ConfigChange) p.cc = 1;
    }
    row += x.n_entries;
    total += p.pages;
    page_off[i + 1] = (u32)total;  // (page ids are u32: a total past that cannot be placed)
  }
  return total;
}

// The replica of the batch that owns page p (< page_off[n]): the last i with
// page_off[i] <= p, so among equal neighbours (replicas without a cold page)
// the one whose range is not empty
RBE_HD u64 launch_page_owner(const u32* page_off, u64 n, u32 p) {
  u64 lo = 0, hi = n;  // page_off[lo] <= p < page_off[hi]
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    if (page_off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// An HBM page between two rounds, from a kernel that frees nothing: either
// free stack (so what the release pass just pushed is usable again), then the
// bump counter and the free-id ring as pool_alloc.  The sticky oom bit is set
// only when all of them are empty.
template <class PL>
RBE_HD u32 launch_stack_pop(const PL& P, u32* fh) {
#if defined(__HIP_DEVICE_COMPILE__)
  u32 h = __hip_atomic_load(fh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (h) {
    const u32 nx = P.pmeta[h].next;
    const u32 o = atomicCAS(fh, h, nx);
    if (o == h) break;
    h = o;
  }
#else
  const u32 h = *fh;
  if (h) *fh = P.pmeta[h].next;
#endif
  return h;
}
template <class PL, class PA>
RBE_HD u32 launch_hbm_alloc(const PL& P, const PA& C) {
  SpillCtl* s = P.sctl;
  u32 h = launch_stack_pop(P, &s->free_head[0]);
  if (!h) h = launch_stack_pop(P, &s->free_head[1]);
  if (!h) {
    const u32 p = sp_atomic_add_u32(&s->bump, 1u);
    if (p < C.pool_pages) {
      h = p;
    } else {
      const u32 i = p - C.pool_pages;
      if (s->hpool_first && i < s->fa_n) h = s->fa[(s->fa_base + i) & s->fa_mask];
    }
  }
  if (h) sp_atomic_add_u32(&s->live, 1u);
  else sp_atomic_or_u32(&s->oom, 1u);
  return h;
}
// The page id of a replica's page: `tail` = the replica's last page
template <class PL, class PA>
RBE_HD u32 launch_page_alloc(const PL& P, const PA& C, bool tail) {
  u32 p = P.sctl->hpool_first && !tail ? host_alloc(P, C) : 0u;
  if (!p) p = launch_hbm_alloc(P, C);
  return p;
}

// Whether every page of a replica (ids[0, pages)) got an id; the lanes of a
// wave share the loop on the device (stride 64 from `lane`)
RBE_HD bool launch_ids_ok(const u32* ids, u32 pages, u32 lane = 0, u32 stride = 1) {
  bool ok = true;
  for (u32 j = lane; j < pages; j += stride) ok = ok && ids[j] != 0;
  return ok;
}

// Slot `slot` of page number pn of the replica planned as x: the entry from
// the batch's rows when its index lies in the cold range, else zero (a page's
// bytes do not depend on what the page held before)
RBE_HD Ent launch_slot(const LaunchPg& x, const u64* terms, const Body* bodies, u64 pn, u32 slot) {
  const u64 idx = pn * kPageEnts + slot;
  Ent e;
  e.term = e.lo = e.hi = 0;
  e.type = e.len = 0;
  if (idx >= x.first && idx <= x.last) {
    const u64 row = x.row + (idx - x.first);
    const Body b = bodies[row];
    e.term = terms[row];
    e.type = b.type;
    e.len = b.len;
    e.lo = b.lo;
    e.hi = b.hi;
  }
  return e;
}

// The chain record of the replica's j-th page (ids = the replica's ids)
RBE_HD PoolMeta launch_meta(const LaunchPg& x, const u32* ids, u32 j) {
  PoolMeta m;
  m.pn = x.first / kPageEnts + j;
  m.prev = j ? ids[j - 1] : 0u;
  m.next = j + 1 < x.pages ? ids[j + 1] : 0u;
  return m;
}

// After relaunch_replica over the ring rows (its own release found nothing and
// left the chain empty): the chain the passes built, or, when a page of it
// found no room in either tier, the pages it did get go back (parity `par`;
// nothing pops in that kernel), the chain stays empty and the replica alone
// takes F_NOMEM
RBE_HD void launch_install(const Planes& P, u64 r, const LaunchPg& x, const u32* ids, u32 par) {
  if (!x.pages) return;
  if (launch_ids_ok(ids, x.pages)) {
    ColdRef cr;
    cr.head = ids[0];
    cr.tail = ids[x.pages - 1];
    cr.tail_pn = x.last / kPageEnts;
    P.cold[r] = cr;
    if (x.cc) P.core[r].mflags |= MB_CC_IN_LOG;
    return;
  }
  for (u32 j = 0; j < x.pages; j++)
    if (ids[j]) pool_free(P, par, ids[j]);
  P.upd[r].fault |= F_NOMEM;
  P.hot[r].flags |= HF_FAULTED;
}

}  // namespace rbe
