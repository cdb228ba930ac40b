// rbe_launch_kernels.h — the passes of an rbe_launch whose LogDBs reach below
// the ring (rbe_launch.h), on the engine stream between two rounds.  Included
// only by rbe_engine.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rbe_kernels.h"
#include "rbe_launch.h"

namespace rbe {

// rbe_launch: the record of one relaunched replica (rbe_step.h relaunch_replica)
struct LaunchRec {
  u64 replica, term, vote, commit, last, off;  // off: first row in the terms/bodies arrays
  u32 n, removed;                              // removed: rbe_launch_state::removed
  u64 marker, marker_term, ss_index, ss_term;  // compacted LogDB (rbe_launch_state)
};

// Release: a lane per launched replica.  The old incarnation's cold log (host
// pages too) and pooled readIndex queue go back before any page is taken; the
// kernel allocates nothing.
__global__ __launch_bounds__(kBlock) void k_launch_release(Planes P, Params C,
                                                           const LaunchRec* rec, u64 n, u32 par) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) spill_replica_release(P, C, rec[i].replica, par);
}

// Alloc: a fixed grid whose lanes stride over the batch's pages.  The kernel
// frees nothing and runs between rounds, so it pops both free stacks.
static constexpr unsigned kLaunchAllocGrid = 1024;
__global__ __launch_bounds__(kBlock) void k_launch_alloc(Planes P, Params C, const u32* page_off,
                                                         u64 n, u32* ids) {
  const u32 total = page_off[n];
  for (u64 p = (u64)blockIdx.x * kBlock + threadIdx.x; p < total;
       p += (u64)gridDim.x * kBlock) {
    const u64 i = launch_page_owner(page_off, n, (u32)p);
    ids[p] = launch_page_alloc(P, C, (u32)p + 1u == page_off[i + 1]);
  }
}

// Fill: a fixed grid whose waves stride over the pages, lane l owns slot l
// (32 B as two 16-B stores: 2 KiB a wave, coalesced, to HBM or over the host
// link); lane 0 then writes the page's chain record.  Every load comes before
// the first store.  A replica that missed a page is skipped whole.
static constexpr unsigned kLaunchFillGrid = 2048;
__global__ __launch_bounds__(kBlock) void k_launch_fill(Planes P, const LaunchPg* pg,
                                                        const u32* page_off, u64 n,
                                                        const u64* terms, const Body* bodies,
                                                        const u32* ids) {
  const u32 total = page_off[n];
  const u32 lane = threadIdx.x & 63u;
  const u32 w0 = (blockIdx.x * kBlock + threadIdx.x) >> 6, nw = gridDim.x * (kBlock >> 6);
  for (u32 p = w0; p < total; p += nw) {
    const u64 i = launch_page_owner(page_off, n, p);
    const LaunchPg x = pg[i];
    const u32 j = p - page_off[i];
    const u32* rid = ids + page_off[i];
    const bool ok = launch_ids_ok(rid, x.pages, lane, 64u);
    if (__any(!ok)) continue;  // (wave-uniform: p and i are)
    const u32 id = rid[j];
    const Ent e = launch_slot(x, terms, bodies, x.first / kPageEnts + j, lane);
    const PoolMeta m = launch_meta(x, rid, j);
    uint4* dst = (uint4*)pool_ent(P, id, lane);
    uint4 a, b;
    a.x = (u32)e.term;
    a.y = (u32)(e.term >> 32);
    a.z = e.type;
    a.w = e.len;
    b.x = (u32)e.lo;
    b.y = (u32)(e.lo >> 32);
    b.z = (u32)e.hi;
    b.w = (u32)(e.hi >> 32);
    dst[0] = a;
    dst[1] = b;
    if (lane == 0) P.pmeta[id] = m;
  }
}

// Relaunch: one lane per replica.  Without a plan (pg null: no launched
// replica has an entry below its ring) the whole LogDB goes through
// relaunch_replica; with one, its ring rows only, and the lane then installs
// the chain the passes built (rbe_launch.h launch_install).
template <int N>
__global__ __launch_bounds__(kBlock) void k_relaunch(Planes P, Params C, const LaunchRec* rec,
                                                     u64 n, const u64* terms, const Body* bodies,
                                                     u32 ppar, u32 tclk, const LaunchPg* pg,
                                                     const u32* page_off, const u32* ids) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const LaunchRec x = rec[i];
  const u32 nr = pg && x.n > C.ring ? C.ring : x.n;
  const u64 off = x.off + (x.n - nr);
  relaunch_replica<N>(P, C, x.replica, x.term, x.vote, x.commit, x.last, nr, terms + off,
                      bodies + off, ppar, tclk, x.marker, x.marker_term, x.ss_index, x.ss_term,
                      x.removed);
  if (pg) launch_install(P, x.replica, pg[i], ids + page_off[i], ppar ^ 1u);
  P.gwake[x.replica / N] = GW_AWAKE;
}

}  // namespace rbe
