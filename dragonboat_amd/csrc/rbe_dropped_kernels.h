// Kernels of rbe_collect_dropped (rbe_dropped.h has the per-replica, per-entry
// and per-context logic).  Included by rbe_engine.hip after
// rbe_collect_kernels.h, whose Cmd passes and record store it reuses.
//
//   k_dr_count    a lane per replica of the range: (listed, dropped entries,
//                 dropped ReadIndex contexts) → block sums
//   launch_scan   block prefixes and the three totals
//   k_dr_write    a lane per replica: replica[], ent_off[], ri_off[] and a
//                 source descriptor per listed replica
//   k_dr_entries  a lane per ENTRY: a fixed grid strides over the entry total;
//                 each lane finds its replica by binary search in ent_off,
//                 reads the Ent from the list's block in the round spill heap
//                 and, for an ET_HEAP entry, its record's header and first Cmd
//                 bytes
//   k_dr_ctx      a lane per context: binary search in ri_off, the context
//                 from the P.dri plane list or its block in the spill heap
//   k_ce_cmd_sum, launch_scan, k_ce_cmd_off, k_ce_cmds   the Cmds, unchanged
// Every write pass checks the totals against the capacities it was launched
// with before it writes (CE_OVER).
#pragma once
#include "rbe_collect_kernels.h"
#include "rbe_dropped.h"

namespace rbe {

// capacities of the regions the passes fill: replicas listed, entries (the
// record array has room for the next multiple of kBlock), contexts
struct DrCaps {
  u64 n, ne, nri;
};

__global__ __launch_bounds__(kBlock) void k_dr_count(Planes P, Params C, DrArgs a, u32* bsum,
                                                     u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  u32 ne = 0, nri = 0, e = 0;
  if (i < a.count) dropped_view(P, C, a.first + i, a, &ne, &nri, nullptr, &e);
  if (e) atomicOr(err, e);
  u32 tf, te, tr;
  block_excl_scan((ne | nri) ? 1u : 0u, &tf);
  block_excl_scan(ne, &te);
  block_excl_scan(nri, &tr);
  if (threadIdx.x == 0) {
    bsum[3 * blockIdx.x] = tf;
    bsum[3 * blockIdx.x + 1] = te;
    bsum[3 * blockIdx.x + 2] = tr;
  }
}

__global__ __launch_bounds__(kBlock) void k_dr_write(Planes P, Params C, DrArgs a, const u64* pre,
                                                     DrOut o, DrCaps caps, u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u64 n_tot = pre[3 * gridDim.x], e_tot = pre[3 * gridDim.x + 1],
            r_tot = pre[3 * gridDim.x + 2];
  if (n_tot > caps.n || e_tot > caps.ne || r_tot > caps.nri) {
    if (i == 0) atomicOr(err, (u32)CE_OVER);
    return;
  }
  u32 ne = 0, nri = 0, e = 0;
  if (i < a.count) dropped_view(P, C, a.first + i, a, &ne, &nri, nullptr, &e);
  u32 t;
  const u64 at = pre[3 * blockIdx.x] + block_excl_scan((ne | nri) ? 1u : 0u, &t);
  const u64 be = pre[3 * blockIdx.x + 1] + block_excl_scan(ne, &t);
  const u64 br = pre[3 * blockIdx.x + 2] + block_excl_scan(nri, &t);
  if (i == 0) {  // the closing offsets
    o.ent_off[n_tot] = e_tot;
    o.ri_off[n_tot] = r_tot;
  }
  if (!(ne | nri)) return;
  // (the count pass reported what this view finds wrong with a block)
  dropped_write(P, C, a.first + i, a, at, be, br, o, &e);
}

// tot = {replicas listed, entries, contexts} on the device.  A block takes
// kBlock consecutive entries per trip and stores them as k_ce_entries does.
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void k_dr_entries(Planes P, Params C, const u8* heap,
                                                       u64 heap_head, const u64* tot,
                                                       const u64* ent_off, const DrSrc* dsrc,
                                                       rbe_entry* ents, u32* plen, u64* src,
                                                       DrCaps caps, u32* err) {
  __shared__ uint4 s_rec[STAGE ? kBlock * sizeof(rbe_entry) / 16 : 1];
  const u64 n = tot[0], ne = tot[1], nri = tot[2];
  if (n > caps.n || ne > caps.ne || nri > caps.nri) return;  // (k_dr_write reported it)
  for (u64 base = (u64)blockIdx.x * kBlock; base < ne; base += (u64)gridDim.x * kBlock) {
    const u64 j = base + threadIdx.x;
    CeEnt x;
    x.e = rbe_entry{};
    x.src = kCeInline;
    x.plen = 0;
    if (j < ne) {
      const u32 e = dropped_entry(P, C, heap, heap_head, ent_off, dsrc, n, j, &x);
      if (e) atomicOr(err, e);
      plen[j] = x.plen;
      src[j] = x.src;
    }
    ce_store_records<STAGE>(s_rec, x.e, ents, base, ne);
  }
}

__global__ __launch_bounds__(kBlock) void k_dr_ctx(Planes P, const u64* tot, const u64* ri_off,
                                                   const DrSrc* dsrc, rbe_system_ctx* ctx,
                                                   DrCaps caps) {
  const u64 n = tot[0], ne = tot[1], nri = tot[2];
  if (n > caps.n || ne > caps.ne || nri > caps.nri) return;
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < nri; j += (u64)gridDim.x * kBlock)
    ctx[j] = dropped_ctx(P, ri_off, dsrc, n, j);
}

}  // namespace rbe
