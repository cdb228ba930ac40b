// Kernels of rbe_collect_outbox (rbe_outbox.h has the per-replica, per-message
// and per-entry logic).  Included by rbe_engine.hip after rbe_collect_kernels.h,
// whose Cmd passes and record store it reuses.
//
//   k_ob_count    a lane per replica of the range: (listed, messages wanted,
//                 entries they hand over) → block sums
//   launch_scan   block prefixes and the three totals
//   k_ob_msgs     a lane per replica: replica[], msg_off[], the rbe_message
//                 records, ent_off[] and a source descriptor per message
//   k_ob_entries  a lane per ENTRY (one per Replicate in a steady round, a
//                 whole catch-up in one message after an isolation): a fixed
//                 grid strides over the entry total; each lane finds its
//                 message by binary search in ent_off, reads the Ent from the
//                 sender's arena row or the round spill heap and, for an
//                 ET_HEAP entry, its record's header and first Cmd bytes
//   k_ce_cmd_sum, launch_scan, k_ce_cmd_off, k_ce_cmds   the Cmds, unchanged
// Every write pass checks the totals against the capacities it was launched
// with before it writes (CE_OVER).
#pragma once
#include "rbe_collect_kernels.h"
#include "rbe_outbox.h"

namespace rbe {

// capacities of the regions the passes fill: senders listed, messages, entries
// (the record array has room for the next multiple of kBlock)
struct ObCaps {
  u64 n, nm, ne;
};

__global__ __launch_bounds__(kBlock) void k_ob_count(Planes P, Params C, ObArgs a, u32* bsum,
                                                     u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  u32 nm = 0, ne = 0, e = 0;
  if (i < a.count) outbox_count(P, C, a.first + i, a, &nm, &ne, &e);
  if (e) atomicOr(err, e);
  u32 tf, tm, te;
  block_excl_scan(nm ? 1u : 0u, &tf);
  block_excl_scan(nm, &tm);
  block_excl_scan(ne, &te);
  if (threadIdx.x == 0) {
    bsum[3 * blockIdx.x] = tf;
    bsum[3 * blockIdx.x + 1] = tm;
    bsum[3 * blockIdx.x + 2] = te;
  }
}

__global__ __launch_bounds__(kBlock) void k_ob_msgs(Planes P, Params C, ObArgs a, const u64* pre,
                                                    ObOut o, ObCaps caps, u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u64 n_tot = pre[3 * gridDim.x], m_tot = pre[3 * gridDim.x + 1],
            e_tot = pre[3 * gridDim.x + 2];
  if (n_tot > caps.n || m_tot > caps.nm || e_tot > caps.ne) {
    if (i == 0) atomicOr(err, (u32)CE_OVER);
    return;
  }
  u32 nm = 0, ne = 0, e = 0;
  if (i < a.count) outbox_count(P, C, a.first + i, a, &nm, &ne, &e);
  u32 t;
  const u64 at = pre[3 * blockIdx.x] + block_excl_scan(nm ? 1u : 0u, &t);
  const u64 bm = pre[3 * blockIdx.x + 1] + block_excl_scan(nm, &t);
  const u64 be = pre[3 * blockIdx.x + 2] + block_excl_scan(ne, &t);
  if (i == 0) {  // the closing offsets
    o.msg_off[n_tot] = m_tot;
    o.ent_off[m_tot] = e_tot;
  }
  if (!nm) return;
  // (the count pass reported what this walk finds wrong with a spilled block)
  outbox_write(P, C, a.first + i, a, at, bm, be, o, &e);
}

// tot = {senders listed, messages, entries} on the device.  A block takes
// kBlock consecutive entries per trip and stores them as k_ce_entries does.
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void k_ob_entries(Planes P, Params C, const u8* heap,
                                                       u64 heap_head, const u64* tot,
                                                       const u64* ent_off, const ObSrc* msrc,
                                                       rbe_entry* ents, u32* plen, u64* src,
                                                       ObCaps caps, u32* err) {
  __shared__ uint4 s_rec[STAGE ? kBlock * sizeof(rbe_entry) / 16 : 1];
  const u64 n = tot[0], nm = tot[1], ne = tot[2];
  if (n > caps.n || nm > caps.nm || ne > caps.ne) return;  // (k_ob_msgs reported it)
  for (u64 base = (u64)blockIdx.x * kBlock; base < ne; base += (u64)gridDim.x * kBlock) {
    const u64 j = base + threadIdx.x;
    CeEnt x;
    x.e = rbe_entry{};
    x.src = kCeInline;
    x.plen = 0;
    if (j < ne) {
      const u32 e = outbox_entry(P, C, heap, heap_head, ent_off, msrc, nm, j, &x);
      if (e) atomicOr(err, e);
      plen[j] = x.plen;
      src[j] = x.src;
    }
    ce_store_records<STAGE>(s_rec, x.e, ents, base, ne);
  }
}

}  // namespace rbe
