// Kernels of rbe_collect_entries / rbe_collect_entry_ranges (rbe_collect.h has
// the per-range and per-entry logic).  Included by rbe_engine.hip after its
// block scan (block_excl_scan) and block-sum scan kernels (launch_scan).
//
//   k_ce_count    a lane per range: (listed, entry count) → block sums
//   launch_scan   block prefixes and the totals {ranges listed, entries}
//   k_ce_ranges   a lane per range: replica[], ent_off[], the first index
//   k_ce_entries  a lane per ENTRY (a range is 1 entry in the steady state and
//                 hundreds on a catch-up or a replay): a fixed grid whose
//                 blocks stride over the entry total; each lane finds its
//                 range by binary search in ent_off, reads the entry and, for
//                 an ET_HEAP entry, its record's header and first Cmd bytes
//   k_ce_cmd_sum  padded Cmd lengths (16-B units) → block sums
//   launch_scan   block prefixes and the Cmd total
//   k_ce_cmd_off  cmd_off[]
//   k_ce_cmds     the Cmd bytes, 16 B per access
// Every write pass checks the totals against the capacities it was launched
// with before it writes (as k_cs_write does with CsCaps).
#pragma once
#include "rbe_collect.h"

namespace rbe {

// capacities of the regions the passes fill: ranges listed, entries (the
// record array has room for the next multiple of kBlock), Cmd bytes
struct CeCaps {
  u64 n, ne, cmd;
};

__global__ __launch_bounds__(kBlock) void k_ce_count(Planes P, Params C, CeSrc s, u32* bsum,
                                                     u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  u64 r, lo, cnt = 0;
  u32 e = 0;
  if (i < s.count) cnt = collect_range(P, C, s, i, &r, &lo, &e);
  if (e) atomicOr(err, e);
  u32 tf, te;
  block_excl_scan(cnt ? 1u : 0u, &tf);
  block_excl_scan((u32)cnt, &te);
  if (threadIdx.x == 0) {
    bsum[2 * blockIdx.x] = tf;
    bsum[2 * blockIdx.x + 1] = te;
  }
}

__global__ __launch_bounds__(kBlock) void k_ce_ranges(Planes P, Params C, CeSrc s, const u64* pre,
                                                      u64* rep, u64* ent_off, u64* lo_at,
                                                      CeCaps caps, u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u64 n_tot = pre[2 * gridDim.x], e_tot = pre[2 * gridDim.x + 1];
  if (n_tot > caps.n || e_tot > caps.ne) {
    if (i == 0) atomicOr(err, (u32)CE_OVER);
    return;
  }
  u64 r = 0, lo = 0, cnt = 0;
  u32 e = 0;
  if (i < s.count) cnt = collect_range(P, C, s, i, &r, &lo, &e);
  u32 t;
  const u64 at = pre[2 * blockIdx.x] + block_excl_scan(cnt ? 1u : 0u, &t);
  const u64 eo = pre[2 * blockIdx.x + 1] + block_excl_scan((u32)cnt, &t);
  if (i == 0) ent_off[n_tot] = e_tot;  // the closing offset
  if (!cnt) return;
  rep[at] = r;
  ent_off[at] = eo;
  lo_at[at] = lo;
}

// The entries pass.  tot = {ranges listed, entries} on the device.  A block
// takes kBlock consecutive entries per trip, so its 72-B records are one
// contiguous, 16-B aligned run of the record array.  STAGE: the block stages
// them in LDS and writes the run as 16-B stores (72 B is not a multiple of a
// 32-B sector); else every lane writes its own record as nine 8-B stores.
static constexpr unsigned kCeGrid = 1024;
static_assert(sizeof(rbe_entry) == 72, "k_ce_entries stores a record as nine 8-B words");
// One trip's records of a block into the record array: lane t holds record
// base + t (zero past the end).  STAGE: through s_rec as 16-B stores of the
// contiguous run; else nine 8-B stores per lane.  Every lane of the block calls it.
template <bool STAGE>
__device__ __forceinline__ void ce_store_records(uint4* s_rec, const rbe_entry& rec,
                                                 rbe_entry* ents, u64 base, u64 ne) {
  const u64 j = base + threadIdx.x;
  const u64* w = (const u64*)&rec;
  if (STAGE) {
    u64* mine = (u64*)s_rec + 9u * threadIdx.x;
#pragma unroll
    for (int q = 0; q < 9; q++) mine[q] = w[q];
    __syncthreads();
    // the run's bytes rounded up to 16: the records of lanes past the end are
    // zero and the record array has room for a whole block
    const u64 left = ne - base;
    const u32 nv = left < kBlock ? (u32)left : (u32)kBlock;
    const u32 words = (nv * (u32)sizeof(rbe_entry) + 15u) / 16u;
    uint4* dst = (uint4*)(ents + base);
    for (u32 q = threadIdx.x; q < words; q += kBlock) dst[q] = s_rec[q];
    __syncthreads();  // before the next trip overwrites the stage
  } else if (j < ne) {
    u64* dst = (u64*)(ents + j);
#pragma unroll
    for (int q = 0; q < 9; q++) dst[q] = w[q];
  }
}
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void k_ce_entries(Planes P, Params C, const u8* heap,
                                                       u64 heap_head, const u64* tot, const u64* rep,
                                                       const u64* ent_off, const u64* lo_at,
                                                       rbe_entry* ents, u32* plen, u64* src,
                                                       CeCaps caps, u32* err) {
  __shared__ uint4 s_rec[STAGE ? kBlock * sizeof(rbe_entry) / 16 : 1];
  const u64 n = tot[0], ne = tot[1];
  if (n > caps.n || ne > caps.ne) return;  // (k_ce_ranges reported it)
  for (u64 base = (u64)blockIdx.x * kBlock; base < ne; base += (u64)gridDim.x * kBlock) {
    const u64 j = base + threadIdx.x;
    CeEnt x;
    x.e = rbe_entry{};
    x.src = kCeInline;
    x.plen = 0;
    if (j < ne) {
      const u64 sl = collect_slot_of(ent_off, n, j);
      const u32 e = collect_entry(P, C, heap, heap_head, rep[sl], lo_at[sl] + (j - ent_off[sl]), &x);
      if (e) atomicOr(err, e);
      plen[j] = x.plen;
      src[j] = x.src;
    }
    ce_store_records<STAGE>(s_rec, x.e, ents, base, ne);
  }
}

// Cmd offsets: an exclusive scan of the padded lengths, in 16-B units
__global__ __launch_bounds__(kBlock) void k_ce_cmd_sum(const u32* plen, u64 ne, u32* bsum) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u32 v = i < ne ? plen[i] >> 4 : 0u;
  u32 t;
  block_excl_scan(v, &t);
  if (threadIdx.x == 0) {
    bsum[2 * blockIdx.x] = t;
    bsum[2 * blockIdx.x + 1] = 0;
  }
}
__global__ __launch_bounds__(kBlock) void k_ce_cmd_off(const u32* plen, u64 ne, const u64* pre,
                                                       u64* cmd_off) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u32 v = i < ne ? plen[i] >> 4 : 0u;
  u32 t;
  const u64 at = pre[2 * blockIdx.x] + block_excl_scan(v, &t);
  if (i < ne) cmd_off[i] = at * 16;
  if (i == 0) cmd_off[ne] = pre[2 * gridDim.x] * 16;
}

// The Cmd bytes.  A wave takes 64 consecutive entries per trip.  A Cmd of up
// to kCeLaneWords 16-B words is copied by the entry's own lane (an inline Cmd
// is one word, out of its record); a longer one, always a heap Cmd, by the
// whole wave, lane l taking words l, l + 64, ...: source (record + 32) and
// destination (cmd_off, a multiple of 16) are both 16-B aligned.  Up to four
// words are loaded before the first of them is stored.
static constexpr unsigned kCeCmdGrid = 1024;
static constexpr u32 kCeLaneWords = 4;
__device__ __forceinline__ uint4 ce_word(const u8* heap, const rbe_entry& e, u64 src, u32 w) {
  const CeWord v = collect_cmd_word(heap, e, src, w);
  return make_uint4((u32)v.a, (u32)(v.a >> 32), (u32)v.b, (u32)(v.b >> 32));
}
__global__ __launch_bounds__(kBlock) void k_ce_cmds(const u8* heap, u64 ne, const rbe_entry* ents,
                                                    const u64* src, const u64* cmd_off, u8* cmds,
                                                    CeCaps caps) {
  if (ne > caps.ne || cmd_off[ne] > caps.cmd) return;
  const u32 lane = threadIdx.x & 63u;
  const u64 w0 = ((u64)blockIdx.x * kBlock + threadIdx.x) >> 6, nw = (u64)gridDim.x * (kBlock >> 6);
  for (u64 base = w0 * 64; base < ne; base += nw * 64) {
    const u64 j = base + lane;
    rbe_entry e = rbe_entry{};
    u64 s = kCeInline, off = 0;
    u32 words = 0;
    if (j < ne) {
      e = ents[j];
      s = src[j];
      off = cmd_off[j];
      words = ce_padded(e.cmd_len) >> 4;
      if (s == kCeInline && words > 1) words = 1;  // (an inline Cmd is at most 16 bytes)
      if (off + 16ull * words > caps.cmd) words = 0;    // (never past the capacity)
    }
    if (words && words <= kCeLaneWords) {
      uint4 v[kCeLaneWords];
#pragma unroll
      for (u32 q = 0; q < kCeLaneWords; q++)
        if (q < words) v[q] = ce_word(heap, e, s, q);
#pragma unroll
      for (u32 q = 0; q < kCeLaneWords; q++)
        if (q < words) ((uint4*)(cmds + off))[q] = v[q];
    }
    unsigned long long big = __ballot(words > kCeLaneWords);
    while (big) {
      const int b = __ffsll(big) - 1;
      big &= big - 1;
      const u64 bs = __shfl(s, b, 64), bo = __shfl(off, b, 64);
      const u32 bw = __shfl(words, b, 64), bl = __shfl(e.cmd_len, b, 64);
      rbe_entry h = rbe_entry{};  // (collect_cmd_word reads the length alone for a heap Cmd)
      h.cmd_len = bl;
      uint4* dst = (uint4*)(cmds + bo);
      for (u32 q = lane; q < bw; q += 256) {
        uint4 v[4];
#pragma unroll
        for (u32 k = 0; k < 4; k++)
          if (q + 64 * k < bw) v[k] = ce_word(heap, h, bs, q + 64 * k);
#pragma unroll
        for (u32 k = 0; k < 4; k++)
          if (q + 64 * k < bw) dst[q + 64 * k] = v[k];
      }
    }
  }
}

}  // namespace rbe
