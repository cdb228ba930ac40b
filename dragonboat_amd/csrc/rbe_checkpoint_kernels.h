// Kernels of rbe_export_groups_ex and of the heap section's import
// (rbe_checkpoint.h has the per-replica, per-page and per-record logic).
// Included by rbe_engine.hip after block_excl_scan / launch_scan.
//
//   k_ck_count     a lane per replica walks its chain once: (pages, 16-B units
//                  of its record) → block sums
//   launch_scan    block prefixes and the totals
//   k_ck_replicas  a lane per replica: its SnapLogRec and pooled readIndex
//                  requests at its offset, its pages into the flat page list
//   k_ck_pages     a wave per page, a lane per 32-B entry: SnapPage {pn, 0,
//                  e[64]} at the page's offset, from HBM or the mapped host tier
// and, with RBE_EXPORT_HEAP, over the gathered section (so a host-tier page
// crosses the link once):
//   k_ck_refs      COUNT, then EMIT: a lane per page entry, per replica ring
//                  slot and per replica's message lists; (pos, len) of the
//                  readable ET_HEAP entries at held indices, appended a wave at
//                  a time
//   dev_sort_pairs by pos
//   k_ck_heads     run heads (equal pos, another len: CK_CONFLICT) → block sums
//                  of (records, 16-B units)
//   launch_scan
//   k_ck_table     the section's header, its rows and the record offsets
//   k_ck_records   the records, 16 B per access; each lane finds its record by
//                  binary search.  The same kernel scatters an imported
//                  section into the heap or compares it with the heap.
// Every write pass checks the totals against the capacities it was launched
// with before it writes.
#pragma once
#include "rbe_checkpoint.h"

namespace rbe {

struct CkCaps {
  u64 pages, units;  // page list entries, 16-B units of the log section
  u64 refs;          // reference pairs
};

__global__ __launch_bounds__(kBlock) void k_ck_count(Planes P, Params C, u64 r0, u64 nr,
                                                     u32* bsum) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  u32 np = 0, nq = 0, un = 0;
  if (i < nr) {
    ck_replica_count(P, C, r0 + i, &np, &nq);
    un = (u32)ck_rec_units(np, nq);
  }
  u32 tp, tu;
  block_excl_scan(np, &tp);
  block_excl_scan(un, &tu);
  if (threadIdx.x == 0) {
    bsum[2 * blockIdx.x] = tp;
    bsum[2 * blockIdx.x + 1] = tu;
  }
}

__global__ __launch_bounds__(kBlock) void k_ck_replicas(Planes P, Params C, u64 r0, u64 nr,
                                                        const u64* pre, u8* out, CkPage* list,
                                                        CkCaps caps, u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  if (pre[2 * gridDim.x] > caps.pages || pre[2 * gridDim.x + 1] > caps.units) {
    if (i == 0) atomicOr(err, (u32)CK_OVER);
    return;
  }
  u32 np = 0, nq = 0, un = 0;
  if (i < nr) {
    ck_replica_count(P, C, r0 + i, &np, &nq);
    un = (u32)ck_rec_units(np, nq);
  }
  u32 t;
  const u64 pa = pre[2 * blockIdx.x] + block_excl_scan(np, &t);
  const u64 ua = pre[2 * blockIdx.x + 1] + block_excl_scan(un, &t);
  if (i >= nr) return;
  // (the chains do not change under an export; one that did is caught here)
  if (pa + np > caps.pages || ua + un > caps.units) {
    atomicOr(err, (u32)CK_CHAIN);
    return;
  }
  const u32 e = ck_replica_write(P, C, r0 + i, (u32)i, np, nq, out, ua * 16, list, pa);
  if (e) atomicOr(err, e);
}

// A wave per page; tot[0] = pages listed.  Lane j moves entry j as two 16-B
// words, so a wave's loads and stores are one contiguous 2 KiB run each.
static constexpr unsigned kCkPageGrid = 2048;
__global__ __launch_bounds__(kBlock) void k_ck_pages(Planes P, const u64* tot, const CkPage* list,
                                                     u8* out, CkCaps caps) {
  const u64 n = tot[0];
  if (n > caps.pages || tot[1] > caps.units) return;  // (k_ck_replicas reported it)
  const u32 lane = threadIdx.x & 63u;
  const u64 w0 = ((u64)blockIdx.x * kBlock + threadIdx.x) >> 6, nw = (u64)gridDim.x * (kBlock >> 6);
  for (u64 q = w0; q < n; q += nw) {
    const CkPage x = list[q];
    if (x.out + sizeof(SnapPage) > caps.units * 16) continue;  // (never past the capacity)
    const uint4* s = (const uint4*)pool_ent(P, x.page, lane);
    const uint4 a = s[0], b = s[1];
    uint4* d = (uint4*)(out + x.out);
    if (lane == 0) d[0] = make_uint4((u32)x.pn, (u32)(x.pn >> 32), 0u, 0u);
    d[1 + 2 * lane] = a;
    d[2 + 2 * lane] = b;
  }
}

// The heap references of the range.  Item space: [0, 64 * pages) the entries
// of the gathered pages, then nr * ring ring slots, then nr replicas' message
// lists.  EMIT appends (pos, len) at `cnt` a wave at a time (the order is the
// sort's to fix); COUNT only adds to it.
static constexpr unsigned kCkRefGrid = 4096;
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_ck_refs(Planes P, Params C, u64 r0, u64 nr, u32 round,
                                                    u64 head, const u64* tot, const CkPage* list,
                                                    const u8* sec, u64* keys, u32* vals,
                                                    unsigned long long* cnt, CkCaps caps, u32* err) {
  const u64 np = tot[0];
  if (np > caps.pages || tot[1] > caps.units) return;
  const u32 lane = threadIdx.x & 63u;
  const u64 n_pg = np * kPageEnts, n_ring = nr * C.ring, n_all = n_pg + n_ring + nr;
  for (u64 base = ((u64)blockIdx.x * kBlock + (threadIdx.x & ~63u)); base < n_all;
       base += (u64)gridDim.x * kBlock) {
    const u64 j = base + lane;
    u64 pos = 0;
    u32 len = 0, mine = 0;
    u64 mr = ~0ull;  // a message-list lane's replica
    if (j < n_pg) {
      const CkPage x = list[j >> 6];
      const u64 r = r0 + x.rep;
      const Ent e = ((const SnapPage*)(sec + x.out))->e[j & 63u];
      if (ck_held_page(C, ck_marker(P, C, r), P.core[r].last_index, x.pn * kPageEnts + (j & 63u)) &&
          ck_heap_ref(C, head, e, &pos, &len))
        mine = 1;
    } else if (j < n_pg + n_ring) {
      const u64 q = j - n_pg, r = r0 + q % nr;  // (consecutive lanes, consecutive replicas)
      const u32 s = (u32)(q / nr);
      if (ck_ring_index(C, ck_marker(P, C, r), P.core[r].last_index, s) &&
          ck_heap_ref(C, head, ck_ring_ent(P, C, r, s), &pos, &len))
        mine = 1;
    } else if (j < n_all) {
      mr = r0 + (j - n_pg - n_ring);
      mine = ck_msg_refs(P, C, mr, round, head, nullptr, nullptr);
    }
    // wave-aggregated reservation: one atomic per wave
    u32 x = mine;
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) {
      const u32 t = __shfl_up(x, o, 64);
      if (lane >= o) x += t;
    }
    const u32 wave_tot = __shfl(x, 63, 64);
    if (!wave_tot) continue;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(cnt, (unsigned long long)wave_tot);
    at = __shfl(at, 0, 64) + (x - mine);
    if (!EMIT || !mine) continue;
    if (at + mine > caps.refs) {
      atomicOr(err, (u32)CK_OVER);
      continue;
    }
    if (mr != ~0ull) {
      ck_msg_refs(P, C, mr, round, head, keys + at, vals + at);
    } else {
      keys[at] = pos;
      vals[at] = len;
    }
  }
}

// run heads of the sorted pairs → block sums of (records, 16-B units)
__global__ __launch_bounds__(kBlock) void k_ck_heads(const u64* keys, const u32* vals, u64 n,
                                                     u32* bsum, u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  u32 hd = 0, un = 0;
  if (i < n) {
    hd = i == 0 || keys[i] != keys[i - 1];
    if (!hd && vals[i] != vals[i - 1]) atomicOr(err, (u32)CK_CONFLICT);
    un = hd ? (u32)(heap_rec_bytes(vals[i]) >> 4) : 0u;
  }
  u32 th, tu;
  block_excl_scan(hd, &th);
  block_excl_scan(un, &tu);
  if (threadIdx.x == 0) {
    bsum[2 * blockIdx.x] = th;
    bsum[2 * blockIdx.x + 1] = tu;
  }
}
// the section's header and rows (at `sec`), the record offsets in 16-B units
__global__ __launch_bounds__(kBlock) void k_ck_table(const u64* keys, const u32* vals, u64 n,
                                                     const u64* pre, u64 head, u64 cap, u8* sec,
                                                     u64* rec_off, u64 row_cap, u32* err) {
  const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
  const u64 n_rec = pre[2 * gridDim.x];
  if (n_rec > row_cap) {
    if (i == 0) atomicOr(err, (u32)CK_OVER);
    return;
  }
  u32 hd = 0, un = 0;
  if (i < n) {
    hd = i == 0 || keys[i] != keys[i - 1];
    un = hd ? (u32)(heap_rec_bytes(vals[i]) >> 4) : 0u;
  }
  u32 t;
  const u64 at = pre[2 * blockIdx.x] + block_excl_scan(hd, &t);
  const u64 ua = pre[2 * blockIdx.x + 1] + block_excl_scan(un, &t);
  if (i == 0) {
    SnapHeapHdr h;
    h.magic = kSnapHeapMagic;
    h.n_records = n_rec;
    h.head = head;
    h.cap = cap;
    *(SnapHeapHdr*)sec = h;
    rec_off[n_rec] = pre[2 * gridDim.x + 1];
  }
  if (!hd) return;
  SnapHeapRow x;
  x.pos = keys[i];
  x.len = vals[i];
  x.pad = 0;
  ((SnapHeapRow*)(sec + sizeof(SnapHeapHdr)))[at] = x;
  rec_off[at] = ua;
}

// The records of a heap section, a lane per 16-B word.  GATHER: heap → section
// (export).  SCATTER: section → heap (resume).  COMPARE: CK_DIFF when a word of
// the section is not the heap's (hand-off).  rows / rec_off describe n_rec
// records of rec_off[n_rec] words, which is at most `word_cap`.
enum : int { CK_GATHER = 0, CK_SCATTER = 1, CK_COMPARE = 2 };
static constexpr unsigned kCkRecGrid = 4096;
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_ck_records(u8* heap, u64 cap, const SnapHeapRow* rows,
                                                       const u64* rec_off, u64 n_rec, u8* recs,
                                                       u64 word_cap, u32* err) {
  const u64 nw = rec_off[n_rec];
  if (nw > word_cap || n_rec == 0) return;
  for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < nw; j += (u64)gridDim.x * kBlock) {
    const u64 s = ck_slot_of(rec_off, n_rec, j), w = j - rec_off[s];
    const SnapHeapRow x = rows[s];
    const u64 at = x.pos % cap;
    if (at + 16 * w + 16 > cap) continue;  // (never past the ring: ck_heap_ref / ck_heap_check)
    uint4* sw = (uint4*)recs + j;
    if (MODE == CK_SCATTER) {
      *((uint4*)(heap + at) + w) = *sw;
      continue;
    }
    const CeWord v = ck_heap_word(heap, cap, x.pos, x.len, w);
    const uint4 hv = make_uint4((u32)v.a, (u32)(v.a >> 32), (u32)v.b, (u32)(v.b >> 32));
    if (MODE == CK_GATHER) {
      *sw = hv;
    } else {
      const uint4 c = *sw;
      if (c.x != hv.x || c.y != hv.y || c.z != hv.z || c.w != hv.w) atomicOr(err, (u32)CK_DIFF);
    }
  }
}

}  // namespace rbe
