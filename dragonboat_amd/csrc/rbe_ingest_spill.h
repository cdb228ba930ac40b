// rbe_ingest_spill.h — the receiving side of the transport past maxm / ecap.
//
// rbe_wire_ingest (rbe_ingest.h ingest_check / ingest_sender) and
// rbe_push_messages (rbe_xchg.h messages_to_records) answer RBE_E_NOMEM for a
// (sender, destination) list of more than maxm messages and for a sender with
// more than ecap entries, although Peer.Handle takes any such message
// (peer.go:186-198; a catch-up Replicate is sized by MaxEntrySize alone,
// raft.go:709-740).  ingest_sender_spill here is ingest_sender's spilling form;
// with it go ingest_check's `spill` argument and messages_to_records's
// reservation (XSpillRes, rbe_xchg.h).  The same checks and the same plane
// layout for a batch that fits, and for one that does not, the layout a local
// sender's step leaves in the round spill heap
// (rbe_spill.h): outbox_relocate's block and M_SpillRef record for a list,
// Lane::set_ents's kMsgXEnt reference for a message's entries.  Every reader
// of the inbox (list_view, msg_ents, msg_nent, triage's saturated counts,
// host_list, the export's refusal) then works unchanged.
//
// Granules come from this engine's own share of the heap of the last round's
// parity (spill_share, share * rep_rank + at), after whatever that round's
// local senders took: base = SpillCtl::used when the call starts, plus an
// exclusive scan of each sender run's need in sorted order; within a run its
// spilled lists by ascending destination, then the spilled messages' entries.
// No atomics, so the host build leaves the bytes a device pass would.  The
// caller checks the total against share - used before anything is written
// (RBE_E_NOMEM, SpillCtl::oom untouched: no round ran out), and raises used /
// peak after the write; the next round's reset (spill_clear_next) is what gives
// the granules back, after that round has read them.
//
// All RBE_HD.  The CPU test tier runs them (tests/ingest_cpu), and so does the
// HIP engine: the bodies of its kernels are the lane functions at the end of
// this file (ingest_walk_lane, ingest_share_gate, ingest_share_commit), which
// tests/ingest_dev_cpu runs as loops under the sanitizers (DESIGN.md §10
// "Inbound spill").
#pragma once
#include "rbe_ingest.h"

namespace rbe {

// Entry e of an inbound message (its Cmd at cb) as the arena / spill heap
// holds it; an entry with a long Cmd or session fields leaves its record
// {Key, ClientID, SeriesID, RespondedTo, Cmd} (HostHeap::put_record) at heap
// position *hpos, which then moves past it.
RBE_HD Ent ingest_entry(const rbe_entry& e, const u8* cb, u8* heap, u64 heap_cap, u64* hpos) {
  Ent y;
  y.term = e.term;
  y.type = e.type & ET_TYPE_MASK;
  y.len = e.cmd_len;
  if (entry_needs_heap(e)) {
    const u64 meta[4] = {e.key, e.client_id, e.series_id, e.responded_to};
    u8* rec = heap + *hpos % heap_cap;
    for (int q = 0; q < 4; q++) ((u64*)rec)[q] = meta[q];
    for (u32 b = 0; b < e.cmd_len; b++) rec[kHeapHdr + b] = cb[b];
    y.type |= ET_HEAP;
    y.lo = entry_fingerprint(meta, cb, e.cmd_len);
    y.hi = *hpos;
    *hpos += heap_rec_bytes(e.cmd_len);
  } else {
    u64 lo = 0, hi = 0;
    for (u32 b = 0; b < e.cmd_len && b < 16; b++) {
      if (b < 8) lo |= (u64)cb[b] << (8 * b);
      else hi |= (u64)cb[b] << (8 * (b - 8));
    }
    y.lo = lo;
    y.hi = hi;
  }
  return y;
}

// One sender's run [p0, p1) of the sorted messages (every key of the run has
// the same sender replica sr = key / N; keys ascending, stream order within a
// key), in two loops.
//
// The first loop counts: the messages of each list, and the entries that find
// no room in the sender's arena row.  A list of more than maxm messages moves
// whole into the round spill heap, as outbox_relocate leaves a local sender's
// (rbe_spill.h): a block of na + nb Msg, Replicates in stream order from the
// front, the rest from the back, plane slot 0 the M_SpillRef record, the count
// word saturated.  A message whose entries would run past ecap keeps them all
// in the spill heap (kMsgXEnt; Lane::arena_put's rule: the arena offset does
// not advance, so later small messages still use the arena).  *need (when
// given) gets the granules the run takes: its spilled lists by ascending
// destination, then the spilled messages' entries in run order.  That is the
// whole of the checking pass (WRITE = false).
//
// The second loop (WRITE = true) builds the lists exactly as
// messages_to_records does and writes them into parity `par`: each message at
// its slot, its entries at the sender's next arena offsets, the spilled parts
// from granule sbase on (the caller's exclusive scan of the runs' needs over
// this engine's share of the heap), heap records at base + hscan[p] (16-B
// aligned, the batch's region does not cross the end of the ring), and the
// sender's outbox header stamped `round` with the count words of the lists
// named (0 for the others).
template <int N, bool WRITE>
RBE_HD u32 ingest_sender_spill(const Planes& P, const Params& C, u32 par, u32 round, const u64* skey,
                         const u32* sidx, u64 p0, u64 p1, const rbe_message* msgs,
                         const rbe_entry* ents, const u64* ent0, const u64* cmd0, const u8* cmd,
                               u8* heap, u64 heap_cap, u64 base, const u64* hscan, u64* need,
                               u64 sbase) {
  const u64 sr = skey[p0] / N;
  u64 lg = 0, xg = 0;  // granules of the spilled lists / entries
  {
    u64 lk = ~0ull, cnt = 0, used = 0;
    for (u64 p = p0; p < p1; p++) {
      const rbe_message& m = msgs[sidx[p]];
      if (skey[p] != lk) {
        if (cnt > C.maxm) lg += cnt * (sizeof(Msg) / 16);
        lk = skey[p];
        cnt = 0;
      }
      if (m.type == M_Quiesce) continue;
      cnt++;
      const u64 ne = m.n_entries;
      if (used + ne > C.ecap) xg += ne * (sizeof(Ent) / 16);
      else used += ne;
    }
    if (cnt > C.maxm) lg += cnt * (sizeof(Msg) / 16);
  }
  if (need) *need = lg + xg;
  if (!WRITE) return 0;
  u32 words[N];
  for (int d = 0; d < N; d++) words[d] = 0;
  u32 used = 0;
  u64 lcur = sbase, xcur = sbase + lg;  // next granule of the lists / the entries
  u64 lk = ~0ull;
  Msg* blk = nullptr;  // the current list's block when it is spilled
  u32 cap = 0, ia = 0, ib = 0;
  for (u64 p = p0; p < p1; p++) {
    const u64 key = skey[p];
    const u32 d = (u32)(key % N);
    const u32 j = sidx[p];
    const rbe_message& m = msgs[j];
    u32& w = words[d];
    if (lg && key != lk) {  // a new list of a run with spilled lists: is it one?
      lk = key;
      blk = nullptr;
      u32 a = 0, b = 0;
      for (u64 q = p; q < p1 && skey[q] == key; q++) {
        const u32 t = msgs[sidx[q]].type;
        if (t != M_Quiesce) (t == M_Replicate ? a : b)++;
      }
      if (a + b > C.maxm) {
        cap = a + b;
        ia = ib = 0;
        blk = spill_at<Msg>(P, par, lcur);
        Msg h = {};
        h.type = M_SpillRef;
        h.hint = lcur;
        h.pad1 = cap;
        h.log_index = a;
        h.commit = b;
        P.msgs[par][key * (u64)C.maxm] = h;
        lcur += (u64)cap * (sizeof(Msg) / 16);
        w |= kCntSpilled;
      }
    }
    if (m.type == M_Quiesce) {
      w |= kCntQ;
      continue;
    }
    Msg* dst;
    if (blk) {
      dst = &blk[m.type == M_Replicate ? ia++ : cap - 1u - ib++];
    } else {
      const u32 na = w & 0x7Fu, nb = (w >> 7) & 0x7Fu;
      u32 slot;
      if (m.type == M_Replicate) {
        slot = na;
        w += 1u;
      } else {
        slot = C.maxm - 1u - nb;
        w += 1u << 7;
      }
      dst = &P.msgs[par][key * (u64)C.maxm + slot];
    }
    const u32 ne = m.n_entries;
    Msg x = mk_msg(m.type, (u32)m.to);
    x.from = (u8)m.from;
    x.reject = (u8)(m.reject ? 1 : 0);
    x.term = m.term;
    x.log_term = m.log_term;
    x.log_index = m.log_index;
    x.commit = m.commit;
    x.hint = m.hint;
    x.hint_high = m.hint_high;
    if (ne) {
      Ent* ed;
      x.n_ent = (u16)(ne > 0xFFFFu ? 0xFFFFu : ne);
      if ((u64)used + ne > C.ecap) {  // (Lane::set_ents)
        ed = spill_at<Ent>(P, par, xcur);
        x.pad0 |= kMsgXEnt;
        x.pad1 = ne;
        x.ent_off = (u32)xcur;
        xcur += (u64)ne * (sizeof(Ent) / 16);
      } else {
        ed = &P.arena[par][sr * C.ecap + used];
        x.ent_off = used;
        used += ne;
      }
      u64 hpos = base + hscan[p];
      const u8* cb = cmd + cmd0[j];
      for (u32 i = 0; i < ne; i++) {
        const rbe_entry& e = ents[ent0[j] + i];
        ed[i] = ingest_entry(e, cb, heap, heap_cap, &hpos);
        cb += e.cmd_len;
      }
    }
    *dst = x;
  }
  CntRow row;
  row.stamp = round;
  for (int q = 0; q < 6; q++) row.w[q] = 0;
  for (int d = 0; d < N; d++)
    if ((u32)d != (u32)(sr % N)) row.w[cnt_widx((u32)d, (u32)(sr % N))] = (u16)words[d];
  P.cnt[par][sr] = row;
  P.gwake[sr / N] = GW_AWAKE;  // a message wakes the destination's group
  return 0;
}

// ------------------------------------------------ the device pipeline's lanes
// rbe_wire_ingest (rbe_engine.hip) runs, after the sort and the heap-byte scan:
//   ingest_walk_lane<N, false>   lane per sorted position: the run's granule
//                                need at its start, 0 everywhere else
//   exclusive scan of the needs  (k_scan_*), the total behind them
//   ingest_share_gate            one lane: the share check, the batch's first
//                                granule and its total into `ctl`
//   ingest_walk_lane<N, true>    lane per sorted position: the run's lists
//   ingest_share_commit          one lane: used += total, peak raised
// The __global__ functions compute the lane index and call these, so the host
// build runs the same index arithmetic.

// the share check's refusal, ORed into the word the writing walk is gated on
// (beside ING_INVALID / ING_NOMEM, rbe_ingest.h)
enum : u32 { ING_SHARE = 4u };
// what the gate leaves for the writing walk, the commit and the host
enum : u32 { IC_BASE = 0, IC_TOTAL = 1, IC_USED = 2, IC_WORDS = 4 };

// Sorted position p of nm: the granules its sender's run needs (need[p]; 0
// when p starts no run), or with WRITE the run's lists, its spilled parts from
// granule ctl[IC_BASE] + need[p] on (need scanned by then).  With WRITE a
// non-zero gate word means a check before this one failed: nothing is written.
template <int N, bool WRITE>
RBE_HD void ingest_walk_lane(const Planes& P, const Params& C, u32 par, u32 round, const u64* skey,
                             const u32* sidx, u64 p, u64 nm, const rbe_message* msgs,
                             const rbe_entry* ents, const u64* ent0, const u64* cmd0, const u8* cmd,
                             u8* heap, u64 heap_cap, u64 base, const u64* hs, u64* need,
                             const u64* ctl, const u32* gate) {
  if (p >= nm) return;
  const bool start = ingest_run_start(C, skey, p);
  if (!WRITE) need[p] = 0;
  if (!start) return;
  if (WRITE && gate && (gate[0] | gate[1])) return;
  const u64 q = ingest_run_end(C, skey, p, nm);
  if (WRITE)
    ingest_sender_spill<N, true>(P, C, par, round, skey, sidx, p, q, msgs, ents, ent0, cmd0, cmd,
                                 heap, heap_cap, base, hs, nullptr, ctl[IC_BASE] + need[p]);
  else
    ingest_sender_spill<N, false>(P, C, par, round, skey, sidx, p, q, msgs, ents, ent0, cmd0, cmd,
                                  nullptr, heap_cap, 0, hs, &need[p], 0);
}

// The share check (one lane, before the writing walk): `total` granules
// against what this engine's share of parity `par` has left.  ctl gets the
// batch's first granule (share * rep_rank + used), the total and `used`; a
// total past the free part ORs ING_SHARE into *gate.  Reads SpillCtl only.
RBE_HD void ingest_share_gate(const Params& C, const SpillCtl* s, u32 par, u64 total, u64* ctl,
                              u32* gate) {
  const u64 share = spill_share(C), used = s->used[par];
  const u64 avail = used < share ? share - used : 0;
  ctl[IC_BASE] = (C.rep_world > 1 ? share * C.rep_rank : 0) + used;
  ctl[IC_TOTAL] = total;
  ctl[IC_USED] = used;
  if (total > avail) *gate |= ING_SHARE;
}

// The commit (one lane, after the writing walk, which reads the base): the
// granules are taken.  Plain stores; nothing else runs between two rounds.
RBE_HD void ingest_share_commit(SpillCtl* s, u32 par, u64 total, const u32* gate) {
  if (gate && (gate[0] | gate[1])) return;
  s->used[par] += total;
  if (total && s->peak[par] < s->used[par]) s->peak[par] = s->used[par];
}

}  // namespace rbe
