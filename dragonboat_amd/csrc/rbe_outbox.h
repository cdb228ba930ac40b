// Batched outbox (rbe_collect_outbox, include/rbe.h): the last round's
// messages of many sender replicas WITH their entries and Cmds, what a
// transport needs of Update.Messages.  The per-replica, per-message and
// per-entry logic, shared by the HIP kernels (rbe_outbox_kernels.h) and the
// host build of the CPU test tier (tests/outbox_cpu/outbox_cpu.cpp).
//
// Per sender the messages and their order are those of rbe_xchg.h
// outbox_messages (rbe_get_outbox): destinations in ascending slot, per
// destination the Quiesce notice, the Replicate messages (the list's A part),
// the rest (its B part); a Replicate's and a forwarded Propose's entries
// follow, from the sender's arena row or the round spill heap (msg_ents).
// Everything read out of the spill heap is bounds-checked first: a block or an
// entry run that does not lie inside the heap sets CE_MISSING in the call's
// error word and nothing of it is dereferenced.
#pragma once
#include "rbe_collect.h"

namespace rbe {

struct ObArgs {
  u64 first, count;  // the sender range
  u32 round;         // the round that reads the outboxes (the engine's round)
  u32 remote;        // RBE_COLLECT_REMOTE_MSGS
  int32_t dst_rank;  // -1, or the only rank whose replicas are destinations
};

// rbe_collect_outbox's dst_rank: -1, or another rank of a replica-mode engine
inline bool outbox_rank_ok(const Params& C, int32_t dst_rank) {
  if (dst_rank == -1) return true;
  return C.rep_world > 1 && dst_rank >= 0 && (u32)dst_rank < C.rep_world &&
         (u32)dst_rank != C.rep_rank;
}
// whether sender group g's messages to destination slot d are returned
RBE_HD bool outbox_dst_wanted(const Params& C, u64 g, u32 d, const ObArgs& a) {
  if (C.rep_world <= 1) return !a.remote;  // (dst_rank is -1: the call checked)
  const u32 owner = owner_of<1>(C, g, d);  // rep_world for a padding group
  if (a.remote && (owner >= C.rep_world || owner == C.rep_rank)) return false;
  return a.dst_rank < 0 || owner == (u32)a.dst_rank;
}

// list_view with the block of a spilled list checked against the heap and the
// counts against the list's capacity; an empty view and CE_MISSING otherwise
RBE_HD ListView outbox_list(const Planes& P, const Params& C, u32 par, u64 li, u32 w, u32* err) {
  ListView v;
  v.base = &P.msgs[par][li * C.maxm];
  v.cap = C.maxm;
  v.na = v.nb = 0;
  if (!(w & 0x7FFFu)) return v;
  if (!(w & kCntSpill)) {
    v.na = w & 0x7Fu;
    v.nb = (w >> 7) & 0x7Fu;
  } else {
    const Msg h = v.base[0];
    const u64 na = h.log_index, nb = h.commit, cap = h.pad1;
    if (h.type != M_SpillRef || h.hint > C.spill_units ||
        cap * (sizeof(Msg) / 16) > C.spill_units - h.hint || na > cap || nb > cap) {
      *err |= CE_MISSING;
      return v;
    }
    v.base = spill_at<const Msg>(P, par, h.hint);
    v.cap = (u32)cap;
    v.na = (u32)na;
    v.nb = (u32)nb;
  }
  if ((u64)v.na + v.nb > v.cap) {
    *err |= CE_MISSING;
    v.na = v.nb = 0;
  }
  return v;
}

// the entries message m hands over: those outbox_messages walks (an arena
// run is cut at the row's end; a spilled run must lie inside the heap)
RBE_HD u32 outbox_msg_nent(const Params& C, const Msg& m, u32* err) {
  if (m.type != M_Replicate && m.type != M_Propose) return 0;
  const u32 n = msg_nent(m);
  if (m.pad0 & kMsgXEnt) {
    if (m.ent_off > C.spill_units || (u64)n * (sizeof(Ent) / 16) > C.spill_units - m.ent_off) {
      *err |= CE_MISSING;
      return 0;
    }
    return n;
  }
  if (m.ent_off >= C.ecap) return 0;
  const u32 room = C.ecap - m.ent_off;
  return n < room ? n : room;
}

// Sender r's wanted messages in transport order: f(m, type, to, n_ent) per
// message, m the list's record (the Quiesce notice: an empty one), n_ent the
// entries it hands over.  Nothing for a replica another rank steps.
template <class F>
RBE_HD void outbox_walk(const Planes& P, const Params& C, u64 r, const ObArgs& a, u32* err, F&& f) {
  const u32 N = C.n, par = (a.round - 1u) & 1u;
  const u64 g = r / N;
  const u32 k = (u32)(r % N);
  if (a.round == 0 || !owns_replica(C, g, k)) return;
  const CntRow row = P.cnt[par][r];
  for (u32 d = 0; d < N; d++) {
    const u32 pc = row_word(row, d, k, a.round);
    if (!pc || !outbox_dst_wanted(C, g, d, a)) continue;
    if (pc & kCntQ) f(mk_msg(M_Quiesce, d + 1), (u32)M_Quiesce, d + 1, 0u);
    const ListView lv = outbox_list(P, C, par, r * N + d, pc, err);
    for (u32 i = 0; i < lv.n(); i++) {
      const Msg m = lv.at(i);
      f(m, (u32)m.type, d + 1, outbox_msg_nent(C, m, err));
    }
  }
}

// lane r of the count pass: messages wanted and the entries they hand over
RBE_HD void outbox_count(const Planes& P, const Params& C, u64 r, const ObArgs& a, u32* nm,
                         u32* ne, u32* err) {
  u32 m = 0, e = 0;
  outbox_walk(P, C, r, a, err, [&](const Msg&, u32, u32, u32 n) {
    m++;
    e += n;
  });
  *nm = m;
  *ne = e;
}

// the raftpb form of a message as outbox_messages' emit fills it
RBE_HD void outbox_msg_out(const Planes& P, const Params& C, u64 g, u32 k, const Msg& m, u32 type,
                           u32 to, rbe_message& o) {
  Msg x = m;
  x.type = (u8)type;
  x.to = (u8)to;
  x.from = (u8)(k + 1);
  if (!(type == M_Replicate || type == M_Propose)) x.n_ent = 0;
  o = rbe_message{};
  msg_out(x, cid_of(C, g), P.node_ids, C.n, g, o);
}

// Where a message's entries are: `at` is entry 0's index in the arena plane of
// the round's parity (sender row * ecap + ent_off), or kObSpill | its granule
// in the round spill heap; entry j's Index is base + j for a Replicate (base =
// LogIndex + 1) and 0 for a forwarded Propose.
static constexpr u64 kObSpill = 1ull << 63;
struct ObSrc {
  u64 at, base;
  u32 rep, par;  // a Replicate's; the round's parity
};

// the regions the messages pass fills
struct ObOut {
  u64* replica;       // n
  u64* msg_off;       // n + 1
  rbe_message* msgs;  // n_messages
  u64* ent_off;       // n_messages + 1
  ObSrc* src;         // n_messages
};
// lane r of the messages pass: listed sender number `at`, whose messages start
// at `bm` and whose entries start at `be`
RBE_HD void outbox_write(const Planes& P, const Params& C, u64 r, const ObArgs& a, u64 at, u64 bm,
                         u64 be, const ObOut& o, u32* err) {
  const u64 g = r / C.n;
  const u32 k = (u32)(r % C.n), par = (a.round - 1u) & 1u;
  o.replica[at] = r;
  o.msg_off[at] = bm;
  u64 w = bm, eo = be;
  outbox_walk(P, C, r, a, err, [&](const Msg& m, u32 type, u32 to, u32 n) {
    rbe_message x;
    outbox_msg_out(P, C, g, k, m, type, to, x);
    ObSrc s;
    s.at = (m.pad0 & kMsgXEnt) ? kObSpill | (u64)m.ent_off : r * C.ecap + m.ent_off;
    s.base = m.log_index + 1;
    s.rep = type == M_Replicate ? 1u : 0u;
    s.par = par;
    o.msgs[w] = x;
    o.ent_off[w] = eo;
    o.src[w] = s;
    w++;
    eo += n;
  });
}

// Entry j of the call: its message by binary search in ent_off[0 .. nm], the
// Ent from where the message's descriptor says, and the record half of
// rbe_collect.h.  Every load happens before the caller's first store.
RBE_HD u32 outbox_entry(const Planes& P, const Params& C, const u8* heap, u64 heap_head,
                        const u64* ent_off, const ObSrc* src, u64 nm, u64 j, CeEnt* out) {
  const u64 sl = collect_slot_of(ent_off, nm, j);
  const ObSrc s = src[sl];
  const u64 q = j - ent_off[sl];
  const u32 par = s.par & 1u;
  const Ent x = (s.at & kObSpill) ? spill_at<const Ent>(P, par, s.at & ~kObSpill)[q]
                                  : P.arena[par][s.at + q];
  return collect_ent_record(C, heap, heap_head, x, s.rep ? s.base + q : 0, out);
}

}  // namespace rbe
