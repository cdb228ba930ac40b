// TEST-ONLY stand-alone program over the host build of the step
// (tests/soa_cpu/soa_cpu.cpp): the speculative inbound gathers of the fast
// steps' summary-word form (rbe_fast.h lead_gather_slot / foll_gather_slot,
// the functions lead_fast and foll_fast load through).
//
//   1. Every group size with fast steps, every receiver and sender slot,
//      maxm = 1..16 and 127, every 7-bit summary field and every gather slot:
//      a slot that loads lies in [0, maxm), and for a field of a legal
//      unspilled count word that the step accepts the loaded slots are the
//      ones the plain form reads.
//   2. The MIXED-shaped workload of test_spill.py with tiny plane capacities,
//      stepped in the summary-word form (staged = 4, traced) at N = 3 and 5.
//
// tests/test_fast_aux.py builds it with the address and undefined-behaviour
// sanitizers and runs it.  Never linked into the product, never loaded into
// Python.
#include "../soa_cpu/soa_cpu.cpp"

#include <cstdio>

namespace {

int g_bad = 0;
void bad(const char* what, int n, u32 maxm, u32 f, u32 i, u32 at) {
  if (g_bad++ < 10)
    fprintf(stderr, "fast_aux_cpu: %s: N=%d maxm=%u field=%#x (A=%u B=%u) slot %u -> %u\n", what, n,
            maxm, f, f & 7u, (f >> 3) & 7u, i, at);
}

template <int N>
u64 check_indices() {
  using Cap = FastCaps<N>;
  static_assert(Cap::MAXM < 7 && Cap::FMAXM < 7, "the 3-bit summary counts clamp at 7");
  u64 loads = 0;
  for (u32 mi = 1; mi <= 17; mi++) {
    const u32 maxm = mi <= 16 ? mi : 127u;
    for (u32 k = 0; k < (u32)N; k++)
      for (u32 j = 0; j + 1 < (u32)N; j++) {
        const u32 s = j + (j >= k ? 1u : 0u);
        for (u32 f = 0; f < 128; f++) {
          // the count word the steps rebuild from the field, as they do
          const u32 pc = aux_count_word<N>(f << (7 * j), k, s);
          const u32 a = f & 7u, b = (f >> 3) & 7u;
          if ((pc & 0x7Fu) != a || ((pc >> 7) & 0x7Fu) != b) bad("count word", N, maxm, f, 0, pc);
          const bool legal = a + b <= maxm;  // (an unspilled list holds A + B <= maxm messages)
          const bool sat = a == 7 && b == 7;  // kCntSpilled's field
          // leader: accepts A = 0, B <= MAXM; the i-th B message is at maxm - 1 - i
          for (u32 i = 0; i < Cap::MAXM; i++) {
            u32 at = ~0u;
            const bool ld = lead_gather_slot<N>(pc, maxm, i, at);
            loads += ld ? 1 : 0;
            if (ld && at >= maxm) bad(sat ? "leader, spilled list" : "leader out of range", N, maxm, f, i, at);
            if (legal && a == 0 && b <= Cap::MAXM) {
              if (ld != (i < b)) bad("leader slot set", N, maxm, f, i, at);
              if (ld && at != maxm - 1u - i) bad("leader slot", N, maxm, f, i, at);
            }
          }
          // follower: accepts A + B <= FMAXM; A messages from slot 0 up, then
          // the B messages from slot maxm - 1 down
          for (u32 i = 0; i < Cap::FMAXM; i++) {
            u32 at = ~0u;
            const bool ld = foll_gather_slot<N>(pc, maxm, i, at);
            loads += ld ? 1 : 0;
            if (ld && at >= maxm) bad(sat ? "follower, spilled list" : "follower out of range", N, maxm, f, i, at);
            if (legal && a + b <= Cap::FMAXM) {
              if (ld != (i < a + b)) bad("follower slot set", N, maxm, f, i, at);
              if (ld && at != (i < a ? i : maxm - 1u - (i - a))) bad("follower slot", N, maxm, f, i, at);
            }
          }
        }
      }
  }
  return loads;
}

struct Caps {
  u32 maxm, rtr_cap, dri_cap, ecap, rq_cap, ring;
};
// test_spill.py TINY
const Caps kTiny = {1, 1, 1, 1, 1, 8}, kFast = {2, 0, 0, 2, 4, 8};

// the MIXED-shaped workload of test_spill.test_lists_and_queues_past_capacity
template <int N>
int run_tiny(const Caps& cp, u64* slow, u64* steps) {
  rbe_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = RBE_ABI_VERSION;
  cfg.n_groups = 12;
  cfg.n_replicas = N;
  cfg.election_rtt = 10;
  cfg.heartbeat_rtt = 1;
  cfg.check_quorum = 1;
  cfg.quiesce = 1;
  cfg.trace = 1;
  cfg.cid_base = 1;
  cfg.cid_stride = 1;
  cfg.seed = 12345;
  cfg.wl_enabled = 1;
  cfg.wl_start_round = 25;
  cfg.wl_active_mod = 2;
  cfg.wl_read_permille = 500;
  cfg.iso_period = 37;
  cfg.iso_len = 20;
  cfg.iso_mod = 2;
  cfg.maxm = cp.maxm;
  cfg.rtr_cap = cp.rtr_cap;
  cfg.dri_cap = cp.dri_cap;
  cfg.ecap = cp.ecap;
  cfg.rq_cap = cp.rq_cap;
  cfg.ring = cp.ring;
  SoaEngine* e = (SoaEngine*)soa_create(&cfg);
  if (!e) return 1;
  e->staged = 4;
  for (int r = 0; r < 120; r++) run_round<N>(e);
  uint64_t nf = 0, st[5];
  soa_faults(e, &nf);
  soa_spill_stats(e, st);
  *slow += e->slow_total;
  *steps += e->counters[C_STEPS];
  int rc = 0;
  if (nf) rc = 2;
  else if (st[4]) rc = 3;
  else if (!st[2]) rc = 4;  // nothing spilled: the run shows nothing
  else if (e->slow_total >= e->counters[C_STEPS]) rc = 5;  // no fast step took a round
  soa_destroy(e);
  return rc;
}

}  // namespace

int main() {
  const u64 loads = check_indices<3>() + check_indices<4>() + check_indices<5>();
  if (g_bad) {
    fprintf(stderr, "fast_aux_cpu: %d gather slots wrong\n", g_bad);
    return 1;
  }
  u64 slow = 0, steps = 0;
  int rc;
  if ((rc = run_tiny<3>(kTiny, &slow, &steps))) return 10 + rc;
  if ((rc = run_tiny<3>(kFast, &slow, &steps))) return 20 + rc;
  if ((rc = run_tiny<5>(kTiny, &slow, &steps))) return 30 + rc;
  if ((rc = run_tiny<5>(kFast, &slow, &steps))) return 40 + rc;
  printf("fast_aux_cpu ok: %llu loading gather slots checked, %llu of %llu steps of the tiny "
         "runs on the fast steps\n",
         (unsigned long long)loads, (unsigned long long)(steps - slow), (unsigned long long)steps);
  return 0;
}
