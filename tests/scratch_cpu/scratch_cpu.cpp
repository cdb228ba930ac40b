// Stand-alone check of rbe_scratch.h over a fake memory policy: malloc / free /
// memcpy with a log of the calls and a budget of allowed allocations.  Built
// with the address and undefined-behaviour sanitizers by tests/test_scratch.py;
// exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../dragonboat_amd/csrc/rbe_scratch.h"
#include "../../include/rbe.h"

namespace {

struct Call {
  char op;  // 'a' alloc, 'f' free, 'c' copy
  void* p;
  uint64_t n;
};
std::vector<Call> g_log;
long g_allow = -1;  // allocations still allowed (< 0: any number)
int g_allocs = 0, g_frees = 0;

struct FakeMem {
  static int alloc(void** p, uint64_t n) {
    if (g_allow == 0) return RBE_E_HIP;
    if (g_allow > 0) g_allow--;
    *p = malloc(n);
    g_allocs++;
    g_log.push_back({'a', *p, n});
    return RBE_OK;
  }
  static void free(void* p) {
    g_frees++;
    g_log.push_back({'f', p, 0});
    ::free(p);
  }
  static int copy(void* d, const void* s, uint64_t n, void*) {
    g_log.push_back({'c', d, n});
    memcpy(d, s, n);
    return RBE_OK;
  }
};
using Buf = rbe::Scratch<FakeMem>;

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

// 1. need <= bytes: no allocator call, the pointer stays
void case_reuse() {
  Buf b;
  CHECK(b.p() == nullptr && b.bytes() == 0);
  CHECK(b.reserve(0) == RBE_OK && b.p() == nullptr && g_log.empty());
  CHECK(b.reserve(1000) == RBE_OK);
  uint8_t* p = b.p();
  const size_t calls = g_log.size();
  CHECK(b.reserve(1) == RBE_OK && b.reserve(1000) == RBE_OK && b.reserve(b.bytes()) == RBE_OK);
  CHECK(b.reserve_cap(b.bytes(), 1u << 20) == RBE_OK);
  CHECK(b.reserve_keep(b.bytes(), 10, nullptr) == RBE_OK);
  CHECK(b.p() == p && g_log.size() == calls);
}

// 2. growth frees first, then allocates need + need/2 + 4096; reserve_cap: cap
void case_growth() {
  Buf b;
  CHECK(b.reserve(1000) == RBE_OK && b.bytes() == 1000 + 500 + 4096);
  void* old = b.p();
  g_log.clear();
  const uint64_t need = b.bytes() + 1;
  CHECK(b.reserve(need) == RBE_OK);
  CHECK(g_log.size() == 2 && g_log[0].op == 'f' && g_log[0].p == old && g_log[1].op == 'a');
  CHECK(b.bytes() == need + need / 2 + 4096 && g_log[1].n == b.bytes() && g_log[1].p == b.p());
  old = b.p();
  g_log.clear();
  CHECK(b.reserve_cap(b.bytes() + 7, 3 * b.bytes()) == RBE_OK);
  CHECK(g_log.size() == 2 && g_log[0].op == 'f' && g_log[0].p == old && g_log[1].op == 'a');
  CHECK(b.bytes() == 3 * (need + need / 2 + 4096) && g_log[1].n == b.bytes());
  Buf c;
  CHECK(c.reserve_cap(33, 33) == RBE_OK && c.bytes() == 33);
  c.p()[32] = 1;  // (the sanitizer checks the size)
}

// 3. a refused allocation empties the object; the next reserve succeeds
void case_refused() {
  Buf b;
  CHECK(b.reserve(100) == RBE_OK);
  g_allow = 0;
  CHECK(b.reserve(100000) == RBE_E_HIP);
  CHECK(b.p() == nullptr && b.bytes() == 0);
  CHECK(b.reserve_cap(10, 10) == RBE_E_HIP && b.p() == nullptr && b.bytes() == 0);
  g_allow = -1;
  CHECK(b.reserve(100000) == RBE_OK && b.p() && b.bytes() == 100000 + 50000 + 4096);
  memset(b.p(), 0xAB, b.bytes());
}

// 4. reserve_keep keeps the prefix byte for byte; refused: nothing changes
void case_keep() {
  Buf b;
  CHECK(b.reserve_cap(300, 300) == RBE_OK);
  for (int i = 0; i < 300; i++) b.p()[i] = (uint8_t)(i * 7 + 3);
  uint8_t* old = b.p();
  g_allow = 0;
  g_log.clear();
  CHECK(b.reserve_keep(5000, 257, nullptr) == RBE_E_HIP);
  CHECK(b.p() == old && b.bytes() == 300 && g_log.empty());
  for (int i = 0; i < 300; i++) CHECK(b.p()[i] == (uint8_t)(i * 7 + 3));
  g_allow = -1;
  CHECK(b.reserve_keep(5000, 257, nullptr) == RBE_OK);
  CHECK(b.p() != old && b.bytes() == 5000 + 2500 + 4096);
  // the new buffer, the copy into it, and only then the old one's free
  CHECK(g_log.size() == 3 && g_log[0].op == 'a' && g_log[0].p == b.p());
  CHECK(g_log[1].op == 'c' && g_log[1].p == b.p() && g_log[1].n == 257);
  CHECK(g_log[2].op == 'f' && g_log[2].p == old);
  for (int i = 0; i < 257; i++) CHECK(b.p()[i] == (uint8_t)(i * 7 + 3));
  // from empty: an allocation and nothing to copy
  Buf c;
  g_log.clear();
  CHECK(c.reserve_keep(64, 64, nullptr) == RBE_OK && g_log.size() == 1 && g_log[0].op == 'a');
  // keep is bounded by what the old buffer holds
  Buf d;
  CHECK(d.reserve_cap(16, 16) == RBE_OK);
  memset(d.p(), 0x5A, 16);
  CHECK(d.reserve_keep(100, 1000, nullptr) == RBE_OK);
  for (int i = 0; i < 16; i++) CHECK(d.p()[i] == 0x5A);
}

// 5. one free per buffer; moved-from and never-reserved objects free nothing
void case_lifetime() {
  const int f0 = g_frees;
  { Buf never; }
  CHECK(g_frees == f0);
  {
    Buf a;
    CHECK(a.reserve(10) == RBE_OK);
    uint8_t* p = a.p();
    Buf b(std::move(a));
    CHECK(a.p() == nullptr && a.bytes() == 0 && b.p() == p);
    Buf c;
    CHECK(c.reserve(20) == RBE_OK);
    c = std::move(b);  // c's own buffer goes now
    CHECK(g_frees == f0 + 1 && c.p() == p && b.p() == nullptr && b.bytes() == 0);
    std::vector<Buf> v;
    v.push_back(std::move(c));
    v.emplace_back();
    v.emplace_back();  // (reallocations move the elements)
    CHECK(v[0].p() == p && g_frees == f0 + 1);
  }
  CHECK(g_frees == f0 + 2);
}

}  // namespace

int main() {
  case_reuse();
  case_growth();
  case_refused();
  case_keep();
  case_lifetime();
  CHECK(g_allocs == g_frees);
  printf("scratch_cpu ok: %d allocations, %d frees\n", g_allocs, g_frees);
  return 0;
}
