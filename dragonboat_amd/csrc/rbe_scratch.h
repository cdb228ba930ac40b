// rbe_scratch.h — the one owner of a buffer in the host layer (DESIGN.md
// §Buffer ownership): a growable block of one kind of memory, released by its
// destructor.  The kind is a policy M, so this header needs no HIP:
//   static int  alloc(void** p, uint64_t bytes);   RBE_OK, or an error it has reported
//   static void free(void* p);
//   static int  copy(void* dst, const void* src, uint64_t bytes, void* stream);
//                                  within the kind, on `stream`, and wait for it
// The HIP policies (DevMem, PinnedMem, MappedMem) are in rbe_kernels.h.
//
// Any reserve may move the buffer: recompute pointers derived from p() after it.
#pragma once
#include <cstdint>

namespace rbe {

template <class M>
class Scratch {
 public:
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  Scratch(Scratch&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.forget(); }
  Scratch& operator=(Scratch&& o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_;
      bytes_ = o.bytes_;
      o.forget();
    }
    return *this;
  }
  ~Scratch() { release(); }

  uint8_t* p() const { return p_; }
  uint64_t bytes() const { return bytes_; }

  // At least `need` bytes, contents undefined after a growth.  The old buffer
  // is freed before the new one is allocated (peak memory next to a large
  // pool); after a failed allocation the object is empty and usable again.
  int reserve(uint64_t need) { return reserve_cap(need, cap_for(need)); }
  // The same with the caller's capacity rule: `cap` (>= need) bytes when short.
  int reserve_cap(uint64_t need, uint64_t cap) {
    if (need <= bytes_) return 0;
    release();
    return take(cap);
  }
  // At least `need` bytes with the first `keep` bytes preserved: when short,
  // a new buffer, a copy on `stream`, a wait, then the old one is freed.  On a
  // failure the new buffer is freed and the old one is left as it was.
  int reserve_keep(uint64_t need, uint64_t keep, void* stream) {
    if (need <= bytes_) return 0;
    Scratch n;
    int rc = n.take(cap_for(need));
    if (!rc && p_) rc = M::copy(n.p_, p_, keep < bytes_ ? keep : bytes_, stream);
    if (rc) return rc;
    *this = static_cast<Scratch&&>(n);
    return 0;
  }

 private:
  static uint64_t cap_for(uint64_t need) { return need + need / 2 + 4096; }
  int take(uint64_t cap) {  // (empty on entry)
    void* q = nullptr;
    const int rc = M::alloc(&q, cap);
    if (rc) return rc;
    p_ = static_cast<uint8_t*>(q);
    bytes_ = cap;
    return 0;
  }
  void forget() {
    p_ = nullptr;
    bytes_ = 0;
  }
  void release() {
    if (p_) M::free(p_);
    forget();
  }
  uint8_t* p_ = nullptr;
  uint64_t bytes_ = 0;
};

}  // namespace rbe
