// dev_buf.h -- move-only owners of what a handle allocates: device buffers, pinned host blocks, graph executables.
// A member of one of these types is released with the struct that holds it (psba_internal.h: ProblemState for what an
// upload creates, psba_ctx for what lives as long as the handle), so nothing has to be listed anywhere to be freed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

struct psba_ctx;

namespace psba {

// hipMalloc (device) or hipHostMalloc (pinned) of at least one byte, errors through fail() (psba_api.cpp).  Device
// memory under PSBA_DEBUG_POISON=1 (tests) is filled with 0xFF bytes (NaN as doubles, -1 as ints) and the handle's
// stream waited for, so that anything read before it is written shows in the results instead of depending on what
// the allocator recycled
int alloc_bytes(psba_ctx *h, void **p, size_t bytes, bool pinned);

template <typename P, auto Free>
class Owned {
 public:
  Owned() = default;
  Owned(Owned &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  Owned &operator=(Owned &&o) noexcept {
    if (this != &o) {
      reset(o.p_);
      o.p_ = nullptr;
    }
    return *this;
  }
  ~Owned() { reset(); }
  void reset(P p = nullptr) {
    if (p_) (void)Free(p_);
    p_ = p;
  }
  P get() const { return p_; }
  operator P() const { return p_; }  // launch sites, hipMemcpy calls and pointer arithmetic read as with a plain pointer

 protected:
  P p_ = nullptr;
};

template <typename T, bool PINNED>
class Buf : public Owned<T *, PINNED ? hipHostFree : hipFree> {
 public:
  // n elements (at least one): whatever was held is released first
  int alloc(psba_ctx *h, size_t n) {
    this->reset();
    return alloc_bytes(h, (void **)&this->p_, sizeof(T) * (n ? n : 1), PINNED);
  }
};
template <typename T>
using DevBuf = Buf<T, false>;
template <typename T>
using PinnedBuf = Buf<T, true>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

}  // namespace psba
