// crh_devmem.h -- who owns a block of device or pinned memory: ONE buffer type, a pointer and its capacity that only ever change together.
// No HIP and no context here (the two HIP memory policies are in crh_context.h); checked on the CPU, against a memory policy that can be told
// to refuse, by tests/devmem_model.cpp.
//
// The rule: p == nullptr exactly when cap == 0, at every point a caller can observe -- also after a call that failed.
// NOT in here: streams and synchronisation.  Whether kernels in flight may still read the block that is about to be released, and on which
// stream, is known only where the buffer is used: the caller waits first, then reserves.
#pragma once
#include <cstddef>
#include <type_traits>
#include <utility>

namespace crh {

// Mem: struct { using status = ...; static constexpr status ok = ...; static status alloc(void** p, size_t bytes); static status free(void* p); }
template <class T, class Mem> class Buf {
 public:
  using status = typename Mem::status;
  static constexpr size_t elem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);      // Buf<void, ...>: a capacity in bytes

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buf& operator=(Buf&& o) noexcept { if (this != &o) { release(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); } return *this; }
  ~Buf() { release(); }

  operator T*() const { return p_; }      // kernel launches, copies and the kernels' scene record read the buffer as the pointer it was
  template <class U> U* as() const { return static_cast<U*>(static_cast<void*>(p_)); }
  size_t cap() const { return cap_; }     // elements
  size_t bytes() const { return cap_ * elem; }

  // Room for n elements; the old contents are GONE when it had to grow (then n + headroom are allocated).  Enough room already: nothing happens, the allocator
  // is not called.  Refused: the buffer is empty, the status says why, and a later reserve simply tries again.
  status reserve(size_t n, size_t headroom = 0)
  {
    if (n <= cap_) return Mem::ok;
    const status freed = release();
    if (freed != Mem::ok) return freed;
    void* q = nullptr;
    const status s = Mem::alloc(&q, (n + headroom) * elem);
    if (s != Mem::ok || !q) return s;
    p_ = static_cast<T*>(q); cap_ = n + headroom;
    return Mem::ok;
  }

  // Room for n elements with the first `keep` of the old ones carried over: the new block first, then copy(new, old, keep) -- the caller's copy and the
  // caller's wait for it -- then the old block is released.  Refused, or the copy failed: the OLD block and capacity stay.
  template <class Copy> status reserve_keep(size_t n, size_t keep, Copy&& copy)
  {
    if (n <= cap_) return Mem::ok;
    void* q = nullptr;
    status s = Mem::alloc(&q, n * elem);
    if (s != Mem::ok || !q) return s;
    if (p_ && keep && (s = copy(static_cast<T*>(q), p_, keep)) != Mem::ok) { Mem::free(q); return s; }
    s = release();
    p_ = static_cast<T*>(q); cap_ = n;
    return s;
  }

  status release()
  {
    if (!p_) return Mem::ok;
    void* q = std::exchange(p_, nullptr); cap_ = 0;
    return Mem::free(q);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace crh
