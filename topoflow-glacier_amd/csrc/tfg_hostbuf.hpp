// tfg_hostbuf.hpp -- the host layer's owning buffer.  Host only: no HIP
// header, so tests/native/hostbuf_main.cpp compiles it with a plain C++
// compiler and a counting allocator.
//
// Buf<Mem> owns one allocation of a memory policy
//   struct Mem { static int alloc(void**, size_t); static int release(void*); };
// (0 = success, anything else the allocator's own error code).  It only ever
// grows: reserve() keeps a buffer that is large enough, and otherwise releases
// it BEFORE allocating the larger one.  A failed grow therefore leaves
// {nullptr, 0}, never a null pointer with a stale capacity, and the next
// reserve() allocates again.  The old contents are not carried over.
//
// reserve() knows nothing of streams: a caller whose device work may still
// use the buffer asks `cap < bytes` first and waits before it calls reserve().
#pragma once

#include <cstddef>
#include <utility>

namespace tfg_host {

template <class Mem>
struct Buf {
  void* ptr = nullptr;
  size_t cap = 0;  // bytes

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      (void)reset();
      ptr = std::exchange(o.ptr, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~Buf() { (void)reset(); }

  // Release the allocation, if any: {nullptr, 0} afterwards whatever release() returned.
  int reset() {
    const int rc = ptr ? Mem::release(ptr) : 0;
    ptr = nullptr;
    cap = 0;
    return rc;
  }

  // At least `bytes` bytes.
  int reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    if (const int rc = reset()) return rc;
    void* p = nullptr;
    if (const int rc = Mem::alloc(&p, bytes)) return rc;
    ptr = p;
    cap = bytes;
    return 0;
  }
};

}  // namespace tfg_host
