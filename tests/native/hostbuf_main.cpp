// hostbuf_main.cpp -- csrc/tfg_hostbuf.hpp's Buf<Mem> against a counting
// allocator that can fail its n-th allocation.  Stand-alone (its own main, no
// HIP): tests/test_hostbuf.py compiles and runs it; a failed check prints its
// line and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../topoflow-glacier_amd/csrc/tfg_hostbuf.hpp"

namespace {

int g_live = 0;      // allocations not yet released
int g_allocs = 0;    // alloc() calls so far
int g_fail_at = -1;  // the alloc() call (counted from 0) that fails, or -1
int g_failed = 0;    // failed checks

struct FakeMem {
  static int alloc(void** p, size_t bytes) {
    if (g_allocs++ == g_fail_at) return 2;  // "out of memory"; *p left alone
    *p = std::malloc(bytes);
    ++g_live;
    return 0;
  }
  static int release(void* p) {
    std::free(p);
    --g_live;
    return 0;
  }
};
using B = tfg_host::Buf<FakeMem>;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("hostbuf_main.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

void test_grow_and_keep() {
  B b;
  CHECK(b.ptr == nullptr && b.cap == 0);
  CHECK(b.reserve(0) == 0 && b.ptr == nullptr && g_allocs == 0);  // nothing asked, nothing allocated
  CHECK(b.reserve(100) == 0 && b.ptr != nullptr && b.cap == 100 && g_live == 1);
  static_cast<char*>(b.ptr)[99] = 1;  // the whole capacity is the caller's (for a sanitizer build)
  void* p = b.ptr;
  const int allocs = g_allocs;
  CHECK(b.reserve(40) == 0 && b.ptr == p && b.cap == 100 && g_allocs == allocs);   // a smaller request keeps the buffer
  CHECK(b.reserve(100) == 0 && b.ptr == p && b.cap == 100 && g_allocs == allocs);  // so does an equal one
  CHECK(b.reserve(101) == 0 && b.cap == 101 && g_allocs == allocs + 1 && g_live == 1);  // released before it grew
  static_cast<char*>(b.ptr)[100] = 1;
  CHECK(b.reset() == 0 && b.ptr == nullptr && b.cap == 0 && g_live == 0);
  CHECK(b.reset() == 0 && g_live == 0);  // twice is harmless
}

// The defect this type replaces: free, null the pointer, fail to allocate, keep
// the old capacity -- and the next smaller request "fits" a null pointer.
void test_failed_grow() {
  B b;
  CHECK(b.reserve(64) == 0 && g_live == 1);
  g_fail_at = g_allocs;
  CHECK(b.reserve(128) == 2);  // the allocator's own code comes back
  CHECK(b.ptr == nullptr && b.cap == 0 && g_live == 0);
  g_fail_at = -1;
  const int allocs = g_allocs;
  CHECK(b.reserve(32) == 0);  // smaller than both earlier sizes: allocates again
  CHECK(b.ptr != nullptr && b.cap == 32 && g_allocs == allocs + 1 && g_live == 1);
  static_cast<char*>(b.ptr)[31] = 1;
  g_fail_at = g_allocs;  // a first allocation that fails
  B c;
  CHECK(c.reserve(8) == 2 && c.ptr == nullptr && c.cap == 0 && g_live == 1);
  g_fail_at = -1;
}

void test_moves() {
  B a;
  CHECK(a.reserve(16) == 0);
  void* pa = a.ptr;
  B b(std::move(a));  // construction empties the source
  CHECK(a.ptr == nullptr && a.cap == 0 && b.ptr == pa && b.cap == 16 && g_live == 1);
  B c;
  CHECK(c.reserve(24) == 0 && g_live == 2);
  c = std::move(b);  // assignment releases the target's old buffer and empties the source
  CHECK(g_live == 1 && c.ptr == pa && c.cap == 16 && b.ptr == nullptr && b.cap == 0);
  B& self = c;
  c = std::move(self);  // to itself: kept
  CHECK(c.ptr == pa && c.cap == 16 && g_live == 1);
  CHECK(a.reserve(8) == 0 && g_live == 2);  // a moved-from buffer is an empty one
}

}  // namespace

int main() {
  test_grow_and_keep();
  CHECK(g_live == 0);
  test_failed_grow();
  CHECK(g_live == 0);
  test_moves();
  CHECK(g_live == 0);  // every destructor released
  std::printf("hostbuf: %d allocations, %d live at exit, %d failed checks\n", g_allocs, g_live, g_failed);
  return g_failed || g_live ? 1 : 0;
}
