// ponyc_amd/csrc/dev_buf.h on its own: alloc, re-alloc, move, swap, reset and
// the failure path, with the process-wide live counts checked after each.
// Runs with or without a GPU: without one every hipMalloc fails (the failure
// path throughout); with one the small allocations succeed and a request no
// device can meet fails. Built with the host sanitizers by hand
// (-Xarch_host -fsanitize=address,undefined) and plain by tests/test_dev_buf.py.
#include "dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#define CHECK(c)                                                              \
  do {                                                                        \
    if(!(c)) { printf("dev_buf_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } \
  } while(0)

static bool live_is(uint64_t count, uint64_t bytes)
{
  return buf_live.count.load() == count && buf_live.bytes.load() == bytes;
}

// alloc either gives n elements or leaves the buffer empty; returns whether it gave them
template<class B>
static bool alloc_checked(B& b, size_t n)
{
  const hipError_t e = b.alloc(n);
  if(e != hipSuccess)
  {
    (void)hipGetLastError();
    CHECK(b.get() == nullptr && b.size() == 0 && !b);
    return false;
  }
  CHECK(b.get() != nullptr && b.size() == n);
  return true;
}

template<class B>
static void exercise(const char* kind)
{
  using T = std::remove_reference_t<decltype(*std::declval<B&>().get())>;
  const size_t esz = sizeof(T);
  CHECK(live_is(0, 0));
  {
    B empty;                                   // destroying and resetting empty buffers is safe
    empty.reset();
    empty.reset();
    B moved(std::move(empty));
    moved = B();
    CHECK(!moved && moved.size() == 0 && live_is(0, 0));
  }
  int ok = 0, failed = 0;
  {
    B a, b;
    const bool ga = alloc_checked(a, 100);
    CHECK(live_is(ga ? 1 : 0, ga ? 100 * esz : 0));
    // re-allocation frees what was held: still at most one live buffer
    const bool ga2 = alloc_checked(a, 300);
    CHECK(live_is(ga2 ? 1 : 0, ga2 ? 300 * esz : 0));
    const bool gb = alloc_checked(b, 50);
    const uint64_t n = (ga2 ? 1 : 0) + (gb ? 1 : 0), by = (ga2 ? 300 : 0) * esz + (gb ? 50 : 0) * esz;
    CHECK(live_is(n, by));
    T* pa = a.get();
    T* pb = b.get();
    a.swap(b);                                 // swap moves pointer and size together
    CHECK(a.get() == pb && b.get() == pa && a.size() == (gb ? 50u : 0u) && b.size() == (ga2 ? 300u : 0u));
    CHECK(live_is(n, by));
    B c(std::move(b));                         // move construction empties the source
    CHECK(c.get() == pa && b.get() == nullptr && b.size() == 0 && live_is(n, by));
    a = std::move(c);                          // move assignment frees the target's own first
    CHECK(a.get() == pa && c.get() == nullptr && live_is(ga2 ? 1 : 0, ga2 ? 300 * esz : 0));
    T* as_ptr = a;                             // reads as a raw pointer
    CHECK(as_ptr == pa);
    // the failure path: a request nothing can meet empties the buffer that
    // held memory before, and leaves nothing live
    const hipError_t e = a.alloc((size_t)1 << 58);
    CHECK(e != hipSuccess);
    (void)hipGetLastError();
    CHECK(a.get() == nullptr && a.size() == 0 && live_is(0, 0));
    ++failed;
    const bool gd = alloc_checked(a, 7);
    (gd ? ok : failed)++;
    a.reset();
    CHECK(!a && live_is(0, 0));
    const bool ge = alloc_checked(b, 9);       // freed by the destructor below
    (ge ? ok : failed)++;
    CHECK(live_is(ge ? 1 : 0, ge ? 9 * esz : 0));
  }
  CHECK(live_is(0, 0));
  printf("dev_buf_check: %s ok (%d allocations given, %d refused)\n", kind, ok, failed);
}

int main()
{
  exercise<DevBuf<uint64_t>>("device");
  exercise<PinBuf<uint32_t>>("pinned");
  printf("dev_buf_check: ok\n");
  return 0;
}
