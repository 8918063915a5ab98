// Owning buffers for the engine's host side (engine.hip): device memory
// (DevBuf<T>, hipMalloc) and pinned host memory (PinBuf<T>, hipHostMalloc).
// A pointer plus the element count it was allocated for; move-only; freed by
// the destructor, by reset() and ahead of a re-allocation. alloc() empties the
// buffer before it asks for the new memory, so a failure leaves it empty, not
// dangling. Converts to T*, so kernel arguments and EngDev fields read as with
// a raw pointer. Host-only: no kernel and no device header includes it.
//
// buf_live counts the buffers that hold memory, and their bytes, over the
// whole process (gpu_actor_debug_live_buffers): what the leak tests read.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

struct BufLive {
  std::atomic<uint64_t> count{0}, bytes{0};
};
inline BufLive buf_live;

template<class T, bool kPinned = false>
class DevBuf {
public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    if(this != &o) { reset(); swap(o); }
    return *this;
  }
  ~DevBuf() { reset(); }

  // n elements, uninitialised; what it held before is freed first
  hipError_t alloc(size_t n)
  {
    reset();
    void* q = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault)
                                 : hipMalloc(&q, n * sizeof(T));
    if(e != hipSuccess || !q) return e;
    p_ = static_cast<T*>(q);
    n_ = n;
    buf_live.count.fetch_add(1, std::memory_order_relaxed);
    buf_live.bytes.fetch_add(n * sizeof(T), std::memory_order_relaxed);
    return hipSuccess;
  }

  void reset() noexcept
  {
    if(!p_) return;
    (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
    buf_live.count.fetch_sub(1, std::memory_order_relaxed);
    buf_live.bytes.fetch_sub(n_ * sizeof(T), std::memory_order_relaxed);
    p_ = nullptr;
    n_ = 0;
  }

  void swap(DevBuf& o) noexcept
  {
    T* p = p_; p_ = o.p_; o.p_ = p;
    size_t n = n_; n_ = o.n_; o.n_ = n;
  }

  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  T* get() const { return p_; }
  size_t size() const { return n_; }      // elements allocated

private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

template<class T> using PinBuf = DevBuf<T, true>;
