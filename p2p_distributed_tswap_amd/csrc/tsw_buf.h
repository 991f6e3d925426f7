// tsw_buf.h — the two owning buffer types of the host runtime: device memory (DevBuf) and pinned host
// memory (PinnedBuf). Move-only; the destructor frees. Neither synchronises a stream: a caller that
// regrows a buffer a kernel may still use drains its stream first. Host-only (HIP runtime API and the
// standard library), so a host compiler builds it alone (tests/host/devbuf_main.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

namespace tsw {

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { (void)reset(); }

  operator T*() const { return p; }
  T* operator->() const { return p; }
  bool holds(size_t n) const { return n <= cap && p; }

  // frees and nulls (also when hipFree reports an error: the block is never freed twice)
  hipError_t reset() {
    hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    cap = 0;
    return e;
  }
  // exactly n elements, contents not preserved; on failure the buffer is empty
  hipError_t alloc(size_t n) {
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) p = nullptr;
    else cap = n;
    return e;
  }
  // room for `need` elements, growing by half at least (16 elements at least), contents not preserved;
  // nothing happens while the buffer holds `need`; on failure the buffer is empty
  hipError_t grow(size_t need) {
    if (holds(need)) return hipSuccess;
    return alloc(std::max<size_t>(need, std::max<size_t>(cap + cap / 2, 16)));
  }
};

template <class T>
struct PinnedBuf {
  T* p = nullptr;
  T* dev = nullptr;  // the device's address of a hipHostMallocMapped buffer, once map() has asked for it
  size_t cap = 0;    // elements

  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept
      : p(std::exchange(o.p, nullptr)), dev(std::exchange(o.dev, nullptr)), cap(std::exchange(o.cap, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p = std::exchange(o.p, nullptr);
      dev = std::exchange(o.dev, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~PinnedBuf() { (void)reset(); }

  operator T*() const { return p; }
  T* operator->() const { return p; }
  bool holds(size_t n) const { return n <= cap && p; }

  hipError_t reset() {
    hipError_t e = p ? hipHostFree(p) : hipSuccess;
    p = dev = nullptr;
    cap = 0;
    return e;
  }
  // exactly n elements with the given hipHostMalloc flags; on failure the buffer is empty
  hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), flags);
    if (e != hipSuccess) p = nullptr;
    else cap = n;
    return e;
  }
  // the device alias of a buffer allocated with hipHostMallocMapped
  hipError_t map() { return hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), p, 0); }
};

}  // namespace tsw
