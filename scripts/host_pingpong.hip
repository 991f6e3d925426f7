// host_pingpong.hip — round trip of one word between a running kernel and a host thread through mapped
// coherent host memory (hipHostMallocCoherent | hipHostMallocMapped, as the context's h_flags and the
// host A* service's rings): the transport cost of asking the host for a next hop from inside k_plan.
// One lane stores a sequence number to `ping` (system scope), the host echoes it into `pong`, the lane
// spins on `pong` with system-scope loads and records the wall_clock64 delta (100 MHz ticks).
// Build: hipcc --offload-arch=gfx950 -O2 -o scripts/bin/host_pingpong scripts/host_pingpong.hip
// Run:   scripts/bin/host_pingpong [trips]     (scripts/host_pingpong.py does both)
// Two passes: the host spinning on `ping`, and the host in a 50 us sleep loop (the dispatch wait loop
// before the service). A trip that gets no echo within 20 ms ends the kernel (reported as lost).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

__global__ void k_pingpong(uint32_t* ping, const uint32_t* pong, uint32_t trips, unsigned long long* dt, uint32_t* lost) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (uint32_t i = 1; i <= trips; ++i) {
    const unsigned long long t0 = wall_clock64();
    __hip_atomic_store(ping, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    unsigned long long t = t0;
    while (__hip_atomic_load(pong, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != i) {
      t = wall_clock64();
      if (t - t0 > 2000000ull) {  // 20 ms: no echo
        *lost = i;
        __hip_atomic_store(ping, trips, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // releases the host loop
        return;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    dt[i - 1] = wall_clock64() - t0;
  }
}

#define CHK(x)                                                                      \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                       \
      return 1;                                                                     \
    }                                                                               \
  } while (0)

int main(int argc, char** argv) {
  const uint32_t trips = argc > 1 ? (uint32_t)std::max(1, atoi(argv[1])) : 1000u;
  uint32_t* words = nullptr;  // [0] ping, [32] pong: separate 128-B lines
  uint32_t* dwords = nullptr;
  CHK(hipHostMalloc(&words, 256, hipHostMallocCoherent | hipHostMallocMapped));
  CHK(hipHostGetDevicePointer((void**)&dwords, words, 0));
  unsigned long long* d_dt = nullptr;
  uint32_t* d_lost = nullptr;
  CHK(hipMalloc(&d_dt, trips * sizeof(unsigned long long)));
  CHK(hipMalloc(&d_lost, 4));
  int khz = 100000;
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0);
  hipStream_t s;
  CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  for (int pass = 0; pass < 3; ++pass) {  // pass 0 warms up (spinning host)
    const bool sleeping = pass == 2;
    volatile uint32_t* ping = words;
    volatile uint32_t* pong = words + 32;
    *ping = 0u;
    *pong = 0u;
    CHK(hipMemsetAsync(d_lost, 0, 4, s));
    hipLaunchKernelGGL(k_pingpong, dim3(1), dim3(64), 0, s, dwords, dwords + 32, trips, d_dt, d_lost);
    CHK(hipGetLastError());
    (void)hipStreamQuery(s);  // submits the launch
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t last = 0;
    while (last != trips && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(30)) {
      const uint32_t v = *ping;
      if (v != last) {
        *pong = v;
        last = v;
      }
      if (sleeping) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    CHK(hipStreamSynchronize(s));
    uint32_t lost = 0;
    std::vector<unsigned long long> dt(trips);
    CHK(hipMemcpy(&lost, d_lost, 4, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(dt.data(), d_dt, trips * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (pass == 0) continue;
    if (lost) {
      printf("%s host: trip %u got no echo within 20 ms\n", sleeping ? "sleeping (50 us)" : "spinning", lost);
      continue;
    }
    std::sort(dt.begin(), dt.end());
    auto us = [&](size_t i) { return (double)dt[std::min<size_t>(i, trips - 1)] * 1e3 / khz; };
    printf("%s host: %u round trips, us: min %.2f p10 %.2f median %.2f p90 %.2f p99 %.2f max %.2f\n",
           sleeping ? "sleeping (50 us)" : "spinning", trips, us(0), us(trips / 10), us(trips / 2), us(trips * 9 / 10),
           us(trips * 99 / 100), us(trips - 1));
  }
  (void)hipFree(d_dt);
  (void)hipFree(d_lost);
  (void)hipHostFree(words);
  return 0;
}
