// tsw_codes.hip — utilities over the next-hop code store: pending markers back to unknown (the whole
// store, or the pairs of a queue range) and the codes of queued pairs out of / into the store.
#include <hip/hip_runtime.h>

#include "tsw_internal.h"
#include "tsw_launch.h"

namespace tsw {

// Error recovery: every NH_PENDING / NH_PENDING_S code of the store back to NH_UNKNOWN (a K3 pass that failed
// after its pairs were marked must not leave them pending for later calls). 8 codes per thread.
__global__ void k_reset_pending(uint64_t* __restrict__ nh8, uint64_t n8) {
  constexpr uint64_t ONES = 0x0101010101010101ull, HIGH = 0x8080808080808080ull;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n8; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w = nh8[i];
    // bytes equal to 0xFE: x = w ^ 0xFE.. has a zero byte there (classic zero-byte test, exact
    // after masking out borrows with ~x)
    // bytes 0xFE / 0xFD: w ^ 0xFE.. / w ^ 0xFD.. has a zero byte there (classic zero-byte test,
    // may flag a byte above a match too — the loop below checks each byte exactly)
    const uint64_t x1 = w ^ (ONES * (uint64_t)NH_PENDING), x2 = w ^ (ONES * (uint64_t)NH_PENDING_S);
    const uint64_t z = ((x1 - ONES) & ~x1 & HIGH) | ((x2 - ONES) & ~x2 & HIGH);
    if (z) {
      uint64_t out = w;
      for (int b = 0; b < 8; ++b) {
        const uint32_t c = (uint32_t)((w >> (8 * b)) & 0xFFu);
        if (c == NH_PENDING || c == NH_PENDING_S) out |= 0xFFull << (8 * b);
      }
      nh8[i] = out;
    }
  }
}

hipError_t launch_reset_pending(uint8_t* nh, uint64_t nbytes, hipStream_t s) {
  const uint64_t n8 = nbytes / 8u;  // table strides are multiples of 8
  if (n8 == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n8 + 255) / 256, 8192);
  hipLaunchKernelGGL(k_reset_pending, dim3(grid), dim3(256), 0, s, reinterpret_cast<uint64_t*>(nh), n8);
  return hipGetLastError();
}

// Caller-resolved K3 (tsw_plan_mapd_resolved / tsw_next_hop_codes): codes of queued (start, goal) pairs
// out of / into the next-hop store. Q[i].tab is the goal's table slot.
__global__ void k_gather_codes(const AstarQuery* __restrict__ Q, uint32_t nq, const uint8_t* __restrict__ nh,
                               uint64_t nstride, uint8_t* __restrict__ out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) {
    const AstarQuery q = Q[i];
    out[i] = q.tab < 0 ? NH_UNKNOWN : nh[(uint64_t)q.tab * nstride + q.v];
  }
}
__global__ void k_put_codes(const AstarQuery* __restrict__ Q, uint32_t nq, const uint8_t* __restrict__ codes,
                            uint8_t* __restrict__ nh, uint64_t nstride) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) {
    const AstarQuery q = Q[i];
    if (q.tab >= 0) nh[(uint64_t)q.tab * nstride + q.v] = codes[i];
  }
}

hipError_t launch_gather_codes(const AstarQuery* Q, uint32_t nq, const uint8_t* nh, uint64_t nstride, uint8_t* out,
                               hipStream_t s) {
  if (nq == 0) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((nq + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_gather_codes, dim3(grid), dim3(256), 0, s, Q, nq, nh, nstride, out);
  return hipGetLastError();
}

hipError_t launch_put_codes(const AstarQuery* Q, uint32_t nq, const uint8_t* codes, uint8_t* nh, uint64_t nstride,
                            hipStream_t s) {
  if (nq == 0) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((nq + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_put_codes, dim3(grid), dim3(256), 0, s, Q, nq, codes, nh, nstride);
  return hipGetLastError();
}

// The pending markers of queue entries [from, to) back to NH_UNKNOWN (a coop plan's unclaimed
// speculative pairs): O(entries), where launch_reset_pending sweeps the whole store (C5: 18 GB).
__global__ void k_reset_queue(const AstarQuery* __restrict__ Q, uint32_t from, uint32_t to, uint8_t* __restrict__ nh,
                              uint64_t nstride) {
  for (uint32_t i = from + blockIdx.x * blockDim.x + threadIdx.x; i < to; i += gridDim.x * blockDim.x) {
    const AstarQuery q = Q[i];
    if (q.tab < 0) continue;
    uint8_t* p = nh + (uint64_t)q.tab * nstride + q.v;
    const uint8_t c = *p;
    if (c == NH_PENDING || c == NH_PENDING_S) *p = NH_UNKNOWN;
  }
}

hipError_t launch_reset_queue(const AstarQuery* Q, uint32_t from, uint32_t to, uint8_t* nh, uint64_t nstride,
                              hipStream_t s) {
  if (to <= from) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((to - from + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_reset_queue, dim3(grid), dim3(256), 0, s, Q, from, to, nh, nstride);
  return hipGetLastError();
}

}  // namespace tsw
