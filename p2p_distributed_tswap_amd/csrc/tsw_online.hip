// tsw_online.hip — the two kernels that run between k_plan segments of tsw_plan_mapd_online
// (tsw_online_host.hip): the tasks of a release epoch become live entries of the K4 index, and the last
// recorded column is repeated while the fleet has nothing to do. Plain grid-stride kernels, no LDS.
#include <hip/hip_runtime.h>

#include "tsw_internal.h"
#include "tsw_launch.h"

namespace tsw {

constexpr uint32_t KCH_ONLINE = 32u;  // entries per K4 index chunk (k_plan's KCH, build_task_index)

// Tasks rel_order[lo .. hi) become visible: their entries of the Morton-ordered LIVE array get their pickup
// points back (they were TASK_TAKEN while hidden) and their chunks' counts of untaken entries rise. Many
// tasks of one epoch may share a chunk, hence the atomic. Every task is released once, so no two threads
// write the same LIVE entry.
__global__ void k_task_release(const uint32_t* __restrict__ rel_order, uint32_t lo, uint32_t hi,
                               const uint32_t* __restrict__ kpos, const uint32_t* __restrict__ pxy,
                               uint32_t* __restrict__ live, uint32_t* __restrict__ kcnt) {
  for (uint32_t j = lo + blockIdx.x * blockDim.x + threadIdx.x; j < hi; j += gridDim.x * blockDim.x) {
    const uint32_t k = rel_order[j], pos = kpos[k];
    live[pos] = pxy[k];
    atomicAdd(&kcnt[pos / KCH_ONLINE], 1u);
  }
}

hipError_t launch_task_release(const uint32_t* rel_order, uint32_t lo, uint32_t hi, const uint32_t* kpos,
                               const uint32_t* pxy, uint32_t* live, uint32_t* kcnt, hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>((hi - lo + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_task_release, dim3(grid), dim3(256), 0, s, rel_order, lo, hi, kpos, pxy, live, kcnt);
  return hipGetLastError();
}

// Columns t_from .. t_to - 1 of the timestep-major records (t * n + i), and of the goal trace when there is
// one, repeat column t_from - 1 (t_from >= 1): a fleet at rest, every agent idle on its goal.
__global__ void k_rec_hold(uint64_t* __restrict__ rec, uint32_t* __restrict__ grec, uint32_t n, uint32_t t_from,
                           uint32_t t_to) {
  const uint64_t total = (uint64_t)(t_to - t_from) * n, src = (uint64_t)(t_from - 1u) * n, dst = (uint64_t)t_from * n;
  for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e % n;
    rec[dst + e] = rec[src + i];
    if (grec) grec[dst + e] = grec[src + i];
  }
}

hipError_t launch_rec_hold(uint64_t* rec, uint32_t* grec, uint32_t n, uint32_t t_from, uint32_t t_to, hipStream_t s) {
  if (n == 0u || t_to <= t_from || t_from == 0u) return hipSuccess;
  const uint64_t total = (uint64_t)(t_to - t_from) * n;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_rec_hold, dim3(grid), dim3(256), 0, s, rec, grec, n, t_from, t_to);
  return hipGetLastError();
}

}  // namespace tsw
