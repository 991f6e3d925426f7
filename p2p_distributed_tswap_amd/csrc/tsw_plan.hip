// tsw_plan.hip — host side of the persistent plan kernel k_plan (tsw_plan_kernel.h): the occupancy
// build and the launch, which picks one of the k_plan instantiations (launch_plan_t, tsw_plan.h)
// that tsw_plan_v*.hip compile.
#include "tsw_plan_dev.h"

namespace tsw {

// occupancy in the k_plan encoding: lowest agent index | OCC_FLAG if shared, OCC_NONE if empty
__global__ void k_occ_init(uint32_t* occ, uint32_t* cnt, uint32_t ncell) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncell) {
    occ[c] = OCC_NONE;
    cnt[c] = 0u;
  }
}
__global__ void k_occ_add(const uint32_t* v, uint32_t n, uint32_t* occ, uint32_t* cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    atomicAdd(&cnt[v[i]], 1u);
    atomicMin(&occ[v[i]], i);
  }
}
__global__ void k_occ_flag(uint32_t* occ, const uint32_t* cnt, uint32_t ncell, uint32_t* dups) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncell && cnt[c] > 1u) {
    occ[c] |= OCC_FLAG;
    *dups = 1u;
  }
}

hipError_t launch_occ(const uint32_t* v, uint32_t n, uint32_t* occ, uint32_t* cnt, uint32_t ncell, uint32_t* dups,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_occ_init, dim3((ncell + 255) / 256), dim3(256), 0, s, occ, cnt, ncell);
  if (n) hipLaunchKernelGGL(k_occ_add, dim3((n + 255) / 256), dim3(256), 0, s, v, n, occ, cnt);
  hipLaunchKernelGGL(k_occ_flag, dim3((ncell + 255) / 256), dim3(256), 0, s, occ, cnt, ncell, dups);
  return hipGetLastError();
}

hipError_t launch_plan(const PlanArgs& P, PlanArgs* d_args, const WorkerArgs* W, uint32_t worker_blocks, size_t lds,
                       uint32_t block, hipStream_t s) {
  WorkerArgs none{};
  const WorkerArgs& A = (W && P.coop) ? *W : none;
  const uint32_t grid = 1u + ((W && P.coop) ? worker_blocks : 0u);
  if (grid > 1u && ((size_t)A.wpb * A.lds_per_wave > lds || A.wpb * 64u > block)) return hipErrorInvalidValue;
  // the kernel reads its arguments from d_args (stream order: after the previous dispatch has finished)
  if (hipError_t e = hipMemcpyAsync(d_args, &P, sizeof(PlanArgs), hipMemcpyHostToDevice, s); e != hipSuccess) return e;
  // k_plan<AG, OC, MUL, PG> by what the host placed in LDS (plan_variant, tsw_place.h: case k is tsw_plan_v<k>.hip)
  const PlanPlacement pl{P.agents_lds != 0u, P.occ_lds != 0u, P.mu_lds != 0u, P.f_lds != 0u, P.tasks_lds != 0u, P.part_lds};
  switch (plan_variant(pl)) {
    case 0: return launch_plan_t<true, true, true, false>(d_args, A, grid, lds, block, s);
    case 1: return launch_plan_t<true, true, false, false>(d_args, A, grid, lds, block, s);
    case 2: return launch_plan_t<true, false, false, false>(d_args, A, grid, lds, block, s);
    case 3: return launch_plan_t<false, false, false, true>(d_args, A, grid, lds, block, s);
    case 4: return launch_plan_t<false, true, true, false>(d_args, A, grid, lds, block, s);
    case 5: return launch_plan_t<false, true, false, false>(d_args, A, grid, lds, block, s);
    default: return launch_plan_t<false, false, false, false>(d_args, A, grid, lds, block, s);
  }
}

}  // namespace tsw
