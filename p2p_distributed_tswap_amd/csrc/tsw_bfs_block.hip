// tsw_bfs_block.hip — K1 v1: k_bfs, batched per-goal BFS distance tables, one workgroup per goal
// (bit-parallel rows, LDS-resident frontier / visited bitmaps and, where it fits, the u16 table, one
// coalesced 16-B-per-lane write-out), fused with the next-hop classification of every cell (unique
// optimal neighbour / unreachable fallback / needs-A*). The last resort of the K1 choice (choose_bfs,
// tsw_place.h) and the test suite's TSW_BFS_KERNEL=block.
#include <hip/hip_runtime.h>

#include "tsw_internal.h"
#include "tsw_launch.h"
#include "tsw_astar.h"

namespace tsw {

// ----------------------------------------------------------------------------
// K1: batched BFS distance tables.
// One workgroup per goal (grid-stride). LDS holds the frontier bitmap (double
// buffered), the visited bitmap, the free-cell bitmap and — when LDS_TABLE —
// the whole u16 table. Each level expands the frontier with word-parallel
// shifts (east/west inside a row word with carries, north/south from the
// adjacent rows) over the Manhattan band |y - gy| <= level + 1 only. Newly
// reached cells get level+1 written into the table. The table then leaves
// LDS in one pass of 16-B stores together with the 8-B next-hop codes.
// ----------------------------------------------------------------------------
template <bool LDS_TABLE>
__global__ void __launch_bounds__(1024) k_bfs(DevGrid G, const uint32_t* __restrict__ goals,
                                              const uint32_t* __restrict__ slots, uint32_t k,
                                              uint16_t* __restrict__ dist_base, uint64_t dstride,
                                              uint8_t* __restrict__ nh_base, uint64_t nstride,
                                              uint32_t* __restrict__ err, uint8_t* __restrict__ govf) {
  extern __shared__ __align__(16) uint32_t smem[];
  const uint32_t W = G.W, H = G.H, Ww = G.Ww, nw = H * Ww, nwp = (nw + 3u) & ~3u;
  const uint32_t ncell = G.ncell, ncp = (ncell + 7u) & ~7u;
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  uint32_t* bufA = smem;
  uint32_t* bufB = smem + nwp;
  uint32_t* V = smem + 2 * nwp;
  uint32_t* FR = smem + 3 * nwp;
  uint16_t* Dl = reinterpret_cast<uint16_t*>(smem + 4 * nwp);
  const float invWw = 1.0f / (float)Ww;
  // 16-B table stores / 8-B code stores need every table (base + slot * stride) aligned, not the stride
  // alone: the caller's memory is only promised as uint16_t* / uint8_t* (run_bfs tests the same for vec16)
  const bool vec_ok = (dstride % 8u) == 0 && (reinterpret_cast<uintptr_t>(dist_base) & 15u) == 0;
  const bool nh_vec = (nstride % 8u) == 0 && (reinterpret_cast<uintptr_t>(nh_base) & 7u) == 0;

  for (uint32_t t = tid; t < nw; t += bd) FR[t] = G.freebits[t];

  for (uint32_t gi = blockIdx.x; gi < k; gi += gridDim.x) {
    const uint32_t goal = goals[gi];
    const uint64_t slot = slots ? slots[gi] : gi;
    uint16_t* Dg = dist_base + slot * dstride;
    uint16_t* D = LDS_TABLE ? Dl : Dg;
    for (uint32_t t = tid; t < nw; t += bd) {
      bufA[t] = 0u;
      bufB[t] = 0u;
      V[t] = 0u;
    }
    if (LDS_TABLE || vec_ok) {
      const uint4 inf4 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
      const uint32_t lim = LDS_TABLE ? ncp / 8u : ncell / 8u;
      for (uint32_t t = tid; t < lim; t += bd) reinterpret_cast<uint4*>(D)[t] = inf4;
      if (!LDS_TABLE)
        for (uint32_t c = (ncell & ~7u) + tid; c < ncell; c += bd) D[c] = DIST_INF;
    } else {
      for (uint32_t c = tid; c < ncell; c += bd) D[c] = DIST_INF;
    }
    __syncthreads();
    const uint32_t gx = goal % W, gy = goal / W;
    if (tid == 0) {
      const uint32_t wt = gy * Ww + (gx >> 5);
      bufA[wt] = 1u << (gx & 31u);
      V[wt] = 1u << (gx & 31u);
      D[goal] = 0;
    }
    __syncthreads();
    uint32_t* cur = bufA;
    uint32_t* nxt = bufB;
    uint32_t level = 0;
    for (;;) {
      const int lo = max(0, (int)gy - (int)level - 1);
      const int hi = min((int)H - 1, (int)gy + (int)level + 1);
      const uint32_t t0 = (uint32_t)lo * Ww, t1 = (uint32_t)(hi + 1) * Ww;
      const uint16_t dn = (uint16_t)(level + 1);
      int any = 0;
      for (uint32_t t = t0 + tid; t < t1; t += bd) {
        const uint32_t r = fast_div(t, Ww, invWw);
        const uint32_t w = t - r * Ww;
        const uint32_t f = cur[t];
        const uint32_t left = (w > 0) ? cur[t - 1] : 0u;
        const uint32_t right = (w + 1 < Ww) ? cur[t + 1] : 0u;
        const uint32_t up = (r > 0) ? cur[t - Ww] : 0u;
        const uint32_t down = (r + 1 < H) ? cur[t + Ww] : 0u;
        const uint32_t hz = (f << 1) | (left >> 31) | (f >> 1) | (right << 31);
        uint32_t nb = (hz | up | down) & FR[t] & ~V[t];
        nxt[t] = nb;
        if (nb) {
          V[t] |= nb;
          any = 1;
          const uint32_t base = r * W + (w << 5);
          while (nb) {
            const uint32_t b = __builtin_ctz(nb);
            D[base + b] = dn;
            nb &= nb - 1u;
          }
        }
      }
      any = __syncthreads_or(any);
      if (!any) break;
      ++level;
      // this pass found cells at distance `level`: 0xFFFE is the largest a table holds (0xFFFF is DIST_INF, and
      // what the pass wrote for cells 65,535 steps away), so only a pass that finds cells there is an overflow
      if (level >= 0xFFFFu) {
        if (tid == 0) atomicOr(err, ERR_DIST_OVERFLOW);
        if (tid == 0 && govf) govf[gi] = 1u;  // planned without a table (K3)
        break;
      }
      uint32_t* tmp = cur;
      cur = nxt;
      nxt = tmp;
    }
    __syncthreads();
    // write-out (+ fused next-hop classification)
    uint8_t* NHg = nh_base ? nh_base + slot * nstride : nullptr;
    if (LDS_TABLE && vec_ok) {
      for (uint32_t c8 = tid; c8 < ncell / 8u; c8 += bd)
        reinterpret_cast<uint4*>(Dg)[c8] = reinterpret_cast<const uint4*>(Dl)[c8];
      for (uint32_t c = (ncell & ~7u) + tid; c < ncell; c += bd) Dg[c] = Dl[c];
    } else if (LDS_TABLE) {
      for (uint32_t c = tid; c < ncell; c += bd) Dg[c] = Dl[c];
    }
    if (NHg && !nh_vec) {
      for (uint32_t c = tid; c < ncell; c += bd)
        NHg[c] = classify_cell(D, c, G.nbmask[c], W, goal, gx, gy);
    } else if (NHg) {
      for (uint32_t c8 = tid; c8 < ncp / 8u; c8 += bd) {
        const uint64_t m8 = reinterpret_cast<const uint64_t*>(G.nbmask)[c8];
        uint64_t codes = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
          const uint32_t c = c8 * 8u + j;
          uint8_t code = NH_UNKNOWN;
          if (c < ncell) code = classify_cell(D, c, (uint8_t)(m8 >> (8 * j)), W, goal, gx, gy);
          codes |= (uint64_t)code << (8 * j);
        }
        reinterpret_cast<uint64_t*>(NHg)[c8] = codes;
      }
    }
    __syncthreads();
  }
}

hipError_t launch_bfs(const DevGrid& G, const uint32_t* goals, const uint32_t* slots, uint32_t k,
                      uint16_t* dist_base, uint64_t dstride, uint8_t* nh_base, uint64_t nstride,
                      uint32_t* err, int max_lds, int num_cu, hipStream_t s, uint8_t* govf) {
  if (k == 0) return hipSuccess;
  size_t lds_tab = bfs_lds_bytes(G.H, G.Ww, G.ncell, true);
  size_t lds_no = bfs_lds_bytes(G.H, G.Ww, G.ncell, false);
  const bool use_tab = lds_tab <= (size_t)max_lds;
  const size_t lds = use_tab ? lds_tab : lds_no;
  if (lds > (size_t)max_lds) return hipErrorInvalidValue;
  const uint32_t nw = G.H * G.Ww;
  uint32_t bd;
  if (lds > 80 * 1024) bd = 1024;
  else if (nw <= 64) bd = 64;
  else if (nw <= 1024) bd = 256;
  else bd = 512;
  const uint32_t per_cu = (uint32_t)std::max<size_t>(1, CU_LDS_BYTES / std::max<size_t>(lds, 1));
  uint32_t grid = std::min<uint32_t>(k, (uint32_t)num_cu * std::min<uint32_t>(per_cu, 16u) * 4u);
  if (grid == 0) grid = 1;
  if (use_tab) {
    hipFuncSetAttribute((const void*)k_bfs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_bfs<true>, dim3(grid), dim3(bd), lds, s, G, goals, slots, k, dist_base, dstride,
                       nh_base, nstride, err, govf);
  } else {
    hipFuncSetAttribute((const void*)k_bfs<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_bfs<false>, dim3(grid), dim3(bd), lds, s, G, goals, slots, k, dist_base, dstride,
                       nh_base, nstride, err, govf);
  }
  return hipGetLastError();
}

}  // namespace tsw
