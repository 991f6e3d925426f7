// tsw_nearby.hip — K5: NearbyAgents::get_nearby (src/bin/decentralized/agent.rs:108-153) for a whole
// fleet, on the device.
//
// Agent i's list is every agent j != i with |xi-xj| + |yi-yj| <= radius, in ascending agent index (the
// reference's order is a HashMap iteration order, i.e. unspecified; a decision depends on it only
// through "first entry at a position", which this order makes the smallest-index agent of the cell).
//   1. bin: per-cell histogram (the atomic's return value is the agent's rank inside its cell),
//      multi-block exclusive prefix -> cell_start, scatter of the agent indices into cell order (done by
//      the count kernel's lane 0)
//   2. count: the radius diamond meets row y' in the contiguous cells x +- (r - |y'-y|), i.e. in one
//      contiguous range of the cell-sorted array; one wave per agent, lanes over rows
//   3. fill: per-row ranges again, copied into LDS (self dropped) and rank-sorted into ascending index;
//      if any list is longer than NB_SORT_MAX every list comes from the ordered brute-force kernel
// Nothing that depends on the histogram atomics' arrival order reaches an output: the order inside a
// cell is removed by the sort, and the brute-force form never reads the bins.
#include <hip/hip_runtime.h>

#include "tsw_nearby.h"

namespace tsw {

namespace {

constexpr uint32_t NB_ITEMS = NB_SCAN_TILE / NB_BLOCK;

// ---- multi-block exclusive scan -------------------------------------------------------------------

__global__ __launch_bounds__(NB_BLOCK) void k_scan_reduce(const uint32_t* data, uint32_t m, uint32_t* bsum) {
  __shared__ uint32_t sh[NB_WAVES];
  const uint64_t base = (uint64_t)blockIdx.x * NB_SCAN_TILE;
  uint32_t s = 0;
#pragma unroll
  for (uint32_t k = 0; k < NB_ITEMS; ++k) {
    const uint64_t p = base + k * NB_BLOCK + threadIdx.x;
    if (p < m) s += data[p];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// exclusive prefix of the nb block sums, one workgroup (nb = m / NB_SCAN_TILE: 512 for a 2^20-cell grid)
__global__ __launch_bounds__(NB_BLOCK) void k_scan_sums(uint32_t* bsum, uint32_t nb) {
  __shared__ uint32_t sh[NB_WAVES];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += NB_BLOCK) {
    const uint32_t p = b0 + threadIdx.x;
    const uint32_t x = p < nb ? bsum[p] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan(x, sh, &total);
    if (p < nb) bsum[p] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(NB_BLOCK) void k_scan_apply(uint32_t* data, uint32_t m, const uint32_t* bsum) {
  __shared__ uint32_t sh[NB_WAVES];
  const uint64_t base = (uint64_t)blockIdx.x * NB_SCAN_TILE + (uint64_t)threadIdx.x * NB_ITEMS;
  uint32_t x[NB_ITEMS];
  uint32_t s = 0;
#pragma unroll
  for (uint32_t k = 0; k < NB_ITEMS; ++k) {
    x[k] = base + k < m ? data[base + k] : 0u;
    s += x[k];
  }
  uint32_t total;
  const uint32_t before = bsum ? bsum[blockIdx.x] : 0u;  // nullptr: the one-tile scan, nothing before it
  uint32_t run = before + block_excl_scan(s, sh, &total);
  // block_excl_scan ended on a barrier: every load of this tile is done before its first store, so the
  // scan is in place (data[m], written below, is loaded by no one: p < m above)
#pragma unroll
  for (uint32_t k = 0; k < NB_ITEMS; ++k) {
    if (base + k < m) data[base + k] = run;
    run += x[k];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) data[m] = before + total;
}

// ---- 1. bins --------------------------------------------------------------------------------------

__global__ __launch_bounds__(NB_BLOCK) void k_nb_hist(NearbyArgs A) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  if (i < A.n) A.rank[i] = atomicAdd(&A.cell_start[A.v[i]], 1u);
}

// the diamond's cells of row yy around (x, y): [*lo, *hi] as indices into cell_start (hi exclusive)
__device__ __forceinline__ void row_range(int x, int y, int yy, int r, int W, uint32_t* lo, uint32_t* hi) {
  const int d = yy > y ? yy - y : y - yy;
  const int half = r - d;
  const int x0 = x - half > 0 ? x - half : 0;
  const int x1 = x + half < W - 1 ? x + half : W - 1;
  *lo = (uint32_t)(yy * W + x0);
  *hi = (uint32_t)(yy * W + x1 + 1);
}

// ---- 2. count -------------------------------------------------------------------------------------

__global__ __launch_bounds__(NB_BLOCK) void k_nb_count(NearbyArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * NB_WAVES + (threadIdx.x >> 6);
  if (i >= A.n) return;  // wave-uniform
  const int W = (int)A.W, H = (int)A.H, r = (int)A.radius;
  const uint32_t c = A.v[i];
  const int x = (int)(c % A.W), y = (int)(c / A.W);
  const int y0 = y - r > 0 ? y - r : 0, y1 = y + r < H - 1 ? y + r : H - 1;
  uint32_t sum = 0;
  for (int yy = y0 + (int)lane; yy <= y1; yy += 64) {
    uint32_t lo, hi;
    row_range(x, y, yy, r, W, &lo, &hi);
    sum += A.cell_start[hi] - A.cell_start[lo];
  }
  sum = wave_sum(sum);  // >= 1: the agent itself
  if (lane == 0) {
    A.sorted[A.cell_start[c] + A.rank[i]] = i;  // the scatter into cell order rides along (read by the fill only)
    A.off[i] = sum - 1u;
    atomicMax(A.maxlen, sum - 1u);
    atomicAdd(A.total64, (unsigned long long)(sum - 1u));
  }
}

// ---- 3. fill --------------------------------------------------------------------------------------

// g, nb_v, nb_g (nb_v == nullptr: lists only): also the lists in tsw_decide's form, nb_v[k] = v[nb_idx[k]],
// nb_g[k] = g[nb_idx[k]]
__global__ __launch_bounds__(NB_BLOCK) void k_nb_fill(NearbyArgs A, uint32_t* __restrict__ nb_idx,
                                                      const uint32_t* __restrict__ g, uint32_t* __restrict__ nb_v,
                                                      uint32_t* __restrict__ nb_g) {
  __shared__ uint32_t buf[NB_WAVES][NB_SORT_MAX];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * NB_WAVES + wave;
  const bool live = i < A.n;  // no early return: every wave reaches the barrier
  uint32_t o = 0, len = 0;
  if (live) {
    const int W = (int)A.W, H = (int)A.H, r = (int)A.radius;
    const uint32_t c = A.v[i];
    const int x = (int)(c % A.W), y = (int)(c / A.W);
    const int y0 = y - r > 0 ? y - r : 0, y1 = y + r < H - 1 ? y + r : H - 1;
    o = A.off[i];
    len = A.off[i + 1] - o;
    uint32_t base = 0;
    for (int c0 = y0; c0 <= y1; c0 += 64) {  // wave-uniform trip count
      const int yy = c0 + (int)lane;
      uint32_t a = 0, cnt = 0, keep = 0;
      if (yy <= y1) {
        uint32_t lo, hi;
        row_range(x, y, yy, r, W, &lo, &hi);
        a = A.cell_start[lo];
        cnt = A.cell_start[hi] - a;
        keep = cnt - (yy == y ? 1u : 0u);  // the agent's own row holds the agent itself once
      }
      const uint32_t incl = wave_incl_scan(keep, lane);
      uint32_t w = base + incl - keep;
      for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t e = A.sorted[a + k];
        if (e != i && w < NB_SORT_MAX) buf[wave][w++] = e;
      }
      base += __shfl(incl, 63);
    }
  }
  __syncthreads();
  if (!live) return;
  if (len > NB_SORT_MAX) len = NB_SORT_MAX;  // not reached: the host takes this kernel only for maxlen <= NB_SORT_MAX
  // rank sort: the indices of one list are distinct, so the rank of an entry is its final place
  for (uint32_t p = lane; p < len; p += 64u) {
    const uint32_t e = buf[wave][p];
    uint32_t rank = 0;
    for (uint32_t k = 0; k < len; ++k) rank += buf[wave][k] < e ? 1u : 0u;
    nb_idx[o + rank] = e;
    if (nb_v) {
      nb_v[o + rank] = A.v[e];
      nb_g[o + rank] = g[e];
    }
  }
}

// ordered brute force: lanes stride over j = 0 .. n-1, ballot + mbcnt compaction (ascending by construction)
__global__ __launch_bounds__(NB_BLOCK) void k_nb_brute(NearbyArgs A, uint32_t* __restrict__ nb_idx,
                                                       const uint32_t* __restrict__ g, uint32_t* __restrict__ nb_v,
                                                       uint32_t* __restrict__ nb_g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * NB_WAVES + (threadIdx.x >> 6);
  if (i >= A.n) return;  // wave-uniform
  const uint32_t c = A.v[i];
  const int x = (int)(c % A.W), y = (int)(c / A.W), r = (int)A.radius;
  const uint32_t o = A.off[i], len = A.off[i + 1] - o;
  uint32_t base = 0;
  for (uint32_t j0 = 0; j0 < A.n; j0 += 64u) {
    const uint32_t j = j0 + lane;
    bool in = false;
    uint32_t cj = 0;
    if (j < A.n && j != i) {
      cj = A.v[j];
      const int dx = (int)(cj % A.W) - x, dy = (int)(cj / A.W) - y;
      in = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= r;
    }
    const unsigned long long mask = __ballot(in);
    const uint32_t pre =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (in && base + pre < len) {
      nb_idx[o + base + pre] = j;
      if (nb_v) {
        nb_v[o + base + pre] = cj;
        nb_g[o + base + pre] = g[j];
      }
    }
    base += (uint32_t)__popcll(mask);
  }
}

// ---- around k_decide ------------------------------------------------------------------------------

__global__ __launch_bounds__(NB_BLOCK) void k_fleet_finish(uint32_t n, const uint32_t* nb_off, const uint32_t* nb_idx,
                                                           uint32_t* partner, const uint32_t* npart,
                                                           const uint32_t* part_in, const uint32_t* part_off,
                                                           uint32_t* part_out, uint32_t part_cap) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t o0 = nb_off[i];
  const uint32_t p = partner[i];
  if (p != 0xFFFFFFFFu) partner[i] = nb_idx[o0 + p];
  if (part_off[n] <= part_cap) {  // else the caller's buffer is too small: it gets part_off alone
    const uint32_t np = npart[i], dst = part_off[i];
    const uint32_t* src = part_in + o0 + i;
    for (uint32_t k = 0; k < np; ++k) part_out[dst + k] = nb_idx[o0 + src[k]];
  }
}

inline dim3 blocks_for(uint64_t items, uint32_t per_block) { return dim3((uint32_t)((items + per_block - 1) / per_block)); }

}  // namespace

hipError_t launch_exclusive_scan(uint32_t* data, uint32_t m, uint32_t* bsum, hipStream_t s) {
  if (m == 0) return hipMemsetAsync(data, 0, 4, s);
  const uint32_t nb = (uint32_t)nb_scan_blocks(m);
  if (nb == 1) {  // one tile: the apply pass alone
    hipLaunchKernelGGL(k_scan_apply, dim3(1), dim3(NB_BLOCK), 0, s, data, m, (const uint32_t*)nullptr);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(NB_BLOCK), 0, s, data, m, bsum);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(NB_BLOCK), 0, s, bsum, nb);
  hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(NB_BLOCK), 0, s, data, m, bsum);
  return hipGetLastError();
}

hipError_t launch_nearby_count(const NearbyArgs& A, hipStream_t s) {
  const uint32_t ncell = A.W * A.H;
  hipError_t e;
  // one memset: [total64 (2 words), maxlen, pad] sit right in front of cell_start
  uint32_t* head = reinterpret_cast<uint32_t*>(A.total64);
  if (A.maxlen != head + 2 || A.cell_start != head + 4) return hipErrorInvalidValue;
  if ((e = hipMemsetAsync(head, 0, ((size_t)ncell + 5) * 4, s)) != hipSuccess) return e;
  if (A.n) hipLaunchKernelGGL(k_nb_hist, blocks_for(A.n, NB_BLOCK), dim3(NB_BLOCK), 0, s, A);
  if ((e = launch_exclusive_scan(A.cell_start, ncell, A.bsum, s)) != hipSuccess) return e;
  if (A.n) hipLaunchKernelGGL(k_nb_count, blocks_for(A.n, NB_WAVES), dim3(NB_BLOCK), 0, s, A);
  if ((e = launch_exclusive_scan(A.off, A.n, A.bsum, s)) != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_nearby_fill(const NearbyArgs& A, uint32_t maxlen, uint32_t* nb_idx, const uint32_t* g,
                              uint32_t* nb_v, uint32_t* nb_g, hipStream_t s) {
  if (A.n == 0) return hipSuccess;
  if (maxlen <= NB_SORT_MAX)
    hipLaunchKernelGGL(k_nb_fill, blocks_for(A.n, NB_WAVES), dim3(NB_BLOCK), 0, s, A, nb_idx, g, nb_v, nb_g);
  else
    hipLaunchKernelGGL(k_nb_brute, blocks_for(A.n, NB_WAVES), dim3(NB_BLOCK), 0, s, A, nb_idx, g, nb_v, nb_g);
  return hipGetLastError();
}

hipError_t launch_fleet_finish(uint32_t n, const uint32_t* nb_off, const uint32_t* nb_idx, uint32_t* partner,
                               const uint32_t* npart, const uint32_t* part_in, const uint32_t* part_off,
                               uint32_t* part_out, uint32_t part_cap, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fleet_finish, blocks_for(n, NB_BLOCK), dim3(NB_BLOCK), 0, s, n, nb_off, nb_idx, partner, npart,
                     part_in, part_off, part_out, part_cap);
  return hipGetLastError();
}

}  // namespace tsw
