// tsw_nearby.h — host-callable launch wrappers for the kernels in tsw_nearby.hip (K5: the nearby lists
// of NearbyAgents::get_nearby for a whole fleet, and the index translation around k_decide).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tsw {

// lists of up to this many entries are sorted in LDS (== k_decide's DEC_MAX_LIST); when the count pass
// finds a longer one, every list is built by the ordered brute-force kernel instead
constexpr uint32_t NB_SORT_MAX = 1024;
// elements per workgroup of the multi-block exclusive scan
constexpr uint32_t NB_SCAN_TILE = 2048;
inline size_t nb_scan_blocks(size_t m) { return (m + NB_SCAN_TILE - 1) / NB_SCAN_TILE; }

// ---- device helpers shared by the K5 kernels (tsw_nearby.hip, tsw_fleet.hip) --------------------------
#if defined(__HIPCC__)
constexpr uint32_t NB_BLOCK = 256;                 // threads per workgroup, all kernels
constexpr uint32_t NB_WAVES = NB_BLOCK / 64u;      // agents per workgroup of the wave-per-agent kernels

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// block-wide sum of one value per thread (NB_BLOCK threads), valid in every thread
__device__ __forceinline__ uint32_t block_sum(uint32_t x, uint32_t* sh /*NB_WAVES*/) {
  x = wave_sum(x);
  if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (uint32_t w = 0; w < NB_WAVES; ++w) t += sh[w];
  __syncthreads();
  return t;
}

// block-wide exclusive prefix of one value per thread; *total = the block's sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* sh /*NB_WAVES*/, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(x, lane);
  if (lane == 63u) sh[wave] = incl;
  __syncthreads();
  uint32_t before = 0, t = 0;
#pragma unroll
  for (uint32_t w = 0; w < NB_WAVES; ++w) {
    const uint32_t sw = sh[w];
    if (w < wave) before += sw;
    t += sw;
  }
  __syncthreads();
  *total = t;
  return before + incl - x;
}
#endif  // __HIPCC__

struct NearbyArgs {
  uint32_t W, H, n;
  uint32_t radius;       // clamped to W + H by the caller (a larger one sees the same agents)
  const uint32_t* v;     // [n] agent cells, every one < W * H (checked by the caller)
  uint32_t* cell_start;  // [W*H + 1] per-cell histogram, then its exclusive prefix; == (uint32_t*)total64 + 4
  uint32_t* rank;        // [n] arrival rank of agent i inside its cell (any order: the lists are sorted)
  uint32_t* sorted;      // [n] agent indices in cell order
  uint32_t* off;         // [n + 1] list lengths, then their exclusive prefix (nb_off)
  uint32_t* bsum;        // [max(nb_scan_blocks(W*H), nb_scan_blocks(n))] scan block sums
  uint32_t* maxlen;      // [1] longest list; == (uint32_t*)total64 + 2
  unsigned long long* total64;  // [1] sum of the list lengths without the u32 wrap of off[n]; with maxlen and a
                                // pad word right in front of cell_start, so that one memset clears all three
};

// In-place exclusive prefix of data[0 .. m) over several workgroups (reduce, scan of the block sums,
// apply); data[m] receives the total. bsum: nb_scan_blocks(m) words.
hipError_t launch_exclusive_scan(uint32_t* data, uint32_t m, uint32_t* bsum, hipStream_t s);

// Bins the agents by cell, counts every list and turns the counts into offsets (A.off, A.maxlen, A.total64).
hipError_t launch_nearby_count(const NearbyArgs& A, hipStream_t s);
// Writes the lists (agent indices, ascending inside a list) behind launch_nearby_count's offsets.
// maxlen: the value the count pass left in A.maxlen (picks the LDS-sorted or the brute-force kernel).
// With nb_v != nullptr the same pass also writes the lists in tsw_decide's form: nb_v[k] = v[nb_idx[k]],
// nb_g[k] = g[nb_idx[k]] (g: the agents' goals on the device).
hipError_t launch_nearby_fill(const NearbyArgs& A, uint32_t maxlen, uint32_t* nb_idx, const uint32_t* g,
                              uint32_t* nb_v, uint32_t* nb_g, hipStream_t s);

// k_decide's list indices -> agent indices: partner[i] in place and, when part_off[n] <= part_cap (read on
// the device), agent i's npart[i] participants (k_decide's part layout: nb_off[i] + i ..) into
// part_out[part_off[i] ..)
hipError_t launch_fleet_finish(uint32_t n, const uint32_t* nb_off, const uint32_t* nb_idx, uint32_t* partner,
                               const uint32_t* npart, const uint32_t* part_in, const uint32_t* part_off,
                               uint32_t* part_out, uint32_t part_cap, hipStream_t s);

}  // namespace tsw
