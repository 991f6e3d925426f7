// tsw_astar.hip — K3: the exact get_path() next hop (tswap.rs:288-390) as host-launched kernels, Rust
// std BinaryHeap sift semantics restated (tsw_astar.h):
//   k_astar_lds   grids of <= 1024 cells, one query per lane, heap in LDS.
//   k_astar       one query per lane, heap and g-scores in global memory (the last tier).
//   k_astar_wave  grids of > 1024 cells, one query per wave, heap (and g-scores, where they fit) in LDS;
//                 its sizes are tsw_place.h's wave_* functions.
// The coop workers inside the plan dispatch (tsw_worker.h) run the same device functions. The lone-lane
// core of k_astar_wave (TSW_ASTAR_SERIAL) exists in the diagnostic build only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tsw_internal.h"
#include "tsw_launch.h"
#include "tsw_astar.h"

namespace tsw {


// ----------------------------------------------------------------------------
// K3 (small grids, ncell <= 1024): the same exact A*, heap in LDS.
// Heap entry u32: f:11 | g:10 | cell:11 (key = entry >> 11, same order as above);
// each lane's heap is interleaved with its block-mates (element i of lane t at
// i*BLK + t), so lanes touching equal heap depths never share an LDS bank.
// g_score u16 per cell in HBM/L2 per slot: tag:4 | label:2 | g:10.
// A query whose heap would exceed HCAP is handed to k_astar via the overflow list.
// ----------------------------------------------------------------------------
constexpr uint32_t LDS_HCAP = 128;
constexpr uint32_t LDS_BLK = 256;

__device__ __forceinline__ void lheap_sift_up(uint32_t* Hs, uint32_t t, uint32_t pos, uint32_t elem) {
  const uint32_t k = elem >> 11;
  while (pos > 0) {
    const uint32_t parent = (pos - 1u) >> 1;
    const uint32_t pe = Hs[parent * LDS_BLK + t];
    if (k >= (pe >> 11)) break;
    Hs[pos * LDS_BLK + t] = pe;
    pos = parent;
  }
  Hs[pos * LDS_BLK + t] = elem;
}

__device__ __forceinline__ uint32_t lheap_pop(uint32_t* Hs, uint32_t t, uint32_t& len) {
  const uint32_t end = --len;
  const uint32_t last = Hs[end * LDS_BLK + t];
  if (end == 0) return last;
  const uint32_t top = Hs[t];
  uint32_t pos = 0, child = 1;
  while (child + 1u < end) {
    uint32_t l = Hs[child * LDS_BLK + t];
    const uint32_t r = Hs[(child + 1) * LDS_BLK + t];
    if ((l >> 11) >= (r >> 11)) {
      ++child;
      l = r;
    }
    Hs[pos * LDS_BLK + t] = l;
    pos = child;
    child = 2u * pos + 1u;
  }
  if (child == end - 1u) {
    Hs[pos * LDS_BLK + t] = Hs[child * LDS_BLK + t];
    pos = child;
  }
  lheap_sift_up(Hs, t, pos, last);
  return top;
}

__global__ void __launch_bounds__(LDS_BLK) k_astar_lds(DevGrid G, const AstarQuery* __restrict__ Q, uint32_t nq,
                                                        uint8_t* __restrict__ nh_base, uint64_t nstride,
                                                        uint8_t* __restrict__ res, int32_t* __restrict__ lens,
                                                        uint16_t* __restrict__ gs_all, uint32_t* __restrict__ epochs,
                                                        uint32_t nslots, AstarQuery* __restrict__ ovf,
                                                        uint32_t* __restrict__ novf, uint32_t* __restrict__ qnext) {
  __shared__ uint32_t Hs[LDS_HCAP * LDS_BLK];
  const uint32_t t = threadIdx.x;
  const uint32_t slot = blockIdx.x * LDS_BLK + t;
  if (slot >= nslots || slot >= nq) return;
  const uint32_t W = G.W, ncell = G.ncell;
  const float invW = 1.0f / (float)W;
  uint16_t* GS = gs_all + (uint64_t)slot * ncell;
  uint32_t ep = epochs[slot];
  // first query static (qi = slot), then dynamic dequeue: query times vary by orders of
  // magnitude, so lanes that finish early take the rest instead of a fixed stride
  for (uint32_t qi = slot; qi < nq; qi = nslots + atomicAdd(qnext, 1u)) {
    if (ep % 15u == 0u && ep > 0u)
      for (uint32_t c = 0; c < ncell; ++c) GS[c] = 0;
    const uint32_t tagw = (ep % 15u + 1u) << 12;
    ++ep;
    const AstarQuery q = Q[qi];
    const uint32_t v = q.v, goal = q.goal;
    const uint32_t vy = fast_div(v, W, invW), vx = v - vy * W;
    const uint32_t gy = fast_div(goal, W, invW), gx = goal - gy * W;
    uint8_t code = NH_STAY;
    int32_t L = 1;
    if (v != goal) {
      GS[v] = (uint16_t)tagw;
      Hs[t] = ((vx > gx ? vx - gx : gx - vx) + (vy > gy ? vy - gy : gy - vy)) << 21 | v;
      uint32_t len = 1;
      bool found = false, overflow = false;
      while (len > 0) {
        const uint32_t e = lheap_pop(Hs, t, len);
        const uint32_t c = e & 0x7FFu, cg = (e >> 11) & 0x3FFu;
        if (c == goal) {
          code = (uint8_t)((GS[goal] >> 10) & 3u);
          L = (int32_t)cg + 1;
          found = true;
          break;
        }
        const uint32_t cy = fast_div(c, W, invW), cx = c - cy * W;
        const uint8_t m = G.nbmask[c];
        const uint32_t labc = (GS[c] >> 10) & 3u;
        const uint32_t tg = cg + 1u;
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          if (!(m & (1u << d))) continue;
          const uint32_t nx = d == 1 ? cx + 1 : (d == 3 ? cx - 1 : cx);
          const uint32_t ny = d == 0 ? cy + 1 : (d == 2 ? cy - 1 : cy);
          const uint32_t nc = ny * W + nx;
          const uint32_t old = GS[nc];
          const uint32_t oldg = ((old & 0xF000u) == tagw) ? (old & 0x3FFu) : 0xFFFFu;
          if (tg < oldg) {
            const uint32_t lab = cg == 0 ? d : labc;
            GS[nc] = (uint16_t)(tagw | (lab << 10) | tg);
            if (len >= LDS_HCAP) {
              overflow = true;
              break;
            }
            const uint32_t h = (nx > gx ? nx - gx : gx - nx) + (ny > gy ? ny - gy : gy - ny);
            lheap_sift_up(Hs, t, len, ((tg + h) << 21) | (tg << 11) | nc);
            ++len;
          }
        }
        if (overflow) break;
      }
      if (overflow) {
        ovf[atomicAdd(novf, 1u)] = q;  // resolved by k_astar (global-memory heap)
        continue;
      }
      if (!found) {
        code = fallback_code(G.nbmask[v], vx, vy, gx, gy);
        L = 2;
      }
    }
    if (res) res[q.out] = code;
    if (lens) lens[q.out] = L;
    if (nh_base && q.tab >= 0) nh_base[(uint64_t)q.tab * nstride + q.v] = code;
  }
  epochs[slot] = ep;
}

__global__ void __launch_bounds__(64) k_astar(DevGrid G, const AstarQuery* __restrict__ Q,
                                              const uint32_t* __restrict__ nq_dev, uint32_t nq_host,
                                              uint8_t* __restrict__ nh_base, uint64_t nstride,
                                              uint8_t* __restrict__ res, int32_t* __restrict__ lens,
                                              uint64_t* __restrict__ heaps, uint32_t hcap,
                                              uint32_t* __restrict__ gs_all, uint32_t* __restrict__ epochs,
                                              uint32_t nslots, uint32_t* __restrict__ err) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nslots) return;
  const uint32_t nq = nq_dev ? *nq_dev : nq_host;
  if (slot >= nq) return;
  uint64_t* Hp = heaps + (uint64_t)slot * hcap;
  uint32_t* GS = gs_all + (uint64_t)slot * G.ncell;
  uint32_t ep = epochs[slot];
  for (uint32_t qi = slot; qi < nq; qi += nslots) {
    if (ep % 1023u == 0u && ep > 0u)
      for (uint32_t c = 0; c < G.ncell; ++c) GS[c] = 0u;
    const uint32_t tag = ep % 1023u + 1u;
    ++ep;
    const AstarQuery q = Q[qi];
    int32_t L = 0;
    const uint8_t code = astar_one(G, q.v, q.goal, tag, Hp, hcap, GS, &L, err);
    if (res) res[q.out] = code;
    if (lens) lens[q.out] = L;
    if (nh_base && q.tab >= 0) nh_base[(uint64_t)q.tab * nstride + q.v] = code;
  }
  epochs[slot] = ep;
}

// astar_one with a BYTE g_score per cell (LDS-resident on grids of up to ~120k cells):
// bit 7 valid | label:2 | h:5 with g = manhattan(start, cell) + 2h (g and the Manhattan
// distance from the start have the same parity on a 4-grid, and g >= it). A g that would
// need h > 31, or a heap longer than hcap, returns NH_UNKNOWN with *len_out = -2 (the caller
// hands the query to the u32 g_score kernel). Same heap, same relaxations, same labels.
__device__ __forceinline__ uint8_t astar_one_b8(const DevGrid& G, uint32_t v, uint32_t goal, uint64_t* Hp,
                                                uint32_t hcap, uint8_t* GB, int32_t* len_out) {
  const uint32_t W = G.W;
  const uint32_t vx = v % W, vy = v / W, gx = goal % W, gy = goal / W;
  if (v == goal) {
    *len_out = 1;
    return NH_STAY;
  }
  uint32_t len = 0;
  GB[v] = 0x80u;
  {
    const uint32_t h0 = (vx > gx ? vx - gx : gx - vx) + (vy > gy ? vy - gy : gy - vy);
    Hp[0] = mk_entry(h0, 0, vx, vy);
    len = 1;
  }
  while (len > 0) {
    const uint64_t e = heap_pop(Hp, len);
    const uint32_t cx = (uint32_t)(e >> 11) & 0x7FFu, cy = (uint32_t)e & 0x7FFu;
    const uint32_t cg = (uint32_t)(e >> 22) & 0x1FFFFFu;
    const uint32_t c = cy * W + cx;
    if (c == goal) {
      *len_out = (int32_t)cg + 1;
      return (uint8_t)((GB[goal] >> 5) & 3u);
    }
    const uint8_t m = G.nbmask[c];
    const uint32_t labc = (GB[c] >> 5) & 3u;
    const uint32_t tg = cg + 1u;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      if (!(m & (1u << d))) continue;
      const uint32_t nx = d == 1 ? cx + 1 : (d == 3 ? cx - 1 : cx);
      const uint32_t ny = d == 0 ? cy + 1 : (d == 2 ? cy - 1 : cy);
      const uint32_t nc = ny * W + nx;
      const uint32_t man = (nx > vx ? nx - vx : vx - nx) + (ny > vy ? ny - vy : vy - ny);
      const uint32_t old = GB[nc];
      const uint32_t oldg = (old & 0x80u) ? man + 2u * (old & 31u) : 0xFFFFFFFFu;
      if (tg < oldg) {
        const uint32_t hh = (tg - man) >> 1;
        if (hh > 31u || len >= hcap) {
          *len_out = -2;
          return NH_UNKNOWN;
        }
        const uint32_t lab = cg == 0 ? d : labc;
        GB[nc] = (uint8_t)(0x80u | (lab << 5) | hh);
        const uint32_t h = (nx > gx ? nx - gx : gx - nx) + (ny > gy ? ny - gy : gy - ny);
        heap_sift_up(Hp, len, mk_entry(tg + h, tg, nx, ny));
        ++len;
      }
    }
  }
  *len_out = 2;
  return fallback_code(G.nbmask[v], vx, vy, gx, gy);
}


// ----------------------------------------------------------------------------
// K3 (grids of > 1024 cells): the same exact A* (astar_one), ONE QUERY PER WAVE with the heap
// in LDS and, when the grid fits (WAVE_GS_LDS_MAX cells), the g_score words in LDS too. The
// planner's lazy mode exits to the host whenever a step needs unresolved next hops, so K3
// runs in many small batches and its latency is the slowest query of a batch: a heap sift
// step here is an LDS round trip instead of a dependent global load. Queries whose heap
// outgrows the LDS heap go to the overflow list (k_astar, global-memory heap).
// ----------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_astar_wave(DevGrid G, const AstarQuery* __restrict__ Q, uint32_t nq,
                                                   uint8_t* __restrict__ nh_base, uint64_t nstride,
                                                   uint8_t* __restrict__ res, int32_t* __restrict__ lens,
                                                   uint32_t hcap, uint32_t gs_lds, uint32_t* __restrict__ gs_all,
                                                   uint32_t* __restrict__ epochs, AstarQuery* __restrict__ ovf,
                                                   uint32_t* __restrict__ novf, uint32_t serial,
                                                   unsigned long long* __restrict__ prof,
                                                   uint32_t* __restrict__ qnext) {
  extern __shared__ __align__(16) uint64_t wsm[];
  uint64_t* Hp = wsm;
  const uint32_t lane = threadIdx.x, ncell = G.ncell;
  // gs_lds: 0 = u32 g_scores in global slots, 1 = u32 in LDS, 2 = bytes in LDS (astar_one_b8)
  // LDS and global g-scores are separate pointers for separate calls (a run-time selected pointer is
  // generic: flat loads on the pop's chain instead of ds_read)
  uint32_t* const GSl = reinterpret_cast<uint32_t*>(wsm + hcap);
  uint32_t* const GSg = gs_all + (uint64_t)blockIdx.x * ncell;
  uint32_t* GS = gs_lds == 1u ? GSl : GSg;
  uint8_t* GB = reinterpret_cast<uint8_t*>(wsm + hcap);
  // free-cell bitmap after the heap and the LDS g_scores (wave_lds_bytes' carve)
  const uint32_t gsb = gs_lds == 1u ? ncell * 4u : gs_lds == 2u ? (ncell + 15u) / 16u * 16u : 0u;
  uint32_t* FB = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(wsm + hcap) + gsb);
  const uint32_t nfw = G.H * G.Ww;
  if (!serial)
    for (uint32_t t = lane; t < nfw; t += 64u) FB[t] = G.freebits[t];
  uint32_t ep = gs_lds ? 0u : epochs[blockIdx.x];
  if (gs_lds == 1u)
    for (uint32_t c = lane; c < ncell; c += 64u) GS[c] = 0u;
  __syncthreads();
  // first query static (qi = block), then dynamic dequeue (lane 0's atomic, read by the whole
  // wave): a batch's query times vary by orders of magnitude, a fixed stride idles waves
  auto next_q = [&](uint32_t qi) -> uint32_t {
    if (!qnext) return qi + gridDim.x;
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(qnext, 1u);
    return gridDim.x + (uint32_t)__builtin_amdgcn_readlane((int)t, 0);
  };
  for (uint32_t qi = blockIdx.x; qi < nq; qi = next_q(qi)) {
    if (gs_lds == 2u) {
      uint4* g4 = reinterpret_cast<uint4*>(GB);
      for (uint32_t c = lane; c < (ncell + 15u) / 16u; c += 64u) g4[c] = make_uint4(0u, 0u, 0u, 0u);
    } else if (ep % 1023u == 0u && ep > 0u) {
      for (uint32_t c = lane; c < ncell; c += 64u) GS[c] = 0u;
      __threadfence_block();
    }
    __syncthreads();
    const uint32_t tag = ep % 1023u + 1u;
    ++ep;
    const AstarQuery q = Q[qi];
    int32_t L = 0;
    uint8_t code = NH_UNKNOWN;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long pr[5] = {0, 0, 0, 0, 0};
    if (!serial && prof) {
      code = gs_lds == 2u   ? astar_wave_par<2, true>(G, q.v, q.goal, tag, Hp, hcap, GSl, GB, FB, &L, pr)
             : gs_lds == 1u ? astar_wave_par<1, true>(G, q.v, q.goal, tag, Hp, hcap, GSl, GB, FB, &L, pr)
                            : astar_wave_par<1, true, 0, false>(G, q.v, q.goal, tag, Hp, hcap, GSg, GB, FB, &L, pr);
    } else if (!serial) {
      code = gs_lds == 2u   ? astar_wave_par<2, false>(G, q.v, q.goal, tag, Hp, hcap, GSl, GB, FB, &L, pr)
             : gs_lds == 1u ? astar_wave_par<1, false>(G, q.v, q.goal, tag, Hp, hcap, GSl, GB, FB, &L, pr)
                            : astar_wave_par<1, false, 0, false>(G, q.v, q.goal, tag, Hp, hcap, GSg, GB, FB, &L, pr);
    }
#ifdef TSW_DIAG
    else if (lane == 0) {  // lone-lane core (TSW_ASTAR_SERIAL A/B, diagnostic build only)
      code = gs_lds == 2u ? astar_wave_core<2>(G, q.v, q.goal, tag, Hp, hcap, GS, GB, &L)
                          : astar_wave_core<1>(G, q.v, q.goal, tag, Hp, hcap, GS, GB, &L);
    }
#endif
    if (prof && lane == 0) {  // TSW_ASTAR_PROF: pops, shader clocks, 100 MHz ticks per query
      prof[8ull * qi + 1] = __builtin_amdgcn_s_memtime() - t0;
      prof[8ull * qi + 2] = __builtin_amdgcn_s_memrealtime() - r0;
      prof[8ull * qi] = pr[0];
      for (int j = 1; j < 5; ++j) prof[8ull * qi + 2 + j] = pr[j];
    }
    if (lane == 0) {
      if (L == -2) {
        ovf[atomicAdd(novf, 1u)] = q;  // heap outgrew LDS: resolved by k_astar
      } else {
        if (res) res[q.out] = code;
        if (lens) lens[q.out] = L;
        if (nh_base && q.tab >= 0) nh_base[(uint64_t)q.tab * nstride + q.v] = code;
      }
    }
  }
  if (!gs_lds && lane == 0) epochs[blockIdx.x] = ep;
}

hipError_t launch_astar(const DevGrid& G, const AstarQuery* Q, const uint32_t* nq_dev, uint32_t nq_host,
                        uint32_t launch_threads, uint8_t* nh_base, uint64_t nstride, uint8_t* res,
                        int32_t* lens, uint64_t* heaps, uint32_t hcap, uint32_t* gs_all, uint32_t* epochs,
                        uint32_t nslots, uint32_t* err, hipStream_t s) {
  if (launch_threads == 0) return hipSuccess;
  const uint32_t th = std::min(launch_threads, nslots);
  const uint32_t grid = (th + 63) / 64;
  hipLaunchKernelGGL(k_astar, dim3(grid), dim3(64), 0, s, G, Q, nq_dev, nq_host, nh_base, nstride, res, lens,
                     heaps, hcap, gs_all, epochs, th, err);
  return hipGetLastError();
}

hipError_t launch_astar_lds(const DevGrid& G, const AstarQuery* Q, uint32_t nq, uint8_t* nh_base, uint64_t nstride,
                            uint8_t* res, int32_t* lens, uint16_t* gs16, uint32_t* epochs, uint32_t nslots,
                            AstarQuery* ovf, uint32_t* novf, uint32_t* qnext, hipStream_t s) {
  if (nq == 0) return hipSuccess;
  const uint32_t th = std::min(nq, nslots);
  const uint32_t grid = (th + LDS_BLK - 1) / LDS_BLK;
  hipLaunchKernelGGL(k_astar_lds, dim3(grid), dim3(LDS_BLK), 0, s, G, Q, nq, nh_base, nstride, res, lens, gs16,
                     epochs, th, ovf, novf, qnext);
  return hipGetLastError();
}

hipError_t launch_astar_wave(const DevGrid& G, const AstarQuery* Q, uint32_t nq, uint8_t* nh_base, uint64_t nstride,
                             uint8_t* res, int32_t* lens, uint32_t* gs_all, uint32_t* epochs, uint32_t nslots,
                             AstarQuery* ovf, uint32_t* novf, uint32_t hcap, bool global_gs, hipStream_t s,
                             uint32_t* qnext, uint32_t diag) {
  if (nq == 0) return hipSuccess;
  const uint32_t gs_lds = global_gs ? 0u : wave_gs_mode(G);
  hcap = hcap ? std::max<uint32_t>(4u, std::min(hcap, WAVE_HCAP)) : WAVE_HCAP;
  hcap = wave_fit_hcap(G, hcap, gs_lds);  // overflowing queries are handed on
  if (hcap < 4u) return hipErrorInvalidValue;
  const size_t lds = wave_lds_bytes(G, hcap, gs_lds);
  const uint32_t grid = std::min(nq, nslots);
  hipError_t e = hipFuncSetAttribute((const void*)k_astar_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const uint32_t serial = (diag & ASTAR_DIAG_SERIAL) ? 1u : 0u;  // A/B and tests: lone-lane core
  unsigned long long* prof = nullptr;
  if (diag & ASTAR_DIAG_PROF) {
    e = hipMalloc(&prof, (size_t)nq * 64u);
    if (e != hipSuccess) return e;
    hipMemsetAsync(prof, 0, (size_t)nq * 64u, s);
  }
  hipLaunchKernelGGL(k_astar_wave, dim3(grid), dim3(64), lds, s, G, Q, nq, nh_base, nstride, res, lens, hcap,
                     gs_lds, gs_all, epochs, ovf, novf, serial, prof, qnext);
  e = hipGetLastError();
  if (prof) {
    std::vector<unsigned long long> h((size_t)nq * 8u);
    hipStreamSynchronize(s);
    hipMemcpy(h.data(), prof, h.size() * 8u, hipMemcpyDeviceToHost);
    hipFree(prof);
    size_t worst = 0;
    for (size_t i = 0; i < nq; ++i)
      if (h[8 * i + 2] > h[8 * worst + 2]) worst = i;
    const unsigned long long* w = &h[8 * worst];
    const double np = (double)std::max(1ull, w[0]);
    fprintf(stderr,
            "[k_astar_wave] nq %u gs_mode %u hcap %u | slowest: pops %llu clocks %llu real_us %.1f -> %.1f clk/pop "
            "(pop %.0f, relax %.0f, push %.0f; %.2f pushes/pop), %.3f us/pop, %.0f MHz\n",
            nq, gs_lds, hcap, w[0], w[1], w[2] / 100.0, w[1] / np, w[3] / np, w[4] / np, w[5] / np, w[6] / np,
            w[2] / 100.0 / np, (double)w[1] / std::max(1.0, w[2] / 100.0));
  }
  return e;
}

}  // namespace tsw
