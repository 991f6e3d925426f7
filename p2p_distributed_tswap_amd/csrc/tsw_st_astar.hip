// tsw_st_astar.hip — K9: astar_with_reservation (src/algorithm/a_star.rs:32-112) for a batch of queries, the
// search over (cell, time) defined above tsw_astar_reserved in include/tswap.h. gfx950 only.
//
// One wavefront per query, ST_WPB of them in a workgroup (tsw_place.h st_astar_config); wave s of the launch
// runs queries s, s + nslots, ... and owns visited table s and overflow heap s, so no wave ever waits for
// another and nothing here is atomic.
//  * Open set: the BinaryHeap of tsw_astar.h (heap_pop / heap_sift_up, the restatement K3 and the host A* run)
//    over entries f:21 | g:21 | x:11 | y:11, worked by lane 0. It starts in the wave's LDS slice and moves to
//    the wave's global heap for good when a push would pass the slice (same array, same order).
//  * A pop's successors: lanes 0-4 look up the reserved vertex (np, nt), lanes 5-9 the reserved edge, lanes
//    10-14 the visited table — direction d = lane % 5 in a_star.rs:40's order — and lane 15 the reserved
//    current cell (pos, nt), all at once: the lookups are dependent global loads and this is where a pop's
//    time goes. One ballot gives the survivors; lane 0 then enters them into the visited table and pushes them
//    in direction order.
//  * The visited word holds the direction a state was entered by (tsw_st_astar.h); at the goal's pop lane 0
//    walks the directions back to the start and writes the path into the query's segment of `seg`.
// Bounds that hold whatever the data: pops <= pushes <= max_nodes, a probe sequence <= the table's slots, the
// walk back <= the path's room. A workgroup-scope fence after a pop's stores orders them before the next pop's
// loads by other lanes of the wave.
#include "tsw_st_astar.h"

#include "tsw_astar.h"
#include "tsw_place.h"
#include "tswap.h"

namespace tsw {

__device__ __forceinline__ void st_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__device__ __forceinline__ void st_astar_query(const StAstarArgs& A, uint32_t q, uint32_t tag, uint64_t* Hl, uint64_t* Hg,
                                               uint64_t* vis, const uint32_t* FB, uint32_t lane) {
  const uint32_t W = A.W, H = A.H, ncell = A.ncell, Ww = A.Ww, vmask = A.vis_mask;
  const uint32_t v = A.start[q], goal = A.goal[q], st = A.start_time[q];
  const uint32_t vy = v / W, vx = v - vy * W, gy = goal / W, gx = goal - gy * W;
  const uint64_t so = A.seg_off[q];
  const uint32_t room = (uint32_t)(A.seg_off[q + 1u] - so);
  uint32_t* const seg = A.seg + so;
  uint64_t* Hp = Hl;
  uint32_t hcap = A.hl;
  bool spilled = false;
  uint32_t len = 1, pushes = 1, pops = 0, status = TSW_SP_NONE, plen = 0;
  if (lane == 0) Hl[0] = mk_entry(st + (vx > gx ? vx - gx : gx - vx) + (vy > gy ? vy - gy : gy - vy), st, vx, vy);
  // lane roles: group 0 vertex (np, nt), 1 edge, 2 visited, each over the five directions; lane 15 the current cell
  const uint32_t grp = lane / ST_NDIR, d = lane - grp * ST_NDIR;
  const uint32_t ddx = st_dx(d), ddy = st_dy(d);
  while (len > 0) {
    uint64_t e = 0;
    if (lane == 0) {
      uint32_t l = len;
      e = heap_pop(Hp, l);
    }
    --len;
    e = rl64(e, 0);
    const uint32_t f = (uint32_t)(e >> 43), g = (uint32_t)(e >> 22) & 0x1FFFFFu;
    const uint32_t x = (uint32_t)(e >> 11) & 0x7FFu, y = (uint32_t)e & 0x7FFu;
    if (f > A.max_time) break;  // the horizon
    ++pops;
    const uint32_t c = y * W + x;
    if (c == goal) {
      if (lane == 0) {
        uint32_t dt = g - st, cur = c;
        status = dt < room ? (uint32_t)TSW_SP_FOUND : ST_SP_INTERNAL;
        if (status == TSW_SP_FOUND) {
          plen = dt + 1u;
          seg[dt] = cur;
          while (dt > 0) {  // <= room steps
            bool found;
            const uint32_t slot = st_vis_find(vis, vmask, tag, (uint64_t)dt * ncell + cur, &found);
            if (!found) {
              status = ST_SP_INTERNAL;
              plen = 0;
              break;
            }
            const uint32_t pd = (uint32_t)vis[slot] & 7u;
            const uint32_t cy = cur / W, cx = cur - cy * W;
            const uint32_t px = cx - st_dx(pd), py = cy - st_dy(pd);
            if (px >= W || py >= H) {  // a direction that leaves the grid: never written by the search
              status = ST_SP_INTERNAL;
              plen = 0;
              break;
            }
            cur = py * W + px;
            seg[--dt] = cur;
          }
        }
      }
      status = rl32(status, 0);
      plen = rl32(plen, 0);
      break;
    }
    const uint32_t nt = g + 1u, dt = nt - st;
    const uint32_t nx = x + ddx, ny = y + ddy;  // unsigned wrap: x - 1 at x = 0 fails the bound test
    const bool inb = lane < 3u * ST_NDIR && nx < W && ny < H;
    const uint32_t fx = inb ? nx : x, fy = inb ? ny : y;
    const uint32_t nc = fy * W + fx;
    const bool ok = inb && ((FB[fy * Ww + (fx >> 5)] >> (fx & 31u)) & 1u);
    bool skip = false;
    uint32_t vslot = 0;
    if (ok) {
      if (grp == 0u) {
        skip = st_res_has(A.res, A.res_mask, st_res_key(nt, nc, ST_KIND_NODE, ncell));
      } else if (grp == 1u) {
        skip = st_res_has(A.res, A.res_mask, st_res_key(nt, c, d, ncell));
      } else {
        vslot = st_vis_find(vis, vmask, tag, (uint64_t)dt * ncell + nc, &skip);
      }
    }
    const bool cur_res = lane == 3u * ST_NDIR && st_res_has(A.res, A.res_mask, st_res_key(nt, c, ST_KIND_NODE, ncell));
    const uint64_t B = ballot64(ok && !skip);
    const bool held = ballot64(cur_res) != 0ull;  // (pos, nt) reserved: no successor at all
    uint32_t surv = held ? 0u : (uint32_t)(B & (B >> ST_NDIR) & (B >> (2u * ST_NDIR))) & 31u;
    bool full = false;
    while (surv) {
      const uint32_t sd = (uint32_t)__builtin_ctz(surv);
      surv &= surv - 1u;
      if (pushes == A.max_nodes) {  // the capacity
        full = true;
        break;
      }
      if (!spilled && len == hcap) {  // the LDS slice is full: the heap moves to the wave's global array
        st_fence();
        for (uint32_t i = lane; i < len; i += 64u) Hg[i] = Hl[i];
        st_fence();
        Hp = Hg;
        hcap = A.max_nodes;
        spilled = true;
      }
      const uint32_t s0 = rl32(vslot, 2u * ST_NDIR + sd) & vmask;
      const uint32_t pc = rl32(nc, sd), px = rl32(fx, sd), py = rl32(fy, sd);
      if (lane == 0) {
        uint32_t i = s0;  // the first empty slot from the lookup's on: an earlier push of this pop may have taken it
        for (uint32_t n = 0; n <= vmask; ++n) {
          if ((uint32_t)(vis[i] >> 46) != tag) break;
          i = (i + 1u) & vmask;
        }
        vis[i] = st_vis_word(tag, (uint64_t)dt * ncell + pc, sd);
        const uint32_t h = (px > gx ? px - gx : gx - px) + (py > gy ? py - gy : gy - py);
        heap_sift_up(Hp, len, mk_entry(nt + h, nt, px, py));
      }
      ++len;
      ++pushes;
    }
    st_fence();
    if (full) {
      status = TSW_SP_CAPACITY;
      break;
    }
  }
  if (lane == 0) {
    A.status[q] = status;
    A.pops[q] = pops;
    A.len[q] = plen;
  }
}

__global__ void __launch_bounds__(ST_WPB * 64u) k_st_astar(StAstarArgs A) {
  extern __shared__ uint64_t st_lds[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t* const Hl = st_lds + (size_t)wave * A.hl;
  const uint32_t* FB = A.freebits;
  if (A.fb_lds) {  // the carve of st_astar_config: the waves' heaps, then the bitmap
    uint32_t* const FBl = reinterpret_cast<uint32_t*>(st_lds + (size_t)A.wpb * A.hl);
    for (uint32_t i = threadIdx.x; i < A.H * A.Ww; i += blockDim.x) FBl[i] = A.freebits[i];
    FB = FBl;
  }
  __syncthreads();
  const uint32_t slot = blockIdx.x * A.wpb + wave;
  if (slot >= A.nslots) return;
  uint64_t* const vis = A.vis + (size_t)slot * ((size_t)A.vis_mask + 1u);
  uint64_t* const Hg = A.gheap + (size_t)slot * A.max_nodes;
  uint32_t tag = A.tag0;
  for (uint64_t q = slot; q < A.k && tag <= ST_TAG_MAX; q += A.nslots, ++tag) {
    st_astar_query(A, (uint32_t)q, tag, Hl, Hg, vis, FB, lane);
    st_fence();
  }
}

hipError_t launch_st_astar(const StAstarArgs& A, size_t lds, hipStream_t s) {
  if (A.wpb == 0u || A.wpb > ST_WPB || A.nslots == 0u) return hipErrorInvalidValue;
  if (lds > 64u * 1024u) {
    hipError_t e = hipFuncSetAttribute((const void*)k_st_astar, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const uint32_t blocks = (A.nslots + A.wpb - 1u) / A.wpb;
  hipLaunchKernelGGL(k_st_astar, dim3(blocks), dim3(A.wpb * 64u), lds, s, A);
  return hipGetLastError();
}

// one wave per query, strided over the grid
__global__ void __launch_bounds__(64) k_st_pack(uint32_t k, const uint64_t* seg_off, const uint32_t* seg,
                                                const uint32_t* path_off, const uint32_t* len, uint32_t* path) {
  for (uint64_t i = blockIdx.x; i < k; i += gridDim.x) {
    const uint32_t* src = seg + seg_off[i];
    uint32_t* dst = path + path_off[i];
    const uint32_t n = len[i];
    for (uint32_t j = threadIdx.x; j < n; j += 64u) dst[j] = src[j];
  }
}

hipError_t launch_st_pack(uint32_t k, const uint64_t* seg_off, const uint32_t* seg, const uint32_t* path_off,
                          const uint32_t* len, uint32_t* path, hipStream_t s) {
  if (k == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_st_pack, dim3(k < 65535u ? k : 65535u), dim3(64), 0, s, k, seg_off, seg, path_off, len, path);
  return hipGetLastError();
}

}  // namespace tsw
