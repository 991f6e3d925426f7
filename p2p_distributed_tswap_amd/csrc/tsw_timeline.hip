// tsw_timeline.hip — K8: the task timeline of plan records (the definitions above tsw_task_timeline in
// include/tswap.h). The replay is sequential in (t, agent) only where tasks are handed out; everything else
// is a fact of one record and its left neighbour. Three passes:
//
//   k_tl_events  pass A, one workgroup per tile of TL_TILE_AGENTS agents x TL_TILE_COLS columns, read like
//                the audit's pass A (lane = column, coalesced). Every transition S(i, t-1) -> S(i, t) becomes
//                one byte of the column-major event table: nothing, a take (dispatch that ends in P), a
//                stay-idle (dispatch that ends in I) or an inconsistency of kind 0. The table is turned
//                through an LDS tile, so pass B reads a column's agents in index order, coalesced: the order
//                of the events is their place in the table, no atomic decides it. Per column the kinds of
//                event it holds (an OR), and the first kind 0 as a minimum of t << 32 | agent.
//   k_tl_replay  pass B, ONE workgroup of TL_B_BLOCK threads: the columns in order, of a column only what
//                its flags ask for. The candidates of rule NEAREST are an unordered array of (pxy, k): a
//                column's releases are appended (the host sorted the tasks by release, so they are a window),
//                a take is a block-wide arg-min of dist << 32 | k — per-lane strided scan, wave reduction,
//                one LDS slot per wave, one more reduction — and the winner's entry is overwritten by the
//                last one. The array therefore holds exactly the visible tasks not taken: a take costs
//                O(candidates) and nothing is ever compacted (the minimum does not depend on the order, ties
//                go to the lowest k by the key). Its first lds_cap entries live in LDS (tl_lds_candidates,
//                tsw_place.h), the rest in global memory: a scan is bound by what one CU's lanes can load.
//                The candidate count is the array's length, so kinds 1 and 2 are one comparison per event.
//                Rule STREAM: a take is a counter. Stops at the first inconsistency, pass A's included, and
//                leaves it as the bound.
//   k_tl_attach  pass C, one thread per task that was taken: it walks its agent's row on from t_assign — the
//                P columns, the D run — for t_carry and the run's first TSW_DELIVERED, up to the bound, and
//                adds the task's terms to the sums (integer atomics: sums, minima and maxima).
#include <hip/hip_runtime.h>

#include "tsw_timeline.h"

// the device library's wave-wide minimum (DPP); the HIP headers declare the 64-bit one only with the warp-sync
// builtins enabled
extern "C" __device__ __attribute__((const)) unsigned long long __ockl_wfred_min_u64(unsigned long long);

namespace tsw {

namespace {

constexpr uint32_t TL_A_WAVES = TL_A_BLOCK / 64u, TL_B_WAVES = TL_B_BLOCK / 64u;
static_assert(TL_TILE_COLS == 64u, "pass A: one lane per column of the tile");
static_assert(TL_TILE_AGENTS == 64u, "pass A: one lane per agent of the tile when the transpose is written");
static_assert(TL_B_WAVES <= 64u && (TL_B_WAVES & (TL_B_WAVES - 1u)) == 0u, "pass B: a wave reads every wave's slot, lane & (waves - 1)");

// internal state of a record state (<= 3): 0 I, 1 P, 2 D
__device__ inline uint32_t tl_internal(uint32_t st) { return st == 3u ? 0u : st == 0u ? 1u : 2u; }

__device__ inline uint32_t tl_state(unsigned long long r) { return (uint32_t)(r >> 32) & 0xFFu; }

__device__ inline uint8_t tl_event(uint32_t pst, uint32_t cst) {
  if (cst > 3u) return TL_EV_BAD;
  if (pst > 3u) return TL_EV_NONE;  // behind a kind 0 of the column before: never replayed
  const uint32_t p = tl_internal(pst), c = tl_internal(cst);
  if (p == 1u) return c == 0u ? TL_EV_BAD : TL_EV_NONE;  // P->P, P->D (pass C finds the carry); P->I
  if (c == 2u) return p == 0u ? TL_EV_BAD : TL_EV_NONE;  // I->D; D->D
  return c == 1u ? TL_EV_TAKE : TL_EV_STAY;              // I->I, I->P, D->I, D->P: dispatch
}

__global__ __launch_bounds__(TL_A_BLOCK) void k_tl_events(TimelineArgs A) {
  __shared__ uint8_t s_ev[TL_TILE_COLS][TL_TILE_AGENTS + 4];
  __shared__ uint32_t s_flag[TL_TILE_COLS];
  __shared__ unsigned long long s_first;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i0 = blockIdx.x * TL_TILE_AGENTS, t0 = blockIdx.y * TL_TILE_COLS;
  const uint32_t t = t0 + lane;
  if (threadIdx.x < TL_TILE_COLS) s_flag[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_first = TL_NOKEY;
  __syncthreads();

  uint32_t flag = 0;
  unsigned long long first = TL_NOKEY;
  for (uint32_t a = wave; a < TL_TILE_AGENTS; a += TL_A_WAVES) {
    const uint32_t i = i0 + a;
    if (i >= A.n) break;  // the same for the whole wave
    uint8_t e = TL_EV_NONE;
    if (t < A.T) {
      const unsigned long long* row = A.rec + (size_t)i * A.stride;
      const uint32_t cst = tl_state(row[t]), pst = t > 0 ? tl_state(row[t - 1]) : 3u;  // S(i, -1) = I
      e = tl_event(pst, cst);
      if (e == TL_EV_TAKE) flag |= TL_COL_TAKE;
      if (e == TL_EV_STAY) flag |= TL_COL_STAY;
      if (e == TL_EV_BAD) first = min(first, (unsigned long long)t << 32 | i);
    }
    s_ev[lane][a] = e;
  }
  if (flag) atomicOr(&s_flag[lane], flag);
  if (first != TL_NOKEY) atomicMin(&s_first, first);
  __syncthreads();
  if (threadIdx.x < TL_TILE_COLS && s_flag[threadIdx.x] && t0 + threadIdx.x < A.T)
    atomicOr(&A.colflag[t0 + threadIdx.x], s_flag[threadIdx.x]);
  if (threadIdx.x == 0 && s_first != TL_NOKEY) atomicMin(&A.q[TL_Q_FIRST0], s_first);
  // the transpose: a wave writes one column of the tile, lane = agent
  for (uint32_t c = wave; c < TL_TILE_COLS; c += TL_A_WAVES) {
    const uint32_t tt = t0 + c, i = i0 + lane;
    if (tt < A.T && i < A.n) A.ev[(size_t)tt * A.n + i] = s_ev[c][lane];
  }
}

__global__ __launch_bounds__(TL_B_BLOCK) void k_tl_replay(TimelineArgs A) {
  extern __shared__ uint2 s_live[];  // candidates 0 .. lds_cap - 1; the others are A.live's
  __shared__ uint32_t s_vis[TL_B_BLOCK], s_flag[TL_B_BLOCK];  // of the current TL_B_BLOCK columns
  __shared__ uint32_t s_pos[TL_B_BLOCK];                      // of the current TL_B_BLOCK agents: x | y << 16 before the column
  __shared__ unsigned long long s_take[TL_B_WAVES], s_stay[TL_B_WAVES], s_red[TL_B_WAVES];
  static_assert(sizeof s_vis + sizeof s_flag + sizeof s_pos + sizeof s_take + sizeof s_stay + sizeof s_red == tl_replay_lds_bytes(),
                "tl_lds_candidates leaves room for exactly these");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const bool nearest = A.rule == 0u;
  const unsigned long long first0 = A.q[TL_Q_FIRST0];  // pass A's, complete: the launch before this one
  unsigned long long bound = first0;
  uint32_t kind = first0 != TL_NOKEY ? 0u : TL_NONE;
  // everything below is the same in every thread: the loops, the barriers inside them and the exits
  uint32_t len = 0, vis_end = 0, taken = 0;
  const uint32_t cap = A.lds_cap;  // a multiple of TL_B_BLOCK
  auto candidate = [&](uint32_t j) { return j < cap ? s_live[j] : A.live[j]; };
  auto set_candidate = [&](uint32_t j, uint2 c) {
    if (j < cap) s_live[j] = c;
    else A.live[j] = c;
  };
  unsigned long long scanned = 0;
  bool stop = false;
  for (uint32_t t0 = 0; t0 < A.T && !stop; t0 += TL_B_BLOCK) {
    __syncthreads();  // the columns before have read s_vis and s_flag
    s_vis[tid] = nearest && t0 + tid < A.T ? A.vis[t0 + tid] : 0u;
    s_flag[tid] = t0 + tid < A.T ? A.colflag[t0 + tid] : 0u;
    __syncthreads();
    const uint32_t cols = min(TL_B_BLOCK, A.T - t0);
    for (uint32_t tt = 0; tt < cols && !stop; ++tt) {
      const uint32_t t = t0 + tt;
      if (bound != TL_NOKEY && t > (uint32_t)(bound >> 32)) {
        stop = true;
        break;
      }
      if (nearest && s_vis[tt] > vis_end) {  // this column's releases join the candidates
        const uint32_t nv = s_vis[tt];
        for (uint32_t j = vis_end + tid; j < nv; j += TL_B_BLOCK) set_candidate(len + (j - vis_end), A.sorted[j]);
        len += nv - vis_end;
        vis_end = nv;
      }
      const uint32_t flag = s_flag[tt];
      const uint32_t cand0 = nearest ? len : A.m - taken;
      if (!(flag & TL_COL_TAKE) && !((flag & TL_COL_STAY) && cand0 > 0u)) continue;  // nothing to hand out, nobody wrong
      for (uint32_t i0 = 0; i0 < A.n && !stop; i0 += TL_B_BLOCK) {
        __syncthreads();  // the chunk before has read the masks; the appended candidates are visible
        const uint32_t i = i0 + tid;
        uint8_t e = TL_EV_NONE;
        if (i < A.n && ((unsigned long long)t << 32 | i) < bound) e = A.ev[(size_t)t * A.n + i];
        const unsigned long long mt = __ballot(e == TL_EV_TAKE), ms = __ballot(e == TL_EV_STAY);
        if (lane == 0) {
          s_take[wave] = mt;
          s_stay[wave] = ms;
        }
        if (nearest && e == TL_EV_TAKE) {
          if (t == 0u) {
            const uint2 p = A.starts[i];
            s_pos[tid] = min(p.x, 0xFFFFu) | min(p.y, 0xFFFFu) << 16;
          } else {
            s_pos[tid] = (uint32_t)A.rec[(size_t)i * A.stride + (t - 1u)];
          }
        }
        __syncthreads();
        for (uint32_t w = 0; w < TL_B_WAVES && !stop; ++w) {
          unsigned long long takes = s_take[w], stays = s_stay[w];
          while ((takes | stays) && !stop) {
            const uint32_t cand = nearest ? len : A.m - taken;
            if (!takes && cand == 0u) break;  // the rest of the wave stays idle with nothing to take
            const uint32_t l = (uint32_t)__ffsll((long long)(takes | stays)) - 1u;
            const unsigned long long bit = 1ull << l;
            const uint32_t agent = i0 + w * 64u + l;
            if ((stays & bit) ? cand > 0u : cand == 0u) {
              kind = (stays & bit) ? 2u : 1u;
              bound = (unsigned long long)t << 32 | agent;
              stop = true;
              break;
            }
            if (stays & bit) {
              stays &= ~bit;
              continue;
            }
            takes &= ~bit;
            uint32_t k;
            if (nearest) {
              const uint32_t pos = s_pos[w * 64u + l];
              const int x = (int)(pos & 0xFFFFu), y = (int)(pos >> 16);
              unsigned long long best = TL_NOKEY;
              uint32_t bestj = 0;
              auto look = [&](uint32_t j, uint2 c) {
                const int dx = x - (int)(c.x & 0xFFFFu), dy = y - (int)(c.x >> 16);
                const unsigned long long key = (unsigned long long)(uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) << 32 | c.y;
                if (key < best) {
                  best = key;
                  bestj = j;
                }
              };
              const uint2 last = candidate(len - 1u);  // for the winner's place; loaded with the scan, not after it
              const uint32_t in_lds = min(len, cap);
              for (uint32_t j = tid; j < in_lds; j += TL_B_BLOCK) look(j, s_live[j]);
              for (uint32_t j = cap + tid; j < len; j += TL_B_BLOCK) look(j, A.live[j]);
              const unsigned long long wmin = __ockl_wfred_min_u64(best);  // DPP, no LDS traffic
              if (lane == 0) s_red[wave] = wmin;
              __syncthreads();
              const unsigned long long win = __ockl_wfred_min_u64(s_red[lane & (TL_B_WAVES - 1u)]);  // every wave, all slots
              k = (uint32_t)win;
              // k is in the array once, so one thread holds the winner: the last entry takes its place
              if (best == win && bestj != len - 1u) set_candidate(bestj, last);
              scanned += len;
              --len;
              __syncthreads();  // the array and s_red are free for the next take
            } else {
              k = taken;
            }
            if (tid == 0) {
              A.task[(size_t)k * TL_NTASK + 0] = agent;
              A.task[(size_t)k * TL_NTASK + 1] = t;
            }
            ++taken;
          }
        }
      }
    }
  }
  if (tid == 0) {
    A.q[TL_Q_BOUND] = bound;
    A.w[TL_W_KIND] = kind;
    A.w[TL_W_ASSIGNED] = taken;
    A.w[TL_W_SCANNED_LO] = (uint32_t)scanned;
    A.w[TL_W_SCANNED_HI] = (uint32_t)(scanned >> 32);
  }
}

__global__ __launch_bounds__(TL_C_BLOCK) void k_tl_attach(TimelineArgs A) {
  __shared__ unsigned long long s_sum[3];  // wait, service, carry
  __shared__ uint32_t s_cnt[2];            // carried, delivered
  __shared__ uint32_t s_min, s_max, s_last, s_any;
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    s_min = TL_NONE;
    s_max = s_last = s_any = 0;
  }
  __syncthreads();
  const uint32_t k = blockIdx.x * TL_C_BLOCK + threadIdx.x;
  const unsigned long long bound = A.q[TL_Q_BOUND];
  if (k < A.m) {
    const uint32_t agent = A.task[(size_t)k * TL_NTASK + 0];
    if (agent != TL_NONE) {
      const uint32_t ta = A.task[(size_t)k * TL_NTASK + 1], rel = A.release ? A.release[k] : 0u;
      const unsigned long long* row = A.rec + (size_t)agent * A.stride;
      uint32_t tc = TL_NONE, td = TL_NONE;
      for (uint32_t t = ta + 1u; t < A.T; ++t) {
        if (((unsigned long long)t << 32 | agent) >= bound) break;
        const uint32_t st = tl_state(row[t]);
        if (st > 3u) break;  // (only at the bound)
        const uint32_t s = tl_internal(st);
        if (tc == TL_NONE) {
          if (s == 1u) continue;
          if (s != 2u) break;  // (only at the bound)
          tc = t;
        } else if (s != 2u) {
          break;  // the task is finished
        }
        if (st == 2u) {
          td = t;
          break;
        }
      }
      A.task[(size_t)k * TL_NTASK + 2] = tc;
      A.task[(size_t)k * TL_NTASK + 3] = td;
      atomicAdd(&s_sum[0], (unsigned long long)(ta - rel));
      if (tc != TL_NONE) atomicAdd(&s_cnt[0], 1u);
      if (td != TL_NONE) {
        atomicAdd(&s_cnt[1], 1u);
        atomicAdd(&s_sum[1], (unsigned long long)(td - rel));
        atomicAdd(&s_sum[2], (unsigned long long)(td - tc));
        atomicMin(&s_min, td - rel);
        atomicMax(&s_max, td - rel);
        atomicMax(&s_last, td);
      }
      atomicOr(&s_any, 1u);
    }
  }
  __syncthreads();
  if (!s_any) return;
  if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&A.q[TL_Q_WAIT + threadIdx.x], s_sum[threadIdx.x]);
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&A.w[TL_W_CARRIED + threadIdx.x], s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_cnt[1]) {
    atomicMin(&A.w[TL_W_SMIN], s_min);
    atomicMax(&A.w[TL_W_SMAX], s_max);
    atomicMax(&A.w[TL_W_LAST], s_last);
  }
}

}  // namespace

hipError_t launch_timeline_events(const TimelineArgs& A, hipStream_t s) {
  if (A.n == 0 || A.T == 0) return hipSuccess;
  const dim3 grid(tl_tiles(A.n, TL_TILE_AGENTS), tl_tiles(A.T, TL_TILE_COLS));
  hipLaunchKernelGGL(k_tl_events, grid, dim3(TL_A_BLOCK), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_timeline_replay(const TimelineArgs& A, hipStream_t s) {
  if (A.n == 0 || A.T == 0) return hipSuccess;
  if (A.lds_cap % TL_B_BLOCK) return hipErrorInvalidValue;
  const size_t lds = (size_t)A.lds_cap * sizeof(uint2);
  if (lds) {
    hipError_t e = hipFuncSetAttribute((const void*)k_tl_replay, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_tl_replay, dim3(1), dim3(TL_B_BLOCK), lds, s, A);
  return hipGetLastError();
}

hipError_t launch_timeline_attach(const TimelineArgs& A, hipStream_t s) {
  if (A.n == 0 || A.T == 0 || A.m == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tl_attach, dim3(tl_attach_workgroups(A.m)), dim3(TL_C_BLOCK), 0, s, A);
  return hipGetLastError();
}

}  // namespace tsw
