// tsw_fleet.hip — K5b: one decentralized tick's decisions applied on the device, in the lock-step model
// of include/tswap.h (the timer branch and the message handlers of bin/decentralized/agent.rs, agents
// taking their turns in ascending index on the tick-start broadcast v0 / g0).
//
//   k_fleet_moves  one lane per agent: the tick's record column, the snapshot g0, the claim words reset,
//                  the swap / rotation initiators flagged, v1[i] = cell[i] for a Move (reads v0 only)
//   (scan)         launch_exclusive_scan over the flags: initiator i is op number opflag[i]
//   k_fleet_goals  one workgroup. Ops on disjoint agents commute, ops sharing an agent must run in
//                  ascending initiator order. Rounds over the pending ops:
//                    1. every pending op claims the agents it touches: atomicMin(owner[a], initiator)
//                    2. an op that owns all its agents has no smaller pending op on any of them: it fires
//                    3. the claims are cleared, the ops that did not fire are compacted (in order)
//                  The smallest pending op always fires, so a round retires at least one op; the number
//                  of rounds is the longest chain of ops sharing agents. No result depends on the order
//                  in which atomics arrive: a claim word ends a round's step 1 as the minimum.
// One thread handles one op; a rotation's thread walks its participants (rotations are few and short).
#include <hip/hip_runtime.h>

#include "tsw_fleet.h"
#include "tsw_nearby.h"

namespace tsw {

namespace {

constexpr uint32_t ACT_MOVE = 0u, ACT_SWAP = 1u, ACT_ROTATION = 2u;  // TSW_ACT_* of include/tswap.h
constexpr uint32_t NO_OWNER = 0xFFFFFFFFu;

// the claim words are written by atomics of other waves: read and written past the vector L1 too
__device__ __forceinline__ uint32_t owner_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void owner_store(uint32_t* p, uint32_t x) {
  __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NB_BLOCK) void k_fleet_moves(FleetApplyArgs A) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  bool moved = false;
  if (i < A.n) {
    const uint32_t a = A.act[i], v0 = A.v[i], g0 = A.g[i];
    if (A.v_rec) A.v_rec[(size_t)i * A.rec_stride + A.rec_col] = v0;
    if (A.g_rec) A.g_rec[(size_t)i * A.rec_stride + A.rec_col] = g0;
    A.g0[i] = g0;
    A.owner[i] = NO_OWNER;
    A.opflag[i] = (a == ACT_SWAP || a == ACT_ROTATION) ? 1u : 0u;
    if (a == ACT_MOVE) {
      const uint32_t c = A.cell[i];
      if (c != v0) {
        A.v[i] = c;
        moved = true;
      }
    }
  }
  if (__any(moved) && (threadIdx.x & 63u) == 0) atomicMax(A.changed, A.stamp);  // one per wave
}

__global__ __launch_bounds__(NB_BLOCK) void k_fleet_record(FleetApplyArgs A) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  if (i >= A.n) return;
  if (A.v_rec) A.v_rec[(size_t)i * A.rec_stride + A.rec_col] = A.v[i];
  if (A.g_rec) A.g_rec[(size_t)i * A.rec_stride + A.rec_col] = A.g[i];
}

__global__ __launch_bounds__(NB_BLOCK) void k_fleet_goals(FleetApplyArgs A) {
  __shared__ uint32_t sh[NB_WAVES];
  const uint32_t n = A.n, tid = threadIdx.x;
  const uint32_t nops = A.opflag[n];  // the scan's total
  if (nops == 0) return;              // block-uniform: g1 = g0
  uint32_t* cur = A.ops;
  uint32_t* nxt = A.ops + n;
  // the op list in ascending initiator index: op number = exclusive prefix of the flags
  for (uint32_t i = tid; i < n; i += NB_BLOCK) {
    const uint32_t p = A.opflag[i];
    if (A.opflag[i + 1] != p) cur[p] = i;
  }
  __syncthreads();  // the flags are read; opflag[0 .. nops) now holds the rounds' fired marks
  uint32_t np = nops, rounds = 0;
  while (np) {
    if (++rounds > nops) {  // a round retires at least one op; block-uniform
      if (tid == 0) atomicMax(A.changed, FLEET_STUCK);
      return;
    }
    // 1. claims
    for (uint32_t k = tid; k < np; k += NB_BLOCK) {
      const uint32_t i = cur[k];
      if (A.act[i] == ACT_SWAP) {
        atomicMin(&A.owner[i], i);
        atomicMin(&A.owner[A.partner[i]], i);
      } else {
        for (uint32_t m = A.part_off[i], e = A.part_off[i + 1]; m < e; ++m) atomicMin(&A.owner[A.part[m]], i);
      }
    }
    __syncthreads();
    // 2. the ops that own every agent they touch fire
    for (uint32_t k = tid; k < np; k += NB_BLOCK) {
      const uint32_t i = cur[k];
      bool mine;
      if (A.act[i] == ACT_SWAP) {
        const uint32_t j = A.partner[i];
        mine = owner_load(&A.owner[i]) == i && owner_load(&A.owner[j]) == i;
        if (mine) {  // the partner takes the requester's goal and answers with the one it held
          const uint32_t gi = A.g[i];
          A.g[i] = A.g[j];
          A.g[j] = gi;
        }
      } else {
        const uint32_t o = A.part_off[i], len = A.part_off[i + 1] - o;
        mine = true;
        for (uint32_t m = 0; m < len && mine; ++m) mine = owner_load(&A.owner[A.part[o + m]]) == i;
        if (mine)  // the request carries the tick-start goals: g0, not G
          for (uint32_t m = 0; m < len; ++m) A.g[A.part[o + m]] = A.g0[A.part[o + (m + 1 == len ? 0u : m + 1)]];
      }
      A.opflag[k] = mine ? 1u : 0u;
    }
    __syncthreads();
    // 3. claims cleared; the ops that did not fire stay pending, in order
    uint32_t kept = 0;
    for (uint32_t k0 = 0; k0 < np; k0 += NB_BLOCK) {  // block-uniform trip count
      const uint32_t k = k0 + tid;
      uint32_t i = 0, keep = 0;
      if (k < np) {
        i = cur[k];
        keep = A.opflag[k] ? 0u : 1u;
        if (A.act[i] == ACT_SWAP) {
          owner_store(&A.owner[i], NO_OWNER);
          owner_store(&A.owner[A.partner[i]], NO_OWNER);
        } else {
          for (uint32_t m = A.part_off[i], e = A.part_off[i + 1]; m < e; ++m) owner_store(&A.owner[A.part[m]], NO_OWNER);
        }
      }
      uint32_t total;
      const uint32_t ex = block_excl_scan(keep, sh, &total);
      if (keep) nxt[kept + ex] = i;
      kept += total;
    }
    __syncthreads();
    uint32_t* t = cur;
    cur = nxt;
    nxt = t;
    np = kept;
  }
  // g1 != g0 anywhere (ops can cancel, so the writes alone do not tell)
  bool diff = false;
  for (uint32_t a = tid; a < n; a += NB_BLOCK) diff |= A.g[a] != A.g0[a];
  if (__any(diff) && (tid & 63u) == 0) atomicMax(A.changed, A.stamp);
}

inline dim3 blocks_for(uint32_t items) { return dim3((uint32_t)(((uint64_t)items + NB_BLOCK - 1) / NB_BLOCK)); }

}  // namespace

hipError_t launch_fleet_apply(const FleetApplyArgs& A, hipStream_t s) {
  if (A.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fleet_moves, blocks_for(A.n), dim3(NB_BLOCK), 0, s, A);
  hipError_t e = launch_exclusive_scan(A.opflag, A.n, A.bsum, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_fleet_goals, dim3(1), dim3(NB_BLOCK), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_fleet_record(const FleetApplyArgs& A, hipStream_t s) {
  if (A.n == 0 || (!A.v_rec && !A.g_rec)) return hipSuccess;
  hipLaunchKernelGGL(k_fleet_record, blocks_for(A.n), dim3(NB_BLOCK), 0, s, A);
  return hipGetLastError();
}

}  // namespace tsw
