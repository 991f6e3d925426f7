// tsw_fleet_mapd.hip — K5c: the task phase and the record of a decentralized MAPD step, in the model
// above tsw_fleet_mapd in include/tswap.h (the state and task management of tswap_mapd, tswap.rs:106-139,
// keyed on v == g, with the decentralized manager's next-of-the-stream dispatch, manager.rs:275-300).
//
//   k_mapd_arrive  one lane per agent: v == g turns TO_PICKUP into TO_DELIVERY (goal = the task's delivery)
//                  and TO_DELIVERY into IDLE; flag[i] = 1 for an agent that is idle now
//   (scan)         launch_exclusive_scan over the flags: idle agent i has rank flag[i] among the idle ones
//   k_mapd_assign  one lane per agent: the sequential loop hands task next + r to the idle agent of rank r
//                  while next + r < m, so lane i takes exactly that task; lane n - 1 writes the new `next`
//                  into the other slot of the pair (the lanes of this launch read the old one)
//   k_mapd_record  one lane per agent, behind the tick: the tsw_rec of column rec_col, the goal and the task;
//                  lane 0 folds the step's stamps into the status word the host reads
// No atomic decides an order: the atomics are maxima of one stamp value.
#include <hip/hip_runtime.h>

#include "tsw_fleet.h"
#include "tsw_fleet_mapd.h"
#include "tsw_nearby.h"

namespace tsw {

namespace {

constexpr uint32_t REC_PICKING = 0u, REC_CARRYING = 1u, REC_DELIVERED = 2u, REC_IDLE = 3u;  // TSW_* of include/tswap.h

__global__ __launch_bounds__(NB_BLOCK) void k_mapd_arrive(FleetMapdArgs A) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  bool moved = false;
  if (i < A.n) {
    uint32_t st = A.st[i];
    if (st != MAPD_IDLE && A.v[i] == A.g[i]) {
      if (st == MAPD_TO_PICKUP) {
        st = MAPD_TO_DELIVERY;
        A.g[i] = A.dlv[A.tk[i]];
      } else {
        st = MAPD_IDLE;
        A.tk[i] = MAPD_NO_TASK;
      }
      A.st[i] = st;
      moved = true;
    }
    A.flag[i] = st == MAPD_IDLE ? 1u : 0u;
  }
  if (__any(moved) && (threadIdx.x & 63u) == 0) atomicMax(&A.words[MAPD_TCHG], A.stamp);  // one per wave
}

__global__ __launch_bounds__(NB_BLOCK) void k_mapd_assign(FleetMapdArgs A) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  bool moved = false, busy = false;
  if (i < A.n) {
    const uint32_t next = A.words[MAPD_NEXT + ((A.stamp - 1u) & 1u)];
    const uint32_t r = A.flag[i], r1 = A.flag[i + 1];
    if (r1 != r) {  // idle, rank r
      const uint64_t k = (uint64_t)next + r;
      if (k < A.m) {
        A.tk[i] = (uint32_t)k;
        A.st[i] = MAPD_TO_PICKUP;
        A.g[i] = A.pick[k];
        moved = busy = true;
      }
    } else {
      busy = true;
    }
    if (i == A.n - 1u)  // r1 = the number of idle agents
      A.words[MAPD_NEXT + (A.stamp & 1u)] = (uint64_t)next + r1 < A.m ? next + r1 : A.m;
  }
  const bool any_moved = __any(moved), any_busy = __any(busy);
  if ((threadIdx.x & 63u) == 0) {  // one per wave
    if (any_moved) atomicMax(&A.words[MAPD_TCHG], A.stamp);
    if (any_busy) atomicMax(&A.words[MAPD_BUSY], A.stamp);
  }
}

__global__ __launch_bounds__(NB_BLOCK) void k_mapd_record(FleetMapdArgs A) {
  const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
  if (i == 0) {
    const uint32_t chg = *A.tick_changed;
    uint32_t s = 0;
    if (A.words[MAPD_TCHG] == A.stamp) s |= MAPD_S_TASK;
    if (chg == FLEET_STUCK) s |= MAPD_S_STUCK;
    else if (chg == A.stamp) s |= MAPD_S_TICK;
    if (A.words[MAPD_BUSY] != A.stamp && A.words[MAPD_NEXT + (A.stamp & 1u)] == A.m) s |= MAPD_S_DONE;
    A.words[MAPD_STATUS] = s;
  }
  if (i >= A.n) return;
  const uint32_t v = A.v[i], g = A.g[i], st = A.st[i];
  const uint32_t y = v / A.W, x = v - y * A.W;
  const uint32_t state =
      st == MAPD_IDLE ? REC_IDLE : st == MAPD_TO_PICKUP ? REC_PICKING : v == g ? REC_DELIVERED : REC_CARRYING;
  const size_t at = (size_t)i * A.rec_stride + A.rec_col;
  A.rec[at] = (unsigned long long)x | (unsigned long long)y << 16 | (unsigned long long)state << 32;
  if (A.g_rec) A.g_rec[at] = g;
  if (A.t_rec) A.t_rec[at] = A.tk[i];
}

inline dim3 blocks_for(uint32_t items) { return dim3((uint32_t)(((uint64_t)items + NB_BLOCK - 1) / NB_BLOCK)); }

}  // namespace

hipError_t launch_fleet_mapd_tasks(const FleetMapdArgs& A, hipStream_t s) {
  if (A.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mapd_arrive, blocks_for(A.n), dim3(NB_BLOCK), 0, s, A);
  hipError_t e = launch_exclusive_scan(A.flag, A.n, A.bsum, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mapd_assign, blocks_for(A.n), dim3(NB_BLOCK), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_fleet_mapd_record(const FleetMapdArgs& A, hipStream_t s) {
  if (A.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mapd_record, blocks_for(A.n), dim3(NB_BLOCK), 0, s, A);
  return hipGetLastError();
}

}  // namespace tsw
