// tsw_plan_dev.h — what every part of the planner kernel k_plan (tsw_plan_kernel.h) stands on: the barrier and
// instrumentation macros, the constants, the wave reductions, the agent / occupancy arrays (Arrays) and the
// next-hop code lookups.
#pragma once
#include <hip/hip_runtime.h>

#include "tsw_astar.h"
#include "tsw_internal.h"
#include "tsw_plan.h"
#include "tsw_worker.h"

// Planner instrumentation (TSW_PLAN_DEBUG, diagnostic build: sub-phase ticks, change tags, wait classes).
// Round 6 note: the helpers below stay out of line (as in rounds 1-5). Force-inlining them all took
// PlanArgs off the stack (0 B scratch) but the fully inlined planner hung in its first rules phase
// whenever an instrumentation branch ran, and in a two-process run without them;
// scripts/exp_lib.sh + hang_probe.py reproduce it.
// The helpers test the switch as PLAN_DBG, a load of PlanArgs::dbg. k_plan reads it once into `kdbg` and hands that to its
// sections: a PlanArgs field load is a vector load the compiler repeats after stores, and the sections test the switch
// at every sub-step. The section macros below (DTAG, PLAN_TICK, SCAN_*) therefore expect kdbg — and P, tid, s_tick,
// s_tp, s_tp2 — in scope under these names.
#define PLAN_DBG (P.dbg != 0u)
// Planner barrier. Built with -DTSW_PBAR (scripts/exp_lib.sh) and run with TSW_PLAN_DEBUG, every barrier
// also leaves per-wave breadcrumbs in the host-visible watchdog words (line reached / passed, barriers
// passed: the watchdog prints them) and checks that all waves arrived at the same one. Round 6: this is
// how the debug-mode hang was read — waves 1-15 kept passing barriers while wave 0's breadcrumbs stopped,
// i.e. wave 0 ran on with an empty EXEC mask.
#ifndef TSW_PBAR
#define PBAR() __syncthreads()
#else
#define PBAR()                                                                                            \
  do {                                                                                                    \
    if (PLAN_DBG) {                                                                                       \
      uint32_t* bid_ = bar_ids();                                                                         \
      if ((threadIdx.x & 63u) == 0u) {                                                                    \
        bid_[threadIdx.x >> 6] = __LINE__;                                                                \
        if (P.hflags)                                                                                     \
          __hip_atomic_store(&P.hflags[HF_BAR_LINE + (threadIdx.x >> 6)], (uint32_t)__LINE__,             \
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);                                \
      }                                                                                                   \
      __syncthreads();                                                                                    \
      if ((threadIdx.x & 63u) == 0u && P.hflags) {                                                        \
        __hip_atomic_store(&P.hflags[HF_BAR_LINE + (threadIdx.x >> 6)], 0x10000u | (uint32_t)__LINE__,    \
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);                                  \
        __hip_atomic_fetch_add(&P.hflags[HF_BAR_COUNT + (threadIdx.x >> 6)], 1u, __ATOMIC_RELAXED,        \
                               __HIP_MEMORY_SCOPE_SYSTEM);                                                \
      }                                                                                                   \
      if (threadIdx.x == 0u) {                                                                            \
        for (uint32_t w_ = 1; w_ < (blockDim.x >> 6); ++w_)                                               \
          if (bid_[w_] != bid_[0] && bid_[16] == 0u) {                                                    \
            bid_[16] = 1u;                                                                                \
            if (P.hflags)                                                                                 \
              __hip_atomic_store(&P.hflags[HF_BAR_MISMATCH], (bid_[0] << 16) | bid_[w_],                  \
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);                            \
            printf("[k_plan] barrier mismatch: wave 0 at line %u, wave %u at line %u\n", bid_[0], w_, bid_[w_]); \
          }                                                                                               \
      }                                                                                                   \
      __syncthreads();                                                                                    \
    } else {                                                                                              \
      __syncthreads();                                                                                    \
    }                                                                                                     \
  } while (0)
#endif

// diagnostics: wall-clock ticks of sub-phases (the TickSlot names of tsw_plan.h, printed by TSW_PLAN_DEBUG)
#define DTAG(k, bits)                                             \
  do {                                                            \
    if (kdbg && P.dtag) atomicOr(&P.dtag[(k)], (uint32_t)(bits)); \
  } while (0)

#define PLAN_TICK(slot)                              \
  do {                                               \
    if (kdbg && tid == 0) {                          \
      const unsigned long long nw_ = wall_clock64(); \
      s_tick[slot] += nw_ - s_tp;                    \
      s_tp = nw_;                                    \
    }                                                \
  } while (0)

// diagnostics: the K4 scan's parts (thread 0's wall clock) and counters, added in place to P.sec_ticks (TK_SCAN_*)
#define SCAN_TICK(slot)                                              \
  do {                                                               \
    if (kdbg && tid == 0 && P.sec_ticks) {                           \
      const unsigned long long nw_ = wall_clock64();                 \
      atomicAdd(&P.sec_ticks[slot], nw_ - s_tp2);                    \
      s_tp2 = nw_;                                                   \
    }                                                                \
  } while (0)
#define SCAN_COUNT(slot, v)                                                              \
  do {                                                                                   \
    if (kdbg && P.sec_ticks) atomicAdd(&P.sec_ticks[slot], (unsigned long long)(v));     \
  } while (0)

namespace tsw {

namespace {

__device__ __forceinline__ uint32_t* bar_ids() {  // PBAR: per-wave barrier line, [16] = reported
  __shared__ uint32_t b[17];
  return b;
}

constexpr uint8_t NHC_DIRTY = 0xFE;  // per-agent next-hop code must be re-looked-up
constexpr uint32_t OCC_NONE = 0xFFFFFFFFu;
constexpr uint32_t OCC_FLAG = 0x80000000u;  // cell holds more than one agent (duplicate starts)
constexpr uint32_t OCC_IDX = 0x7FFFFFFFu;
constexpr uint32_t SUCC_TERM = 0xFFFFFFFFu;
constexpr uint32_t NO_AGENT = 0xFFFFFFFFu;
constexpr uint32_t NO_CELL = 0xFFFFFFFFu;
constexpr uint32_t ABATCH = 16;   // K4: idle agents whose nearest pickups one pass over the tasks computes (a multiple of 4, <= 32)
constexpr uint32_t SCAN_CAP = 64;  // K4: (chunk, agent mask) entries of the scan's LDS list when it lies in s_ap (two words each)
constexpr uint32_t SCAN_GRP = 4;   // K4: list entries a half-wave loads before it compares them
constexpr uint32_t KCH = 32;      // K4: tasks per spatial chunk (PlanArgs::kbox / kcnt), a multiple of 16
constexpr uint32_t KPT = 2;       // K4: chunks per thread whose count and box stay in registers across a batch
constexpr uint32_t LIST_CAP = 1024;  // entries of the kernel's LDS `list` (ASSIGN compaction, changed agents)
// movement-round decision states
constexpr uint8_t DEC_OPEN = 0, DEC_DONE = 1, DEC_STAY = 2, DEC_MOVE = 3, DEC_SWAP = 4;

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t y = __shfl_xor(x, off, 64);
    x = y < x ? y : x;
  }
  return x;
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t y = __shfl_xor(x, off, 64);
    x = y < x ? y : x;
  }
  return x;
}

// Agent / occupancy arrays; the AG / OC template flags place them in LDS at compile time
// (ds_read/ds_write instead of flat accesses) when they fit.
struct Arrays {
  uint32_t* V;     // cell of agent
  uint32_t* G;     // goal cell of agent
  int32_t* GT;     // goal-table slot of G (goal_tab[G])
  uint32_t* SUCC;  // rules: successor agent; movement: target cell
  uint8_t* NHC;    // next-hop code of (V, G) or NHC_DIRTY
  uint8_t* DEC;    // movement-round state
  uint8_t* ONC;    // rules: agent lies on a cycle of succ
  uint8_t* CANDC;  // rules: next hop of succ(k)'s cell toward k's goal — what succ(k) needs when it takes
                   // k's goal (rule-3 swap, or the rotation of a cycle through both)
  uint32_t* MK;    // rules (wave rounds): lowest batch lane touching each agent, ~0 when clear
  uint32_t* F1;    // rules: pointer-doubling buffers (n + 1 entries, n = terminal sink)
  uint32_t* F2;
  uint32_t* OCC;   // per cell: lowest agent | OCC_FLAG, or OCC_NONE
  uint64_t* MU;    // per cell: (round << 32) | ~(lowest undecided agent targeting it), movement rounds
  uint32_t* MU32;  // the same in LDS (MUL, n < 2^16): round16 << 16 | (0xFFFF - agent), round16 in [1, 65535]
  uint32_t* LIVE;  // K4: pickup points in Morton order, TASK_TAKEN once assigned (PlanArgs::live)
  unsigned long long t0;  // wall clock at the launch (coop: "no worker has started" is measured from here)
};

// Next-hop code of (v, goal slot tab). A plain load may return a stale PENDING from this XCD's L2
// after a worker has stored the code (coop mode): then the word is read again at agent scope, so a
// code that is already known does not send the planner through a refresh pass and a wait. Codes never
// change once written, so either read is exact.
__device__ __forceinline__ uint8_t nh_code_at(const uint8_t* nh, uint64_t nstride, bool coop, int32_t tab, uint32_t v) {
  const uint8_t* p = nh + (uint64_t)tab * nstride + v;
  uint8_t c = *p;
  if (coop && (c == NH_PENDING || c == NH_PENDING_S)) {
    const uint32_t w = __hip_atomic_load(reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3u),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c = (uint8_t)(w >> (8u * (uint32_t)((uintptr_t)p & 3u)));
  }
  return c;
}
__device__ __forceinline__ uint8_t nh_code(const PlanArgs& P, int32_t tab, uint32_t v) {
  return nh_code_at(P.nh, P.nstride, P.coop != 0u, tab, v);
}

// next-hop code of agent k for its current (v, g); -1 unresolved, -2 goal has no table
__device__ __forceinline__ int lookup_code(const PlanArgs& P, const Arrays& S, uint32_t k) {
  const uint8_t c = S.NHC[k];
  if (c <= NH_STAY) return c;
  const int32_t tab = S.GT[k];
  if (tab < 0) return -2;
  const uint8_t code = nh_code(P, tab, S.V[k]);
  if (code <= NH_STAY) {
    S.NHC[k] = code;
    return code;
  }
  return -1;
}

__device__ void occ_rescan(const PlanArgs& P, const Arrays& S, uint32_t cell) {
  uint32_t lowest = OCC_NONE, cnt = 0;
  for (uint32_t k = 0; k < P.n; ++k)
    if (S.V[k] == cell) {
      if (cnt == 0) lowest = k;
      ++cnt;
    }
  S.OCC[cell] = cnt == 0 ? OCC_NONE : (lowest | (cnt > 1 ? OCC_FLAG : 0u));
}

// succ(k) = lowest-index agent at next(k) (position(), tswap.rs:192/223), or TERM when k is at
// its goal, its next cell is empty, or its next hop is not resolved yet (caller checks).
__device__ __forceinline__ uint32_t succ_of(const PlanArgs& P, const Arrays& S, uint32_t k) {
  const uint32_t v = S.V[k];
  if (v == S.G[k]) return SUCC_TERM;
  const uint8_t c = S.NHC[k];
  if (c > NH_STAY) return SUCC_TERM;
  const uint32_t o = S.OCC[step_cell(v, c, P.W)];
  return o == OCC_NONE ? SUCC_TERM : (o & OCC_IDX);
}

// what a section tells the section loop: go round again (the next section, or this one resumed), or leave it
enum SecNext : int { SEC_LOOP = 0, SEC_LEAVE = 1 };

}  // namespace

}  // namespace tsw
