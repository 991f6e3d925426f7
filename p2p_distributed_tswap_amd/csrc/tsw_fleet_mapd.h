// tsw_fleet_mapd.h — host-callable launch wrappers for the kernels in tsw_fleet_mapd.hip (K5c: the task
// phase and the record of a decentralized MAPD step, in the model above tsw_fleet_mapd in include/tswap.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tsw {

// FleetMapdArgs::st
constexpr uint32_t MAPD_IDLE = 0u, MAPD_TO_PICKUP = 1u, MAPD_TO_DELIVERY = 2u;
constexpr uint32_t MAPD_NO_TASK = 0xFFFFFFFFu;

// FleetMapdArgs::words, all zero before step 0
enum : uint32_t {
  MAPD_NEXT = 0,   // [2] tasks handed out so far: step s reads slot s & 1 and writes slot (s + 1) & 1
  MAPD_TCHG = 2,   // atomicMax'ed with `stamp` by a task phase that makes a transition
  MAPD_BUSY = 3,   // atomicMax'ed with `stamp` by a task phase that leaves an agent with a task
  MAPD_STATUS = 4, // the step's MAPD_S_* bits, written by the record kernel
  MAPD_WORDS = 8,
};
// the three facts of the ending decision (and the goal-op rounds' failure mark) in one word
constexpr uint32_t MAPD_S_TASK = 1u;   // stage 1 made a transition
constexpr uint32_t MAPD_S_TICK = 2u;   // the tick changed v or g
constexpr uint32_t MAPD_S_DONE = 4u;   // next == m and every agent IDLE
constexpr uint32_t MAPD_S_STUCK = 8u;  // FleetApplyArgs::changed == FLEET_STUCK

struct FleetMapdArgs {
  uint32_t n, m, W;
  const uint32_t *pick, *dlv;  // [m] pickup / delivery cell of every task (validated by the caller)
  uint32_t *v, *g;             // [n] the resident positions and goals of the run
  uint32_t *st, *tk;           // [n] MAPD_* state, task index or MAPD_NO_TASK
  uint32_t* flag;              // [n + 1] 1 for an agent idle after its arrival transition, then the exclusive prefix
  uint32_t* bsum;              // [nb_scan_blocks(n)] scan block sums
  uint32_t* words;             // [MAPD_WORDS]
  const uint32_t* tick_changed;  // FleetApplyArgs::changed of the step's tick (stamped with the same `stamp`)
  uint32_t stamp;              // step number + 1 (> 0): stamps are compared, never cleared
  // column rec_col of the agent-major records; g_rec / t_rec may be nullptr
  unsigned long long* rec;     // tsw_rec as x | y << 16 | state << 32
  uint32_t *g_rec, *t_rec;
  uint32_t rec_stride, rec_col;
};

// Stage 1 of a step: the arrival transitions, the scan of the idle flags, the dispatch by rank.
hipError_t launch_fleet_mapd_tasks(const FleetMapdArgs& A, hipStream_t s);
// Stage 4 behind the tick's apply: column rec_col of the records and words[MAPD_STATUS].
hipError_t launch_fleet_mapd_record(const FleetMapdArgs& A, hipStream_t s);

}  // namespace tsw
