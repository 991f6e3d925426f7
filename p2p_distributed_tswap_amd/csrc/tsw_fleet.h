// tsw_fleet.h — host-callable launch wrappers for the kernels in tsw_fleet.hip (K5b: one decentralized
// tick's decisions applied to the fleet's positions and goals, in the lock-step model of include/tswap.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tsw {

// FleetApplyArgs::changed after a tick whose goal-op rounds did not end (never seen; the host turns it
// into an error instead of waiting on a loop)
constexpr uint32_t FLEET_STUCK = 0xFFFFFFFFu;

struct FleetApplyArgs {
  uint32_t n;
  // the tick's decisions in tsw_decide_fleet's output form, on the device, validated by the caller:
  // partner < n on a swap, participants < n and distinct, at least 2 per rotation
  const uint32_t *act, *cell, *partner, *part_off, *part;
  uint32_t* v;        // [n] positions, updated in place (a Move reads nothing but cell[i])
  uint32_t* g;        // [n] goals, updated in place: G of the model
  uint32_t* g0;       // [n] the tick-start goals, written by the moves kernel, read by the rotations
  uint32_t* owner;    // [n] claim words of the goal-op rounds (the smallest claiming initiator)
  uint32_t* opflag;   // [n + 1] 1 for a swap / rotation initiator, then its exclusive prefix, then the
                      //         fired marks of a round
  uint32_t* ops;      // [2 * n] pending initiators, two lists used in turn
  uint32_t* bsum;     // [nb_scan_blocks(n)] scan block sums
  uint32_t* changed;  // [1] atomicMax'ed with `stamp` by a tick that changes v or g
  uint32_t stamp;     // tick number + 1 (> 0): the caller compares *changed with it, nobody clears it
  // records (nullptr: none): the tick-start state goes into column rec_col of the agent-major arrays
  uint32_t *v_rec, *g_rec;
  uint32_t rec_stride, rec_col;  // words per agent (ticks + 1), this tick's column
};

// One tick: the moves (and the records, the snapshot g0, the initiator flags), the scan of the flags,
// the goal ops in ascending initiator order. Everything on stream s, nothing read back.
hipError_t launch_fleet_apply(const FleetApplyArgs& A, hipStream_t s);
// Column rec_col of the records from the current v and g alone (the state after the last tick).
hipError_t launch_fleet_record(const FleetApplyArgs& A, hipStream_t s);

}  // namespace tsw
