// tsw_timeline.h — host-callable launch wrappers for the kernels in tsw_timeline.hip (K8: the task timeline
// of plan records, in the definitions above tsw_task_timeline in include/tswap.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tsw_place.h"

namespace tsw {

constexpr uint32_t TL_NTASK = 4u;  // TSW_TL_NTASK of include/tswap.h: agent, t_assign, t_carry, t_deliver
constexpr uint32_t TL_NONE = 0xFFFFFFFFu;
constexpr unsigned long long TL_NOKEY = ~0ull;  // no (t, agent): keys are t << 32 | agent

// One byte per (column, agent) of the column-major event table pass A hands to pass B (ev[t * n + i]): what
// the transition of agent i into column t asks of the replay.
enum : uint8_t { TL_EV_NONE = 0, TL_EV_TAKE = 1, TL_EV_STAY = 2, TL_EV_BAD = 3 };
// colflag[t]: the events column t holds
constexpr uint32_t TL_COL_TAKE = 1u, TL_COL_STAY = 2u;

// The device's 64-bit words (TimelineArgs::q) and its counters (TimelineArgs::w)
enum : uint32_t { TL_Q_FIRST0 = 0, TL_Q_BOUND = 1, TL_Q_WAIT = 2, TL_Q_SERVICE = 3, TL_Q_CARRY = 4, TL_NQ = 5 };
enum : uint32_t { TL_W_KIND = 0, TL_W_ASSIGNED = 1, TL_W_CARRIED = 2, TL_W_DELIVERED = 3, TL_W_SMIN = 4, TL_W_SMAX = 5,
                  TL_W_LAST = 6, TL_W_SCANNED_LO = 7, TL_W_SCANNED_HI = 8, TL_NW = 10 };

struct TimelineArgs {
  uint32_t n, T, m, rule;
  size_t stride;                  // records per agent row
  const unsigned long long* rec;  // tsw_rec as x | y << 16 | state << 32 | pad << 40, agent-major
  const uint2* starts;            // [n] (x, y), NEAREST only
  const uint32_t* release;        // [m] or nullptr: every task at 0
  const uint32_t* vis;            // [T] tasks with release <= t (NEAREST)
  const uint2* sorted;            // [m] (pxy, k) in release order (NEAREST)
  uint2* live;                    // [m] pass B's candidates: the visible tasks not taken, in no order ...
  uint32_t lds_cap;               // ... of which entries 0 .. lds_cap - 1 live in pass B's dynamic LDS instead
  uint8_t* ev;                    // [T * n] events, written by pass A
  uint32_t* colflag;              // [T] zero before pass A
  unsigned long long* q;          // [TL_NQ]: FIRST0 and BOUND ~0, the sums 0 before pass A
  uint32_t* w;                    // [TL_NW]: KIND and SMIN ~0, the others 0 before pass A
  uint32_t* task;                 // [m * TL_NTASK] all ~0 before pass B
};

hipError_t launch_timeline_events(const TimelineArgs& A, hipStream_t s);  // pass A
hipError_t launch_timeline_replay(const TimelineArgs& A, hipStream_t s);  // pass B
hipError_t launch_timeline_attach(const TimelineArgs& A, hipStream_t s);  // pass C

}  // namespace tsw
