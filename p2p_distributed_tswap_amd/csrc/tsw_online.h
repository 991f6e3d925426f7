// tsw_online.h — the release schedule of tsw_plan_mapd_online (tsw_online_host.hip): the tasks in release
// order, cut into epochs (one per distinct release time in (0, max_t]); the timestep limit of every k_plan
// segment; and what follows a segment that stopped: the columns to repeat while the fleet has nothing to do,
// the column the next segment starts at, or the end of the run. Plain C++ (no HIP types), so a host compiler
// builds and tests it alone (tests/host/online_main.cpp).
//
// Column t of the plan is produced by iteration t. A task with release time r is visible from iteration r
// on. Segment 0 starts at column 0 with the tasks released at 0; segment e >= 1 starts at column
// epochs[e - 1].t with that epoch's tasks added. Segment e may record columns up to segment_limit(e).
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace tsw {

// The tasks rel_order[lo .. hi) become visible at column t.
struct OnlineEpoch {
  uint32_t t, lo, hi;
};

struct OnlineSchedule {
  std::vector<uint32_t> rel_order;  // every task index, by (release time, index)
  std::vector<OnlineEpoch> epochs;  // the distinct release times in (0, max_t], ascending
  uint32_t at_zero = 0;             // rel_order[0 .. at_zero): released at 0
  uint32_t never = 0;               // the tail of rel_order: release > max_t, never visible
  uint32_t max_t = 0;

  uint32_t segments() const { return (uint32_t)epochs.size() + 1u; }
  // PlanCtl::max_t of segment e: the column before the next release, the call's max_t for the last one
  uint32_t segment_limit(uint32_t e) const { return e < epochs.size() ? epochs[e].t - 1u : max_t; }
  // tasks visible in segment e that were not in the one before: positions [lo, hi) of rel_order
  uint32_t released_lo(uint32_t e) const { return e == 0u ? 0u : epochs[e - 1u].lo; }
  uint32_t released_hi(uint32_t e) const { return e == 0u ? at_zero : epochs[e - 1u].hi; }
};

// release == nullptr: every task is released at 0 (one segment).
inline OnlineSchedule online_schedule(const uint32_t* release, uint32_t m, uint32_t max_t) {
  OnlineSchedule S;
  S.max_t = max_t;
  S.rel_order.resize(m);
  std::iota(S.rel_order.begin(), S.rel_order.end(), 0u);
  if (!release) {
    S.at_zero = m;
    return S;
  }
  std::stable_sort(S.rel_order.begin(), S.rel_order.end(), [&](uint32_t a, uint32_t b) { return release[a] < release[b]; });
  uint32_t j = 0;
  while (j < m && release[S.rel_order[j]] == 0u) ++j;
  S.at_zero = j;
  while (j < m && release[S.rel_order[j]] <= max_t) {
    const uint32_t r = release[S.rel_order[j]], lo = j;
    while (j < m && release[S.rel_order[j]] == r) ++j;
    S.epochs.push_back(OnlineEpoch{r, lo, j});
  }
  S.never = m - j;
  return S;
}

// What follows segment e once k_plan has stopped with `t` columns recorded (PlanCtl::t), either at the
// segment's limit (t == segment_limit(e) + 1) or before it, because every visible task was used and every
// agent idle. Columns [hold_from, hold_to) repeat column hold_from - 1: valid only for a fleet at rest
// (every agent on its goal), which the caller checks before it holds; a fleet still moving runs on instead.
struct OnlineNext {
  uint32_t hold_from, hold_to;  // empty when hold_from == hold_to
  uint32_t next_t;              // done: the plan's column count (*out_T); else the next segment's first column
  bool done;
};

inline OnlineNext online_next(const OnlineSchedule& S, uint32_t e, uint32_t t) {
  const bool last = e >= S.epochs.size();
  if (!last) return OnlineNext{t, S.epochs[e].t, S.epochs[e].t, false};  // (t == epochs[e].t at the limit: no hold)
  if (t > S.max_t || S.never == 0u) return OnlineNext{t, t, t, true};
  // tasks that are never released keep the run alive to the last column
  return OnlineNext{t, S.max_t + 1u, S.max_t + 1u, true};
}

}  // namespace tsw
