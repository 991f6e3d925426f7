// tsw_online_host.hip — tsw_plan_mapd_online (include/tswap.h): a MAPD plan whose tasks become visible at
// their release times. The plan runs as k_plan segments (the parts of a plan call, tsw_ctx.h / tsw_plan_host.hip):
// a segment ends on the column before the next release (tsw_online.h has the schedule), the host then makes
// that epoch's tasks live entries of the K4 index (k_task_release, tsw_online.hip), adds them to
// PlanCtl::unused and resumes k_plan at SEC_ASSIGN from the control block it saved. k_plan is the kernel of
// tsw_plan_mapd, unchanged: it stops when t > PlanCtl::max_t and re-reads its whole state at a launch.
// Host code only.
#include "tsw_ctx.h"
#include "tsw_online.h"

namespace tsw {

// Is every agent on its goal? k_plan stops when every visible task is used and every agent is idle, but an
// idle agent may still be walking: a rule-3 swap can hand an agent that rested on its goal the goal of
// another. Only a fleet at rest repeats its column.
static int fleet_at_rest(tsw_ctx* c, uint32_t n, bool* rest) {
  std::vector<uint32_t> vg(2 * (size_t)n);
  if (n) {
    HIPCHK(hipMemcpyAsync(vg.data(), c->d_v, n * 4ull, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipMemcpyAsync(vg.data() + n, c->d_g, n * 4ull, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  *rest = std::equal(vg.begin(), vg.begin() + n, vg.begin() + n);
  return TSW_OK;
}

// The task chains a segment's workers walk: those of the tasks released into it, rel_order[lo .. hi). They are
// queued in release order (plan_tables), so a segment's chains are a window of d_QT; reset_dispatch arms
// qt_count of them at every launch.
static void chain_window(tsw_ctx* c, PlanCall& call, const std::vector<uint32_t>& chain_at, uint32_t lo, uint32_t hi) {
  c->qt_count = 0;
  if (chain_at.empty() || hi <= lo) return;
  c->qt_count = chain_at[hi] - chain_at[lo];
  if (call.dispatched) call.D.W.QT = c->d_QT + chain_at[lo];  // (the first segment's window starts at 0)
}

// A stopped segment's control block as the next launch's: everything kept (t, chase_id, the round and relabel
// counters), the planner back at the top of a timestep.
static PlanCtl resume_ctl(const PlanCtl& k) {
  PlanCtl r = k;
  r.status = PLAN_RUNNING;
  r.section = SEC_ASSIGN;
  r.qcount = 0;
  return r;
}

static int online_impl(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, const uint32_t* release,
                       uint32_t m, uint32_t max_t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T) {
  PlanCall call;
  TRY(plan_validate_index(c, starts, n, tasks, m, max_t, out, goal_out, out_T, &call));
  const OnlineSchedule S = online_schedule(release, m, max_t);
  // The index holds every task (its boxes are static, and a box over a superset of the live points still bounds
  // them); a task not released at 0 starts hidden: its entry taken, its chunk's count without it.
  for (uint32_t j = S.at_zero; j < m; ++j) {
    const uint32_t pos = call.ix.kpos[S.rel_order[j]];
    call.ix.live[pos] = TASK_TAKEN;
    --call.ix.kcnt[pos / 32u];
  }
  if (S.never) {  // a task that is never released is never looked up: no table for its cells
    call.goalset.assign(call.vcell.begin(), call.vcell.end());
    for (uint32_t j = 0; j < m - S.never; ++j) {
      const uint32_t k = S.rel_order[j];
      if (call.pick[k] != CELL_BAD) call.goalset.push_back(call.pick[k]);
      if (call.dlv[k] != CELL_BAD) call.goalset.push_back(call.dlv[k]);
    }
  }
  TRY(plan_upload(c, call));
  if (!S.epochs.empty()) {
    TRY(grow_synced(c, c->d_rel_order, m));
    TRY(grow_synced(c, c->d_pxy, m));
    HIPCHK(hipMemcpyAsync(c->d_rel_order, S.rel_order.data(), m * 4ull, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_pxy, call.pxy.data(), m * 4ull, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  std::vector<uint32_t> chain_at;
  TRY(plan_tables(c, call, S.rel_order.data(), &chain_at));

  PlanCtl ctl{};
  ctl.section = SEC_ASSIGN;
  ctl.unused = S.at_zero;  // released and not yet used: what the index holds as live entries
  ctl.max_t = S.segment_limit(0);
  ctl.chase_id = c->chase_id;
  ctl.move_rounds = c->tun.move_round0;
  // the round counters run on through the segments: the stats take the last segment's totals once
  const uint64_t rule0 = c->st.rule_rounds, move0 = c->st.move_rounds;
  auto segment = [&](const PlanCtl& init, PlanCtl* k) {
    TRY(plan_segment(c, call, init));
    *k = *c->h_ctl;
    c->st.rule_rounds = rule0 + k->rule_rounds;
    c->st.move_rounds = move0 + k->move_rounds;
    return (int)TSW_OK;
  };
  uint32_t* const grec = goal_out ? c->d_grec.p : nullptr;
  plan_phase(c, call, "plan dispatch starts");
  uint32_t T = 0;
  for (uint32_t e = 0;; ++e) {
    chain_window(c, call, chain_at, S.released_lo(e), S.released_hi(e));
    PlanCtl k;
    TRY(segment(ctl, &k));
    // Stopped before the limit: nothing to do for now. A fleet at rest holds its column; one that still moves
    // runs on, a column per launch (k_plan records a timestep before it tests for the end).
    while (k.t <= S.segment_limit(e)) {
      const OnlineNext nx = online_next(S, e, k.t);
      if (nx.hold_from == nx.hold_to) break;
      bool rest = false;
      TRY(fleet_at_rest(c, n, &rest));
      if (rest) break;
      c->qt_count = 0;  // this segment's chains were armed by the launches before
      TRY(segment(resume_ctl(k), &k));
    }
    const OnlineNext nx = online_next(S, e, k.t);
    HIPCHK(launch_rec_hold(c->d_rec, grec, n, nx.hold_from, nx.hold_to, c->s));
    if (nx.done) {
      T = nx.next_t;
      break;
    }
    const OnlineEpoch& ep = S.epochs[e];
    HIPCHK(launch_task_release(c->d_rel_order, ep.lo, ep.hi, c->d_kpos, c->d_pxy, c->d_live, c->d_kcnt, c->s));
    ctl = resume_ctl(k);
    ctl.t = nx.next_t;
    ctl.unused = k.unused + (ep.hi - ep.lo);
    ctl.max_t = S.segment_limit(e + 1u);
  }
  plan_phase(c, call, "plan dispatch done");
  return plan_download(c, call, T, out, goal_out, out_T);
}

}  // namespace tsw

extern "C" {

int tsw_plan_mapd_online(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, const uint32_t* release,
                         uint32_t m, uint32_t max_t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  return online_impl(c, starts, n, tasks, release, m, max_t, out, goal_out, out_T);
}

}  // extern "C"
