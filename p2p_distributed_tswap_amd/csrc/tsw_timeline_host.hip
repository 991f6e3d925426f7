// tsw_timeline_host.hip — the task timeline in the host runtime (tsw_ctx.h): tsw_task_timeline and
// tsw_task_timeline_device around the three passes of K8 (tsw_timeline.hip). The host's share is what
// tsw_plan_mapd_online's host does for a plan: the tasks in release order (online_schedule), their clamped
// pickup points (task_pxy) and, per column, how many tasks are released by then. The call reads nothing of the
// context but its stream and scratch: the table store, the queues and the stats stay as they were.
// Host code only.
#include "tsw_ctx.h"
#include "tsw_layout.h"
#include "tsw_online.h"
#include "tsw_timeline.h"

extern "C" {

// tasks with release > T - 1 (every task when T == 0)
static uint32_t timeline_unreleased(const uint32_t* release, uint32_t m, uint32_t T) {
  if (T == 0) return m;
  uint32_t u = 0;
  for (uint32_t k = 0; release && k < m; ++k) u += release[k] >= T;
  return u;
}

static void timeline_empty(tsw_timeline* sum, const uint32_t* release, uint32_t m, uint32_t T, uint32_t* task) {
  std::memset(sum, 0, sizeof *sum);
  sum->unreleased = timeline_unreleased(release, m, T);
  sum->service_min = sum->makespan = 0xFFFFFFFFu;
  sum->consistent = 1;
  sum->bad_kind = sum->bad_t = sum->bad_agent = 0xFFFFFFFFu;
  if (task) std::memset(task, 0xFF, (size_t)m * TL_NTASK * 4);
}

// d_rec: the records on the device, agent-major with `stride` records per row
static int timeline_device(tsw_ctx* c, const unsigned long long* d_rec, uint32_t n, uint32_t T, size_t stride,
                           const tsw_point* starts, const tsw_task* tasks, const uint32_t* release, uint32_t m,
                           uint32_t rule, tsw_timeline* sum, uint32_t* task) {
  const bool nearest = rule == TSW_TL_NEAREST;
  // one block of words: everything before L.live comes from the host image below, live is pass B's own
  const TimelineLayout L = timeline_layout(n, m, T, nearest, TL_NQ, TL_NW, TL_NTASK);
  std::vector<uint32_t> h(L.live, 0u);
  std::fill(h.begin() + L.q + 2 * TL_Q_FIRST0, h.begin() + L.q + 2 * TL_Q_BOUND + 2, 0xFFFFFFFFu);
  h[L.w + TL_W_KIND] = h[L.w + TL_W_SMIN] = 0xFFFFFFFFu;
  std::fill(h.begin() + L.task, h.begin() + L.colflag, 0xFFFFFFFFu);
  if (release) std::copy(release, release + m, h.begin() + L.release);
  if (nearest) {
    const OnlineSchedule S = online_schedule(release, m, T - 1u);
    uint32_t j = 0;
    for (uint32_t t = 0; t < T; ++t) {  // vis[t]: tasks with release <= t, a prefix of the release order
      while (j < m && (!release || release[S.rel_order[j]] <= t)) ++j;
      h[L.vis + t] = j;
    }
    for (uint32_t q = 0; q < m; ++q) {
      h[L.sorted + 2 * (size_t)q] = task_pxy(tasks[S.rel_order[q]]);
      h[L.sorted + 2 * (size_t)q + 1] = S.rel_order[q];
    }
    std::memcpy(h.data() + L.starts, starts, (size_t)n * 8);  // tsw_point is two words
  }
  TRY(scratch_grow(c, c->d_tl_w, L.total, "timeline", "tasks and columns"));
  TRY(scratch_grow(c, c->d_tl_ev, (size_t)T * n, "timeline", "events"));
  uint32_t* const d = c->d_tl_w.p;
  TimelineArgs A{};
  A.n = n;
  A.T = T;
  A.m = m;
  A.rule = rule;
  A.stride = stride;
  A.rec = d_rec;
  A.starts = nearest ? reinterpret_cast<const uint2*>(d + L.starts) : nullptr;
  A.release = release ? d + L.release : nullptr;
  A.vis = nearest ? d + L.vis : nullptr;
  A.sorted = nearest ? reinterpret_cast<const uint2*>(d + L.sorted) : nullptr;
  A.live = nearest ? reinterpret_cast<uint2*>(d + L.live) : nullptr;
  A.lds_cap = nearest ? tl_lds_candidates(m, c->max_lds) : 0u;
  A.ev = c->d_tl_ev;
  A.colflag = d + L.colflag;
  A.q = reinterpret_cast<unsigned long long*>(d + L.q);
  A.w = d + L.w;
  A.task = d + L.task;
  HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->s));
  PassTimer<4> pt(c);
  pt.mark(0);
  HIPCHK(launch_timeline_events(A, c->s));
  pt.mark(1);
  HIPCHK(launch_timeline_replay(A, c->s));
  pt.mark(2);
  HIPCHK(launch_timeline_attach(A, c->s));
  pt.mark(3);
  // q | w | task come down together
  HIPCHK(hipMemcpyAsync(h.data(), d, L.colflag * 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  const uint32_t* w = h.data() + L.w;
  unsigned long long q[TL_NQ];
  std::memcpy(q, h.data() + L.q, sizeof q);
  for (int k = 0; k < 3; ++k) c->tl_last[k] = pt.elapsed(k);
  c->tl_last[3] = w[TL_W_ASSIGNED];
  c->tl_last[4] = (double)((unsigned long long)w[TL_W_SCANNED_HI] << 32 | w[TL_W_SCANNED_LO]);

  std::memset(sum, 0, sizeof *sum);
  sum->wait_sum = q[TL_Q_WAIT];
  sum->service_sum = q[TL_Q_SERVICE];
  sum->carry_sum = q[TL_Q_CARRY];
  sum->assigned = w[TL_W_ASSIGNED];
  sum->carried = w[TL_W_CARRIED];
  sum->delivered = w[TL_W_DELIVERED];
  sum->unreleased = timeline_unreleased(release, m, T);
  sum->service_min = w[TL_W_SMIN];
  sum->service_max = w[TL_W_SMAX];
  sum->makespan = sum->delivered ? w[TL_W_LAST] : 0xFFFFFFFFu;
  sum->consistent = q[TL_Q_BOUND] == TL_NOKEY;
  sum->bad_kind = w[TL_W_KIND];
  sum->bad_t = sum->consistent ? 0xFFFFFFFFu : (uint32_t)(q[TL_Q_BOUND] >> 32);
  sum->bad_agent = sum->consistent ? 0xFFFFFFFFu : (uint32_t)q[TL_Q_BOUND];
  if (task) std::memcpy(task, h.data() + L.task, (size_t)m * TL_NTASK * 4);
  return TSW_OK;
}

// what both entry points check before anything is launched; *empty: nothing to replay, the outputs are final
static int timeline_check(tsw_ctx* c, const tsw_rec* rec, uint32_t n, uint32_t T, uint32_t stride, const tsw_point* starts,
                          const tsw_task* tasks, const uint32_t* release, uint32_t m, uint32_t rule, tsw_timeline* sum,
                          uint32_t* task, bool* empty) {
  NOT_FROM_RESOLVER(c);
  if (!sum) RET(TSW_EINVAL, "null sum");
  if (!rec && n > 0 && T > 0) RET(TSW_EINVAL, "null rec");
  if (!tasks && m > 0) RET(TSW_EINVAL, "null tasks");
  if (rule > TSW_TL_STREAM) RET(TSW_EINVAL, "unknown rule");
  if (!starts && rule == TSW_TL_NEAREST && n > 0 && T > 0) RET(TSW_EINVAL, "null starts");
  if (stride < T) RET(TSW_EINVAL, "stride is smaller than T");
  if (T > (1u << 20) + 1u) RET(TSW_EINVAL, "T too large");
  if (release && rule == TSW_TL_STREAM) RET(TSW_EINVAL, "rule STREAM takes no release times");
  *empty = n == 0 || T == 0;
  if (*empty) timeline_empty(sum, release, m, T, task);
  return TSW_OK;
}

int tsw_task_timeline_device(tsw_ctx* c, const tsw_rec* dev_rec, uint32_t n, uint32_t T, uint32_t stride,
                             const tsw_point* starts, const tsw_task* tasks, const uint32_t* release, uint32_t m,
                             uint32_t rule, tsw_timeline* sum, uint32_t* task) {
  if (!c) return TSW_EINVAL;
  bool empty = false;
  TRY(timeline_check(c, dev_rec, n, T, stride, starts, tasks, release, m, rule, sum, task, &empty));
  if (empty) return TSW_OK;
  TRY(set_device(c));
  HIPCHK(hipDeviceSynchronize());  // dev_rec may have been produced on another stream of the caller
  return timeline_device(c, reinterpret_cast<const unsigned long long*>(dev_rec), n, T, stride, starts, tasks, release, m,
                         rule, sum, task);
}

int tsw_task_timeline(tsw_ctx* c, const tsw_rec* rec, uint32_t n, uint32_t T, uint32_t stride, const tsw_point* starts,
                      const tsw_task* tasks, const uint32_t* release, uint32_t m, uint32_t rule, tsw_timeline* sum,
                      uint32_t* task) {
  if (!c) return TSW_EINVAL;
  bool empty = false;
  TRY(timeline_check(c, rec, n, T, stride, starts, tasks, release, m, rule, sum, task, &empty));
  if (empty) return TSW_OK;
  TRY(set_device(c));
  // columns 0 .. T - 1 of every row go up, packed, into the audit's record buffer
  TRY(upload_records(c, rec, n, T, stride, "timeline"));
  return timeline_device(c, c->d_aud_rec, n, T, T, starts, tasks, release, m, rule, sum, task);
}

int tsw_probe_timeline(const tsw_ctx* c, double* out) {
  if (!c || !out) return TSW_EINVAL;
  std::copy(c->tl_last, c->tl_last + 5, out);
  return TSW_OK;
}

}  // extern "C"
