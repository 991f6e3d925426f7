// tsw_query.hip — the K3 (A*) query path of the host runtime (tsw_ctx.h): the scratch slots, the query
// queue and the per-query results, the host-launched K3 passes (run_astar) with their error read-back, the
// eager resolution of new tables, and the query entry points of include/tswap.h. Host code only.
#include "tsw_ctx.h"

namespace tsw {

// A* scratch slots (global g-scores + overflow heap, one per K3 wave), allocated for the waves that run:
// `need` slots (0: what a host-launched K3 pass uses, astar_wave_slots), grown on demand, at least 64 and
// at most 4,096 / a 32 GB cap. A coop dispatch asks for exactly its worker waves (C5's
// 2,295 workers x 4.5 MB = 10.3 GB instead of a fixed 20 GB budget).
int ensure_astar_scratch(tsw_ctx* c, uint32_t need) {
  const uint64_t ncell = c->G.ncell;
  const uint32_t hcap = (uint32_t)std::min<uint64_t>(4ull * ncell + 8ull, 1ull << 16);
  const uint64_t per_slot = (uint64_t)hcap * 8ull + ncell * 4ull;
  if (need == 0)
    need = std::max(astar_wave_slots(c->G, c->num_cu, true), astar_wave_slots(c->G, c->num_cu, false));
  const uint64_t cap = std::max<uint64_t>(64, std::min<uint64_t>((32ull << 30) / per_slot, 4096));
  const uint32_t ns = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, 64), cap);
  if (c->d_heaps && ns <= c->nslots) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  c->nslots = 0;
  c->hcap = hcap;
  // the old slots go first, all three (GBs for a coop dispatch): the regrowth's peak is the new set alone
  HIPCHK(c->d_heaps.reset());
  HIPCHK(c->d_gs.reset());
  HIPCHK(c->d_epochs.reset());
  HIPCHK(c->d_heaps.alloc((size_t)ns * c->hcap));
  HIPCHK(c->d_gs.alloc((size_t)ns * ncell));
  // every initialisation goes on the context's (non-blocking) stream: a legacy
  // hipMemset is not ordered before kernels on c->s and recycled memory leaks through
  HIPCHK(hipMemsetAsync(c->d_gs, 0, (size_t)ns * ncell * 4ull, c->s));
  HIPCHK(c->d_epochs.alloc(ns));
  HIPCHK(hipMemsetAsync(c->d_epochs, 0, (size_t)ns * 4ull, c->s));
  c->nslots = ns;
  return TSW_OK;
}

int ensure_queue(tsw_ctx* c, size_t need) { return grow_synced(c, c->d_Q, need); }

static int ensure_res(tsw_ctx* c, size_t need) {
  if (c->d_res.holds(need) && c->d_lens.holds(need)) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  HIPCHK(c->d_res.grow(need));
  HIPCHK(c->d_lens.grow(need));
  return TSW_OK;
}

int check_err(tsw_ctx* c) {
  uint32_t e = 0;
  HIPCHK(hipMemcpyAsync(&c->h_stat->err, &c->d_stat->err, 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  e = c->h_stat->err;
  if (e) {
    char buf[160];
    snprintf(buf, sizeof buf,
             "device error bits 0x%x (1 heap overflow, 2 dist overflow, 4 g overflow, 8 no table, 64 nearby list "
             "of more than 1024 entries)",
             e);
    c->err = buf;
    HIPCHK(hipMemsetAsync(&c->d_stat->err, 0, 4, c->s));
    // ERR_DECIDE_LIST: the list limit tswap.h documents as TSW_EOVERFLOW
    return (e & (ERR_HEAP_OVERFLOW | ERR_DIST_OVERFLOW | ERR_G_OVERFLOW | ERR_DECIDE_LIST)) ? TSW_EOVERFLOW : TSW_EINVAL;
  }
  return TSW_OK;
}

// Run K3 over the queued queries until none are left (eager next hops).
// K3 over nq queued queries (device array Q): LDS-heap kernel on small grids, with the
// global-heap kernel for the few whose heap outgrows LDS; global-heap kernel otherwise.
// res / lens (per-query answers, indexed by AstarQuery::out) only for queues the host filled itself
// (tsw_get_path_next): queues written by k_plan reuse `out` for a diagnostic enqueue timestamp in
// coop mode and are always run with res == lens == nullptr, writing codes into the tables.
int run_astar(tsw_ctx* c, const AstarQuery* Q, uint32_t nq, bool to_tables, uint8_t* res, int32_t* lens) {
  if (nq == 0) return TSW_OK;
  if ((res || lens) && to_tables) RET(TSW_EINVAL, "internal: per-query answers are not table writes");
  TRY(ensure_astar_scratch(c));
  Timer t(c, CAT_ASTAR);
  uint8_t* nh = to_tables ? c->d_nh : nullptr;
  if (astar_lds_ok(c->G)) {
    if (!c->d_gs16 || !c->d_ep16) {
      c->nslots16 = 65536;
      HIPCHK(c->d_gs16.alloc((size_t)c->nslots16 * c->G.ncell));
      HIPCHK(hipMemsetAsync(c->d_gs16, 0, (size_t)c->nslots16 * c->G.ncell * 2, c->s));
      HIPCHK(c->d_ep16.alloc(c->nslots16));
      HIPCHK(hipMemsetAsync(c->d_ep16, 0, (size_t)c->nslots16 * 4, c->s));
    }
    if (nq > c->d_ovf.cap) {
      HIPCHK(hipStreamSynchronize(c->s));
      HIPCHK(c->d_ovf.grow(nq));
    }
    HIPCHK(hipMemsetAsync(&c->d_stat->novf, 0, 4, c->s));
    HIPCHK(hipMemsetAsync(&c->d_stat->qnext, 0, 4, c->s));
    HIPCHK(launch_astar_lds(c->G, Q, nq, nh, c->tstride, res, lens, c->d_gs16, c->d_ep16, c->nslots16, c->d_ovf,
                            &c->d_stat->novf, &c->d_stat->qnext, c->s));
    HIPCHK(hipMemcpyAsync(&c->h_stat->novf, &c->d_stat->novf, 4, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    const uint32_t novf = c->h_stat->novf;
    if (novf)
      HIPCHK(launch_astar(c->G, c->d_ovf, nullptr, novf, novf, nh, c->tstride, res, lens, c->d_heaps, c->hcap,
                          c->d_gs, c->d_epochs, c->nslots, &c->d_stat->err, c->s));
  } else {
    // one query per wave, LDS heap; the g_score slots are shared with k_astar (same tag scheme)
    if (nq > c->d_ovf.cap || !c->d_ovf2) {
      HIPCHK(hipStreamSynchronize(c->s));
      HIPCHK(c->d_ovf.grow(nq));
      HIPCHK(c->d_ovf2.grow(c->d_ovf.cap));
    }
    HIPCHK(hipMemsetAsync(&c->d_stat->novf, 0, 8, c->s));   // novf, novf2
    HIPCHK(hipMemsetAsync(&c->d_stat->qnext, 0, 8, c->s));  // qnext, qnext2
    // g_scores in LDS cap residency (the byte words of a 510x220 grid are 112 KB: one wave per
    // CU). When the batch has more queries than LDS-resident waves, throughput wins: keep only
    // the heap in LDS and the g_scores in the global slots (3-4 waves per CU; wh10k prefix
    // 3.32 -> 2.68 s); a smaller batch is bound by its slowest query, where LDS g_scores are
    // faster per pop. TSW_ASTAR_GLOBAL_GS=0/1 forces either (A/B).
    const int ge = c->tun.astar_global_gs;
    const bool ggs = ge >= 0 ? ge != 0
                             : astar_wave_lds_gs(c->G) && nq > std::min(astar_wave_slots(c->G, c->num_cu), c->nslots);
    const uint32_t slots = std::min(astar_wave_slots(c->G, c->num_cu, ggs), c->nslots);
    HIPCHK(launch_astar_wave(c->G, Q, nq, nh, c->tstride, res, lens, c->d_gs, c->d_epochs, slots, c->d_ovf,
                             &c->d_stat->novf, c->tun.wave_hcap, ggs, c->s, &c->d_stat->qnext, c->tun.astar_diag));
    HIPCHK(hipMemcpyAsync(&c->h_stat->novf, &c->d_stat->novf, 4, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    uint32_t novf = c->h_stat->novf;
    AstarQuery* rest = c->d_ovf;
    if (novf && astar_wave_lds_gs(c->G) && c->tun.astar_tier2) {
      // second tier: g_scores that outgrew the LDS encoding (byte words: detours > 62) move to
      // the global u32 slots while the heap stays in LDS; only heap overflows reach k_astar
      const uint32_t slots2 = std::min(astar_wave_slots(c->G, c->num_cu, true), c->nslots);
      HIPCHK(launch_astar_wave(c->G, c->d_ovf, novf, nh, c->tstride, res, lens, c->d_gs, c->d_epochs, slots2,
                               c->d_ovf2, &c->d_stat->novf2, c->tun.wave_hcap, true, c->s, &c->d_stat->qnext2,
                               c->tun.astar_diag));
      HIPCHK(hipMemcpyAsync(&c->h_stat->novf2, &c->d_stat->novf2, 4, hipMemcpyDeviceToHost, c->s));
      HIPCHK(hipStreamSynchronize(c->s));
      novf = c->h_stat->novf2;
      rest = c->d_ovf2;
    }
    if (novf)
      HIPCHK(launch_astar(c->G, rest, nullptr, novf, novf, nh, c->tstride, res, lens, c->d_heaps, c->hcap,
                          c->d_gs, c->d_epochs, c->nslots, &c->d_stat->err, c->s));
  }
  c->st.astar_queries += nq;
  c->st.astar_launches++;
  return TSW_OK;
}

// Error path after pairs were marked NH_PENDING (queued for a K3 pass that did not complete):
// put every pending code of the store back to NH_UNKNOWN so later calls re-queue them instead of
// waiting on a pass that will never run. Returns rc (the original failure).
int reset_pending_after(tsw_ctx* c, int rc) {
  if (rc == TSW_OK || !c->d_nh || c->tab_count == 0) return rc;
  (void)hipStreamSynchronize(c->s);
  if (launch_reset_pending(c->d_nh, (uint64_t)c->tab_count * c->tstride, c->s) == hipSuccess)
    (void)hipStreamSynchronize(c->s);
  return rc;
}

static int resolve_all_unknown_impl(tsw_ctx* c, const std::vector<uint32_t>& goals, const std::vector<uint32_t>& slots) {
  if (goals.empty()) return TSW_OK;
  TRY(ensure_astar_scratch(c));
  TRY(ensure_tmp(c, goals.size()));
  HIPCHK(hipMemcpyAsync(c->d_tmp_a, goals.data(), goals.size() * 4, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_tmp_b, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, c->s));
  // one queue for every pair of the batch (eager_policy bounds it to 8M): a single K3 launch
  // gives each lane several queries, so the launch is not the longest query times the number
  // of 64k-query batches
  const size_t bound = std::min<size_t>((size_t)goals.size() * c->G.ncell, (size_t)1 << 23);
  TRY(ensure_queue(c, std::max<size_t>({c->d_Q.cap, (size_t)1 << 16, bound})));
  for (int iter = 0; iter < 1000000; ++iter) {
    HIPCHK(hipMemsetAsync(&c->d_stat->qcount, 0, 4, c->s));
    HIPCHK(launch_enqueue_unknown(c->G, c->d_tmp_a, c->d_tmp_b, (uint32_t)goals.size(), c->d_nh, c->tstride,
                                  c->d_Q, &c->d_stat->qcount, (uint32_t)c->d_Q.cap, c->s));
    HIPCHK(hipMemcpyAsync(&c->h_stat->qcount, &c->d_stat->qcount, 4, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    const uint32_t cnt = c->h_stat->qcount;
    if (cnt == 0) break;
    const uint32_t run = (uint32_t)std::min<size_t>(cnt, c->d_Q.cap);
    TRY(run_astar(c, c->d_Q, run, true, nullptr, nullptr));
    TRY(check_err(c));
    if (cnt <= c->d_Q.cap) break;
  }
  return TSW_OK;
}

int resolve_all_unknown(tsw_ctx* c, const std::vector<uint32_t>& goals, const std::vector<uint32_t>& slots) {
  return reset_pending_after(c, resolve_all_unknown_impl(c, goals, slots));
}

bool eager_policy(const tsw_ctx* c, size_t new_tables) {
  if ((c->flags & TSW_F_LAZY_NEXTHOP) || c->resolver) return false;
  if (c->flags & TSW_F_EAGER_NEXTHOP) return true;
  return c->G.ncell <= 4096 && (uint64_t)new_tables * c->G.ncell <= (8ull << 20);
}

// The K3 pass of an exit-mode planner exit: the exact A* over the queue into the tables, or — with a
// caller resolver (tsw_plan_mapd_resolved) — the queue's pairs handed to the caller and its codes
// written into the tables.
int resolve_queue(tsw_ctx* c, const AstarQuery* Q, uint32_t nq) {
  if (!c->resolver) {
    TRY(run_astar(c, Q, nq, true, nullptr, nullptr));
    return check_err(c);
  }
  if (nq == 0) return TSW_OK;
  std::vector<AstarQuery> q(nq);
  HIPCHK(hipMemcpyAsync(q.data(), Q, (size_t)nq * sizeof(AstarQuery), hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  std::vector<uint32_t> st(nq), gl(nq);
  for (uint32_t i = 0; i < nq; ++i) {
    st[i] = q[i].v;
    gl[i] = q[i].goal;
  }
  std::vector<uint8_t> codes(nq, NH_UNKNOWN);
  if (c->resolver(c->resolver_user, nq, st.data(), gl.data(), codes.data()) != 0)
    RET(TSW_EINVAL, "the caller's next-hop resolver failed");
  for (uint32_t i = 0; i < nq; ++i)
    if (codes[i] > NH_STAY) RET(TSW_EINVAL, "the caller's next-hop resolver returned a code > 4");
  TRY(ensure_res(c, nq));
  HIPCHK(hipMemcpyAsync(c->d_res, codes.data(), nq, hipMemcpyHostToDevice, c->s));
  HIPCHK(launch_put_codes(Q, nq, c->d_res, c->d_nh, c->tstride, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  c->st.astar_queries += nq;
  return TSW_OK;
}

}  // namespace tsw

extern "C" {

int next_hop_codes_impl(tsw_ctx* c, const uint32_t* start, const uint32_t* goal, uint32_t k, uint8_t* code) {
  for (uint32_t i = 0; i < k; ++i)
    if (!cell_id_ok(c, start[i]) || !cell_id_ok(c, goal[i])) RET(TSW_EINVAL, "query cell off-grid or blocked");
  std::vector<uint32_t> goals(goal, goal + k);
  std::sort(goals.begin(), goals.end());
  goals.erase(std::unique(goals.begin(), goals.end()), goals.end());
  TRY(ensure_tables(c, goals, true));
  std::vector<AstarQuery> q;
  q.reserve(k);
  for (uint32_t i = 0; i < k; ++i) {
    if (start[i] == goal[i]) {
      code[i] = NH_STAY;
      continue;
    }
    q.push_back(AstarQuery{start[i], goal[i], c->h_goal_tab[goal[i]], i});
  }
  if (q.empty()) return TSW_OK;
  const uint32_t nq = (uint32_t)q.size();
  TRY(ensure_queue(c, nq));
  TRY(ensure_res(c, nq));
  std::vector<uint8_t> res(nq);
  for (int pass = 0; pass < 2; ++pass) {
    HIPCHK(hipMemcpyAsync(c->d_Q, q.data(), (size_t)nq * sizeof(AstarQuery), hipMemcpyHostToDevice, c->s));
    HIPCHK(launch_gather_codes(c->d_Q, nq, c->d_nh, c->tstride, c->d_res, c->s));
    HIPCHK(hipMemcpyAsync(res.data(), c->d_res, nq, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    std::vector<AstarQuery> miss;
    for (uint32_t i = 0; i < nq; ++i)
      if (res[i] > NH_STAY) miss.push_back(q[i]);
    if (miss.empty()) break;
    if (pass == 1) RET(TSW_EINVAL, "next hop left unresolved by K3");
    // the exact A* into the tables (the store keeps them for later calls)
    HIPCHK(hipMemcpyAsync(c->d_Q, miss.data(), miss.size() * sizeof(AstarQuery), hipMemcpyHostToDevice, c->s));
    TRY(run_astar(c, c->d_Q, (uint32_t)miss.size(), true, nullptr, nullptr));
    TRY(check_err(c));
  }
  for (uint32_t i = 0; i < nq; ++i) code[q[i].out] = res[i];
  return TSW_OK;
}

int tsw_next_hop_codes(tsw_ctx* c, const uint32_t* start, const uint32_t* goal, uint32_t k, uint8_t* code) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!start || !goal || !code) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  const int rc = reset_pending_after(c, next_hop_codes_impl(c, start, goal, k, code));
  resolve_timing(c);
  return rc;
}

int tsw_get_path_next(tsw_ctx* c, const uint32_t* start, const uint32_t* goal, uint32_t k, uint32_t* next,
                      int32_t* len) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!start || !goal || !next || !len) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  std::vector<AstarQuery> q;
  q.reserve(k);
  for (uint32_t i = 0; i < k; ++i) {
    if (!cell_id_ok(c, start[i]) || !cell_id_ok(c, goal[i])) RET(TSW_EINVAL, "query cell off-grid or blocked");
    if (start[i] == goal[i]) {
      next[i] = start[i];
      len[i] = 1;
      continue;
    }
    AstarQuery a;
    a.v = start[i];
    a.goal = goal[i];
    a.tab = -1;
    a.out = i;
    q.push_back(a);
  }
  if (q.empty()) return TSW_OK;
  TRY(ensure_astar_scratch(c));
  TRY(ensure_queue(c, q.size()));
  TRY(ensure_res(c, k));
  HIPCHK(hipMemcpyAsync(c->d_Q, q.data(), q.size() * sizeof(AstarQuery), hipMemcpyHostToDevice, c->s));
  TRY(run_astar(c, c->d_Q, (uint32_t)q.size(), false, c->d_res, c->d_lens));
  std::vector<uint8_t> res(k);
  std::vector<int32_t> lens(k);
  HIPCHK(hipMemcpyAsync(res.data(), c->d_res, k, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(lens.data(), c->d_lens, k * 4ull, hipMemcpyDeviceToHost, c->s));
  TRY(check_err(c));
  for (const auto& a : q) {
    const uint8_t code = res[a.out];
    uint32_t nx = a.v;
    switch (code) {
      case 0: nx = a.v + c->G.W; break;
      case 1: nx = a.v + 1; break;
      case 2: nx = a.v - c->G.W; break;
      case 3: nx = a.v - 1; break;
      default: nx = a.v; break;
    }
    next[a.out] = nx;
    len[a.out] = lens[a.out];
  }
  resolve_timing(c);
  return TSW_OK;
}

}  // extern "C"
