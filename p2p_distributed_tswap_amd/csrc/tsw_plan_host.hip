// tsw_plan_host.hip — the plan runner of the host runtime (tsw_ctx.h): the agent and coop buffers, k_plan's
// arguments, the dispatch loop with its watchdog and the host A* service threads, and the planning entry
// points of include/tswap.h (tsw_plan_mapd*, tsw_step). Host code only.
#include "tsw_ctx.h"

namespace tsw {

// A failed growth leaves acap 0 and every array either whole or empty: the next call allocates again.
static int ensure_agents(tsw_ctx* c, size_t n) {
  if (n <= c->acap && c->d_v) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  size_t cap = std::max<size_t>(n, 64);
  c->acap = 0;
  // the old arrays go first, all of them: the regrowth's peak is the new set alone
  for (auto* b : {&c->d_onc, &c->d_candc, &c->d_st, &c->d_nhc, &c->d_dec}) (void)b->reset();
  for (auto* b : {&c->d_f1, &c->d_f2, &c->d_v, &c->d_g, &c->d_succ, &c->d_ap}) (void)b->reset();
  (void)c->d_gt.reset();
  (void)c->d_task.reset();
  HIPCHK(c->d_onc.alloc(cap));
  HIPCHK(c->d_candc.alloc(cap));
  HIPCHK(c->d_f1.alloc(cap + 1));
  HIPCHK(c->d_f2.alloc(cap + 1));
  HIPCHK(c->d_v.alloc(cap));
  HIPCHK(c->d_g.alloc(cap));
  HIPCHK(c->d_succ.alloc(cap));
  HIPCHK(c->d_gt.alloc(cap));
  HIPCHK(c->d_ap.alloc(cap + 1));
  HIPCHK(c->d_st.alloc(cap));
  HIPCHK(c->d_nhc.alloc(cap));
  HIPCHK(c->d_dec.alloc(cap));
  HIPCHK(c->d_task.alloc(cap));
  if (!c->h_dups) {  // the per-cell arrays, once (h_dups comes last: set only when all five are)
    HIPCHK(c->d_occ.alloc(c->G.ncell));
    HIPCHK(c->d_cnt.alloc(c->G.ncell));
    HIPCHK(c->d_mu.alloc(c->G.ncell));
    HIPCHK(c->d_dups.alloc(1));
    HIPCHK(c->h_dups.alloc(1));
  }
  c->acap = cap;
  c->chase_id = 0;
  return TSW_OK;
}

// Coop-mode buffers: the A* scratch, the needed queue sized for a whole launch, the control block and
// the speculative queue.
static int ensure_coop(tsw_ctx* c, uint32_t n, uint32_t max_t = 0) {
  TRY(ensure_astar_scratch(c));
  // the needed queue is linear over a coop launch too (urgent walk-ahead pairs join it): sized by the plan
  TRY(ensure_queue(c, std::max<size_t>(std::max<size_t>(4 * (size_t)n + 4096, (size_t)1 << 18),
                                       std::min<size_t>((size_t)n * (max_t + 1u) / 8u, (size_t)1 << 25))));
  if (!c->d_cc || !c->h_cc) {
    HIPCHK(c->d_cc.alloc(1));
    HIPCHK(c->h_cc.alloc(1));
  }
  // The speculative queue is linear over a plan launch (the planner appends, the workers claim in
  // order): once it is full the planner stops speculating for the rest of the launch. C5 (10,000 agents,
  // 2,001 steps) queues ~1M pairs, exactly the old fixed 2^20 entries: the queue filled up mid-plan and
  // every later step waited on unprefetched pairs (43 s instead of 8 s). Sized by the plan: half an entry
  // per agent-step, 2^20 .. 2^26 entries (16 MB .. 1 GB of HBM).
  const size_t want_qs = std::min<size_t>(std::max<size_t>((size_t)n * (max_t + 1u) / 2u, (size_t)1 << 20),
                                          (size_t)1 << 26);
  return grow_synced(c, c->d_QS, want_qs);
}

// A per-agent array that k_plan can do without (PlanArgs::dtag / wf / pred): n elements, filled with the
// byte `fill` on the stream; nullptr when the buffer cannot be had.
template <class T>
static T* per_agent(tsw_ctx* c, DevBuf<T>& b, uint32_t n, int fill) {
  if (b.cap < n) (void)b.alloc(n);
  return b.p && hipMemsetAsync(b.p, fill, (size_t)n * sizeof(T), c->s) == hipSuccess ? b.p : nullptr;
}

// What of the planner's state lives in LDS (choose_plan_placement, tsw_place.h), into PlanArgs.
static void choose_plan_lds(const tsw_ctx* c, PlanArgs* P) {
  const PlanPlacement pl =
      choose_plan_placement(P->n, P->ncell, P->m, c->max_lds, c->tun.part_lds, c->tun.flinks_lds, c->tun.occ_split,
                            c->tun.agents_lds);
  P->part_lds = pl.part, P->f_lds = pl.flinks, P->mu_lds = pl.mu;
  P->agents_lds = pl.agents, P->occ_lds = pl.occ, P->tasks_lds = pl.tasks;
}

static PlanArgs plan_args(tsw_ctx* c, uint32_t n, uint32_t m, uint32_t mode, bool want_goals) {
  PlanArgs P{};
  P.n = n;
  P.m = m;
  P.W = c->G.W;
  P.ncell = c->G.ncell;
  P.mode = mode;
  P.v = c->d_v;
  P.g = c->d_g;
  P.st = c->d_st;
  P.task = c->d_task;
  P.gt = c->d_gt;
  P.succ = c->d_succ;
  P.nhc = c->d_nhc;
  P.dec = c->d_dec;
  P.onc = c->d_onc;
  P.candc = c->d_candc;
  P.f1 = c->d_f1;
  P.f2 = c->d_f2;
  P.mk = c->d_ap;
  P.occ = c->d_occ;
  P.mu = c->d_mu;
  P.has_dups = *c->h_dups;
  // speculative next-hop prefetch only pays in lazy mode (eager tables have nothing unresolved)
  P.prefetch = (!c->tun.prefetch || eager_policy(c, 0)) ? 0u : 1u;
  // wide prefetch (default 8 hops; 4 -> 8: wh10k prefix 2.53 -> 2.28 s, 16 gave 2.32 s): every
  // agent's (succ cell, goal) pair, and its path walked this many hops ahead; TSW_WIDE_PREFETCH=0 restores candidates-only / one hop (A/B)
  // wave-0 rules rounds (scan 64 agents per ballot from the cursor, fire in lane 0): firing
  // agents are dense, so a scan rarely needs more than a chunk or two even for 10k agents;
  // TSW_WAVE_RULES_MAX caps n for A/B
  P.wave_rules_max = c->tun.wave_rules_max;
  P.walk_cap = c->tun.walk_cap;
  P.wide_prefetch = c->tun.wide_prefetch;
  P.wide_hi = c->tun.wide_hi ? c->tun.wide_hi : c->tun.wide_prefetch;
  P.wide_lo = c->tun.wide_lo;
  P.spec_hi = 0;  // set per launch from the worker count (worker_args)
  P.dag_prefetch = c->tun.dag_prefetch;
  P.dag_width = c->tun.dag_width;
  P.urgent_hops = c->tun.urgent_hops;
  P.ab_flags = c->tun.ab_flags;
  P.t0_delay_ticks = c->tun.t0_delay_us * 100u;
  P.prefetch_ext = c->tun.prefetch_ext;
  P.dt = c->d_dt;
  P.nbmask = c->d_nbmask;
  P.live = c->d_live;
  P.klt = c->d_klt;
  P.kpos = c->d_kpos;
  P.kbox = c->d_kbox;
  P.kcnt = c->d_kcnt;
  P.kchunks = c->kchunks;
  P.pick = c->d_pick;
  P.dlv = c->d_dlv;
  P.goal_tab = c->d_goal_tab;
  P.nh = c->d_nh;
  P.nstride = c->tstride;
  P.Q = c->d_Q;
  P.qcap = (uint32_t)c->d_Q.cap;
  P.rec = c->d_rec;
  P.grec = want_goals ? c->d_grec : nullptr;
  P.ctl = c->d_ctl;
  P.sec_ticks = c->d_ticks;
  P.dbg = c->tun.plan_debug ? 1u : 0u;
  P.dtag = nullptr;
  if (P.dbg && n) P.dtag = per_agent(c, c->d_dtag, n, 0);  // diagnostics only: per-agent change tags
  P.wf = nullptr;
  // the frontier is re-armed per call, so a tsw_step call (one timestep) could never carry a budgeted walk on
  P.walk_step = mode == MODE_STEP ? 0u : c->tun.walk_step;
  // re-armed per plan / step call (a goal never matches 0xFFFFFFFF)
  if (c->tun.walk_cache && n) P.wf = per_agent(c, c->d_wf, n, 0xFF);
  P.pred = nullptr;
  // diagnostics only: prediction hits
  if (P.dbg && n && mode == MODE_MAPD) P.pred = per_agent(c, c->d_pred, n, 0xFF);
  choose_plan_lds(c, &P);
  // coop mode: lazy next hops only (eager tables have nothing left to resolve)
  P.coop = (c->tun.coop && !c->resolver && P.prefetch && c->d_cc && c->d_QS) ? 1u : 0u;
  P.hflags = c->h_flags.dev;  // watchdog words, both modes
  if (P.coop) {
    P.QS = c->d_QS;
    P.qscap = (uint32_t)c->d_QS.cap;
    P.cc = c->d_cc;
    P.QH = (mode == MODE_MAPD && c->tun.task_chains && c->tun.hot_chains && c->d_QH && m) ? c->d_QH : nullptr;
    P.qhcap = P.QH ? (uint32_t)std::min<size_t>(c->d_QH.cap, m) : 0u;
    P.QP = (P.QH && c->tun.predict && c->d_QP) ? c->d_QP : nullptr;
    P.qpcap = P.QP ? (uint32_t)std::min<size_t>(c->d_QP.cap, 0xFFFFFFFFu) : 0u;
    P.predict = P.QP ? c->tun.predict : 0u;
  }
  if (!P.QP) P.pred = nullptr;
  return P;
}

// Occupancy grid in k_plan encoding + whether any cell holds several agents.
static int build_occ(tsw_ctx* c, uint32_t n) {
  HIPCHK(hipMemsetAsync(c->d_dups, 0, 4, c->s));
  HIPCHK(launch_occ(c->d_v, n, c->d_occ, c->d_cnt, c->G.ncell, c->d_dups, c->s));
  HIPCHK(hipMemcpyAsync(c->h_dups, c->d_dups, 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  return TSW_OK;
}

// ---- host A* service ------------------------------------------------------------------------
// The request ring's next entry, if the planner has written it: claim it (the claim count is the tail
// the planner reads, HF_HOST_TAIL), run the exact A* on this core and write seq << 8 | code into the reply
// slot. Entries are claimed in ticket order by whichever serving thread sees them first. false: nothing
// to serve. A pair the host cannot answer gets no reply: a K3 worker answers it as before.
static bool host_serve_one(tsw_ctx* c, HostAstar& S) {
  const uint32_t mask = c->hring - 1u;
  uint32_t t = __atomic_load_n(&c->h_flags[HF_HOST_TAIL], __ATOMIC_RELAXED);
  const unsigned long long e = __atomic_load_n(&c->h_hreq[t & mask], __ATOMIC_ACQUIRE);
  if ((uint32_t)(e >> 40) != t + 1u) return false;
  if (!__atomic_compare_exchange_n(&c->h_flags[HF_HOST_TAIL], &t, t + 1u, false, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) return true;
  const uint32_t v = (uint32_t)(e >> 20) & 0xFFFFFu, g = (uint32_t)e & 0xFFFFFu;
  if (v >= c->G.ncell || g >= c->G.ncell || !(c->h_nbmask[v] & NB_FREE) || !(c->h_nbmask[g] & NB_FREE)) return true;
  const auto t0 = std::chrono::steady_clock::now();
  const uint8_t code = host_next_hop(S, c->h_nbmask.data(), c->G.W, c->G.H, v, g);
  c->host_busy_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  c->host_queries++;
  if (c->tun.host_delay_us) std::this_thread::sleep_for(std::chrono::microseconds(c->tun.host_delay_us));
  if (code <= NH_STAY) __atomic_store_n(&c->h_hrep[t & mask], ((t + 1u) << 8) | code, __ATOMIC_RELEASE);
  return true;
}

// helper thread k (1..host_threads - 1): parked between dispatches, serving while one runs
static void host_helper(tsw_ctx* c, uint32_t k) {
  auto& hp = c->host_pool;
  uint64_t seen = 0;
  for (;;) {
    {
      std::unique_lock<std::mutex> lk(hp.mu);
      hp.cv.wait(lk, [&] { return hp.quit || hp.epoch != seen; });
      if (hp.quit) return;
      seen = hp.epoch;
    }
    while (hp.active.load(std::memory_order_acquire))
      if (!host_serve_one(c, c->host_scratch[k])) __builtin_ia32_pause();
    hp.running.fetch_sub(1, std::memory_order_release);
  }
}

static void host_service_begin(tsw_ctx* c) {
  auto& hp = c->host_pool;
  const uint32_t helpers = c->host_threads - 1u;
  if (!helpers) return;
  while (hp.th.size() < helpers) hp.th.emplace_back(host_helper, c, (uint32_t)hp.th.size() + 1u);
  hp.running.store((int)helpers, std::memory_order_relaxed);
  hp.active.store(true, std::memory_order_release);
  {
    std::lock_guard<std::mutex> lk(hp.mu);
    ++hp.epoch;
  }
  hp.cv.notify_all();
}

// every helper is parked again when this returns: the rings may be reset for the next dispatch
static void host_service_end(tsw_ctx* c) {
  auto& hp = c->host_pool;
  if (!hp.active.load(std::memory_order_relaxed)) return;
  hp.active.store(false, std::memory_order_release);
  while (hp.running.load(std::memory_order_acquire) > 0) std::this_thread::yield();
}

// ---- the plan dispatch -------------------------------------------------------------------------
// (Dispatch, what one k_plan launch needs beside PlanArgs: tsw_ctx.h.)
// Coop mode: the K3 workers' arguments and their count for a planner block of `block` threads and `lds` bytes.
// Sets P.spec_hi; clears P.coop (exit mode) when nothing fits beside the planner.
static int worker_args(tsw_ctx* c, PlanArgs& P, size_t lds, uint32_t block, WorkerArgs* Wp, uint32_t* wblocks) {
  WorkerArgs& W = *Wp;
  W.G = c->G;
  W.cc = c->d_cc;
  W.QN = c->d_Q;
  W.QS = c->d_QS;
  W.QT = c->d_QT;
  W.QH = c->d_QH;
  W.QP = P.QP;
  W.klive = c->d_live;
  W.klt = c->d_klt;
  W.kbox = c->d_kbox;
  W.kcnt = c->d_kcnt;
  W.kchunks = c->kchunks;
  W.pick = c->d_pick;
  W.dlv = c->d_dlv;
  W.goal_tab = c->d_goal_tab;
  W.pred = P.pred;
  W.nh = c->d_nh;
  W.nstride = c->tstride;
  // every worker may walk task chains: a chain worker serves queued needed / speculative pairs
  // between hops (W.preempt), so chains only use otherwise idle time. Round 4 A/B (chain share 1/4
  // -> all, profiles/r4/chain_share_ab.txt): wh10k 11.58 -> 10.25 s, C5 3.33 -> 2.76 s, C3 unchanged
  // (it was a quarter with many agents, a half otherwise)
  W.tmask = c->tun.chain_mask >= 0 ? (uint32_t)c->tun.chain_mask : 0u;
  W.preempt = c->tun.chain_preempt ? 1u : 0u;
  W.chain_hops = c->tun.chain_hops;
  W.avoid_xcc = c->tun.avoid_xcc ? 1u : 0u;
  W.hflags = c->h_flags.dev;
  const WorkerCfg wcfg =
      worker_config(c->G, c->num_cu, P.n, c->tun.wave_hcap, c->tun.worker_gs, c->tun.dag_exit, lds, c->tun.worker_fb);
  W.dag = wcfg.dag;
  // the test's heap scan gathers D from LDS (detour bytes) or from the u16 table in global memory:
  // every 16 / 64 pops (C3 worker busy -20 %, wh10k 400 steps 5.77 -> 5.42 s; profiles/r3/dag_exit_ab.txt)
  W.dag_mask = c->tun.dag_mask ? c->tun.dag_mask : (W.dag == 1u ? 15u : 63u);
  W.stale_steps = c->tun.stale_steps;
  W.reg_heap = c->tun.reg_heap;
  W.wake_gate = (1u << c->tun.wake_gate) - 1u;
  W.slow_mask = (1u << c->tun.slow_poll) - 1u;
  W.slow_mult = c->tun.slow_mult;
  W.idle_ticks = c->tun.worker_idle_us * 100ull;  // wall clock: 100 MHz
  W.dt = c->d_dt;
  W.gs_lds = wcfg.gs_lds;
  W.stage_fb = wcfg.stage_fb;
  W.hcap = wcfg.hcap;
  const WorkerLayout L = worker_layout(wcfg.lds, lds, block, c->num_cu);
  TRY(ensure_astar_scratch(c, L.want));  // one g-score / heap slot per worker wave
  W.lds_per_wave = L.lds_per_wave;
  W.wpb = L.wpb;
  W.gs_all = c->d_gs;
  W.epochs = c->d_epochs;
  W.heaps = c->d_heaps;
  W.ghcap = c->hcap;
  W.nworkers = L.nworkers(c->nslots);
  P.spec_hi = 2u * W.nworkers;  // a backlog of two pairs per worker counts as keeping up
  *wblocks = L.wblocks(c->nslots);
  if (c->tun.plan_debug)
    fprintf(stderr, "[k_plan] workers: %u waves (%u per workgroup), g-scores %u, heap %u entries, DAG exit %u, %u B LDS each\n",
            W.nworkers, W.wpb, wcfg.gs_lds, wcfg.hcap, wcfg.dag, W.lds_per_wave);
  if (W.nworkers == 0 || wcfg.hcap < 4u) P.coop = 0;  // nothing fits beside the planner: exit mode
  return TSW_OK;
}

// host A* service: coop mode only (exit mode has no waits to shorten)
static bool host_serves(const tsw_ctx* c, const PlanArgs& P) {
  return P.coop && c->host_threads && c->h_hreq && c->h_hrep;
}

static int host_service_args(tsw_ctx* c, PlanArgs* P) {
  const bool serve = host_serves(c, *P);
  P->hreq = serve ? c->h_hreq.dev : nullptr;
  P->hrep = serve ? c->h_hrep.dev : nullptr;
  P->hring = serve ? c->hring : 0u;
  P->hask = nullptr;
  P->hearly = serve ? c->tun.host_early : 0u;
  if (P->hearly && P->n) {
    if (c->d_hask.cap < 2 * (size_t)P->n) {
      HIPCHK(hipStreamSynchronize(c->s));
      HIPCHK(c->d_hask.alloc(2 * (size_t)P->n));
    }
    P->hask = c->d_hask;
  }
  return TSW_OK;
}

// Everything of a dispatch that depends on P.coop: the launch geometry, the workers, the service.
static int setup_dispatch(tsw_ctx* c, PlanArgs& P, Dispatch* D) {
  *D = Dispatch{};
  const size_t planner = plan_lds_bytes(P.n, P.ncell, P.m, P.agents_lds, P.occ_lds, P.tasks_lds, P.f_lds, P.mu_lds, P.part_lds);
  // coop mode: the planner block reserves its CU's whole LDS so no worker wave is placed beside it
  // (they would compete for its SIMDs and LDS bandwidth on the critical path)
  D->lds = P.coop ? std::max<size_t>(planner, (size_t)std::max(c->max_lds - PLAN_LDS_RESERVE, 0)) : planner;
  // one lane per agent in the parallel passes when possible; >= 4 waves for the task argmin
  D->block = std::min<uint32_t>(PLAN_BLOCK_MAX, std::max<uint32_t>(256, (P.n + 63) / 64 * 64));
  if (c->tun.plan_block) D->block = std::max<uint32_t>(64u, c->tun.plan_block);
  if (P.coop) TRY(worker_args(c, P, D->lds, D->block, &D->W, &D->wblocks));
  TRY(host_service_args(c, &P));
  D->serve = host_serves(c, P);
  if (c->tun.plan_debug)
    fprintf(stderr, "[k_plan] planner LDS: agents %u part 0x%x flinks %u occ %u mu %u tasks %u (%zu B)\n", P.agents_lds,
            P.part_lds, P.f_lds, P.occ_lds, P.mu_lds, P.tasks_lds, planner);
  return TSW_OK;
}

static int upload_ctl(tsw_ctx* c, const PlanCtl& ctl) {
  *c->h_ctl = ctl;
  HIPCHK(hipMemcpyAsync(c->d_ctl, c->h_ctl, sizeof(PlanCtl), hipMemcpyHostToDevice, c->s));
  return TSW_OK;
}

// What the planner, the workers and the host share is zeroed before every launch.
static int reset_dispatch(tsw_ctx* c, const PlanArgs& P, bool serve) {
  if (P.coop) {
    HIPCHK(hipMemsetAsync(c->d_cc, 0, sizeof(CoopCtl), c->s));
    // tickets restart at 0 with every launch: no request word of an earlier one may match
    if (P.hask) HIPCHK(hipMemsetAsync(c->d_hask, 0, (size_t)P.n * 2u * sizeof(unsigned long long), c->s));
    const uint32_t nt = P.mode == MODE_MAPD ? c->qt_count : 0u;
    if (nt) HIPCHK(hipMemcpyAsync(&c->d_cc->head_t, &c->qt_count, 4, hipMemcpyHostToDevice, c->s));
  }
  volatile uint32_t* hf = c->h_flags;
  for (int w = 0; w < HF_WORDS; ++w) hf[w] = 0u;
  if (serve) {
    memset(c->h_hreq, 0, (size_t)c->hring * sizeof(unsigned long long));
    memset(c->h_hrep, 0, (size_t)c->hring * sizeof(uint32_t));
  }
  return TSW_OK;
}

// The helper pool serves for the lifetime of this object: every exit from the wait parks the helpers again.
struct HostServiceScope {
  tsw_ctx* c;
  HostServiceScope(tsw_ctx* c_, bool serve) : c(serve ? c_ : nullptr) {
    if (c) host_service_begin(c);
  }
  ~HostServiceScope() {
    if (c) host_service_end(c);
  }
  HostServiceScope(const HostServiceScope&) = delete;
  HostServiceScope& operator=(const HostServiceScope&) = delete;
};

// The watchdog (PlanWatchdog, tsw_plan.h) said so: raise the abort word. In coop mode the planner's waits
// give up (it exits to the host), the workers leave and the rest of the call runs in exit mode; a planner
// stuck anywhere else sees the word in its round loops and exits with ERR_ABORT and its position. A fault
// can then cost time or fail the call, but never hang it.
static void raise_abort(tsw_ctx* c, volatile uint32_t* hf) {
  hf[HF_ABORT] = 1u;
  ++c->coop_aborts;
  ++c->st.watchdog_fires;
  if (c->watchdog_ms >= 1000u)
    fprintf(stderr, "[tswap] watchdog: planner made no step for %u ms; finishing the call in exit mode\n", c->watchdog_ms);
  if (c->tun.plan_debug && hf[HF_BAR_COUNT]) {  // per-wave barrier breadcrumbs (-DTSW_PBAR): line | 0x10000 once passed
    fprintf(stderr, "[tswap] planner waves at barriers:");
    for (int w = 0; w < PLAN_WAVES_MAX; ++w)
      fprintf(stderr, " %u%s", hf[HF_BAR_LINE + w] & 0xFFFFu, (hf[HF_BAR_LINE + w] >> 16) ? "+" : "");
    fprintf(stderr, "\n[tswap] barriers passed per wave:");
    for (int w = 0; w < PLAN_WAVES_MAX; ++w) fprintf(stderr, " %u", hf[HF_BAR_COUNT + w]);
    fprintf(stderr, "\n[tswap] first mismatch: wave 0 at %u, another at %u\n", hf[HF_BAR_MISMATCH] >> 16,
            hf[HF_BAR_MISMATCH] & 0xFFFFu);
  }
}

// Wait for the launched dispatch: poll the stream and the planner's heartbeat every 50 us. With the host A*
// service on, this thread serves the request ring between the checks, which then run on a 50 us time basis
// instead of after a 50 us sleep. The first check comes at once.
static int wait_dispatch(tsw_ctx* c, bool serve) {
  using Clock = PlanWatchdog::Clock;
  volatile uint32_t* hf = c->h_flags;
  auto next_check = Clock::now();
  PlanWatchdog watchdog(c->watchdog_ms, hf[HF_HEARTBEAT], next_check);
  HostServiceScope helpers(c, serve);
  for (;;) {
    if (serve) {
      const bool any = host_serve_one(c, c->host_scratch[0]);
      if (Clock::now() < next_check) {
        if (!any) __builtin_ia32_pause();
        continue;
      }
    }
    const hipError_t q = hipStreamQuery(c->s);
    if (q == hipSuccess) return TSW_OK;
    if (q != hipErrorNotReady) HIPCHK(q);
    const uint32_t hb = hf[HF_HEARTBEAT];
    if (watchdog.check(hb, hf[HF_ABORT], Clock::now())) raise_abort(c, hf);
    if (serve) next_check = Clock::now() + std::chrono::microseconds(50);
    else std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

// Coop mode, after the dispatch has drained: the workers' and the waits' counters into the stats, the
// workers' error word, and the speculative pairs nobody claimed.
static int harvest_coop(tsw_ctx* c, const WorkerArgs& W) {
  HIPCHK(hipMemcpy(c->h_cc, c->d_cc, sizeof(CoopCtl), hipMemcpyDeviceToHost));
  const CoopCtl& cc = *c->h_cc;
  c->st.host_astar_queries += c->host_queries.exchange(0);
  c->st.host_astar_ms += (double)c->host_busy_ns.exchange(0) * 1e-6;
  c->st.host_astar_used += cc.host_used;
  c->st.coop_waits += cc.waits;
  c->st.coop_wait_ms += (double)cc.wait_ticks / (double)c->wall_khz;
  for (int k = 0; k < 8; ++k) {
    c->st.coop_wait_sec_ms[k] += (double)cc.wait_sec[k] / (double)c->wall_khz;
    c->st.coop_waits_sec[k] += cc.waits_sec[k];
  }
  c->st.astar_queries += cc.worker_queries;
  c->st.coop_workers = W.nworkers;
  for (int k = 0; k < 3; ++k) {
    c->st.coop_worker_busy_ms[k] += (double)cc.wbusy[k] / (double)c->wall_khz;
    c->st.coop_worker_queries[k] += cc.wcount[k];
    c->st.coop_worker_pops[k] += cc.wpops[k];
  }
  if (cc.err) RET(TSW_EOVERFLOW, "K3 worker: A* heap overflow");
  // speculative pairs nobody claimed stay PENDING_S: back to UNKNOWN for later calls — only the
  // unclaimed queue entries (every claimed one was resolved, or reset by the worker that dropped
  // it as stale): a whole-store sweep cost C5 ~4 s per call (18 GB of codes)
  if (cc.head_s > cc.claim_s) {
    HIPCHK(launch_reset_queue(c->d_QS, cc.claim_s, std::min<uint32_t>(cc.head_s, (uint32_t)c->d_QS.cap), c->d_nh,
                              c->tstride, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  return TSW_OK;
}

// ---- TSW_PLAN_DEBUG report ---------------------------------------------------------------------
static hipError_t read_ticks(tsw_ctx* c, unsigned long long (&tk)[TK_COUNT]) {
  return hipMemcpy(tk, c->d_ticks, sizeof tk, hipMemcpyDeviceToHost);
}

// where the stopped planner spent its time: the section and sub-phase slots up to the ASSIGN ones
static void plan_debug_stop(tsw_ctx* c) {
  unsigned long long tk[TK_COUNT];
  if (read_ticks(c, tk) != hipSuccess) return;
  std::string line = "[k_plan] watchdog stop, ticks:";
  for (int q = 0; q <= TK_ASG_SECTIONS; ++q) line += " " + std::to_string(q) + ":" + std::to_string(tk[q]);
  fprintf(stderr, "%s\n", line.c_str());
}

static void coop_debug_report(tsw_ctx* c) {
  const CoopCtl& cc = *c->h_cc;
  fprintf(stderr, "[k_plan] needed pairs unresolved (never queued / queued speculatively): PRE1 %u/%u RULES %u/%u "
          "MOVE %u/%u | PRE1 never queued: assigned %u, picked up %u | chain queries %llu of %llu | host asked %u (early %u) "
          "used %u (early, in refresh %u)\n", cc.dbg_need[0], cc.dbg_need[1], cc.dbg_need[2],
          cc.dbg_need[3], cc.dbg_need[4], cc.dbg_need[5], cc.dbg_need[6], cc.dbg_need[7],
          (unsigned long long)cc.chain_queries, (unsigned long long)cc.worker_queries, cc.host_asked, cc.early_asked,
          cc.host_used, cc.early_taken);
  {
    static const char* nm[6] = {"r3b", "r3s", "rot", "mv", "asg", "pick"};
    std::string line = "[k_plan] PRE1 unresolved by agent change (unknown/pending):";
    for (int tg = 0; tg < 64; ++tg) {
      if (!cc.dbg_tag[0][tg] && !cc.dbg_tag[1][tg]) continue;
      std::string name;
      for (int b = 0; b < 6; ++b)
        if (tg & (1 << b)) name += (name.empty() ? "" : "+") + std::string(nm[b]);
      char buf[96];
      snprintf(buf, sizeof buf, " %s %u/%u", name.empty() ? "none" : name.c_str(), cc.dbg_tag[0][tg], cc.dbg_tag[1][tg]);
      line += buf;
    }
    fprintf(stderr, "%s\n", line.c_str());
  }
  fprintf(stderr, "[k_plan] speculative pairs dropped as stale: %u (older than %u timesteps)\n",
          cc.spec_dropped, c->tun.stale_steps);
  fprintf(stderr, "[k_plan] predicted chains: %u jobs | assignments %u: predicted task %u, no prediction %u\n",
          cc.pred_jobs, cc.pred_asg, cc.pred_hit, cc.pred_none);
  fprintf(stderr, "[k_plan] spec backlog at wait start: avg %.1f max %u | queue delay enqueue -> claim: needed "
          "avg %.1f us (%u > 1 ms, %u already resolved), speculative avg %.1f timesteps (%u > 1, %u already resolved)\n",
          cc.waits ? (double)cc.dbg_depth / cc.waits : 0.0, cc.dbg_depth_max,
          cc.wcount[0] ? cc.qdelay[0] / 100.0 / cc.wcount[0] : 0.0, cc.qlate[0], cc.qskip[0],
          cc.wcount[1] ? (double)cc.qdelay[1] / cc.wcount[1] : 0.0, cc.qlate[1], cc.qskip[1]);
  fprintf(stderr, "[k_plan] worker A* ms (queries, pops): needed %.1f (%u, %llu) spec %.1f (%u, %llu) task chains "
          "%.1f (%u, %llu) | tier-2 hand-offs %llu tier-3 %llu | detour staging %.1f ms (%u)\n",
          cc.wbusy[0] / (double)c->wall_khz, cc.wcount[0], cc.wpops[0], cc.wbusy[1] / (double)c->wall_khz,
          cc.wcount[1], cc.wpops[1], cc.wbusy[2] / (double)c->wall_khz, cc.wcount[2], cc.wpops[2],
          cc.wpops[3] & 0xFFFFFFFFull, cc.wpops[3] >> 32, cc.wbusy[3] / (double)c->wall_khz, cc.wcount[3]);
}

// The finished plan's report: k_plan's tick slots (wall-clock ticks as us, shader cycles as kcycles) and,
// in coop mode, the workers' counters of the last dispatch.
static int plan_debug_report(tsw_ctx* c, const PlanCtl& k, uint64_t launches, bool coop) {
  unsigned long long tk[TK_COUNT];
  HIPCHK(read_ticks(c, tk));
  const auto us = [&](TickSlot s) { return tk[s] / 100.0; };
  const auto kcyc = [&](TickSlot s) { return tk[s] / 1e3; };
  fprintf(stderr, "[k_plan] assign us: transitions %.0f compaction %.0f scan %.0f accept %.0f update %.0f | sections %llu batches %llu accepted %llu\n",
          us(TK_ASG_TRANSITIONS), us(TK_ASG_COMPACT), us(TK_ASG_SCAN), us(TK_ASG_ACCEPT), us(TK_ASG_UPDATE),
          tk[TK_ASG_SECTIONS], tk[TK_ASG_BATCHES], tk[TK_ASG_ACCEPTED]);
  // the scan's parts as thread 0 sees them (the closing part includes its wait for the slowest wave)
  fprintf(stderr, "[k_plan] assign scan us: index %.0f bound %.0f entries %.0f reduce %.0f | chunk-agent pairs %llu chunks %llu "
          "scanning waves %llu list rounds %llu | batch widths 1: %llu 2-4: %llu 5-8: %llu 9-16: %llu\n",
          us(TK_SCAN_INDEX), us(TK_SCAN_BOUND), us(TK_SCAN_ENTRIES), us(TK_SCAN_REDUCE), tk[TK_SCAN_PAIRS],
          tk[TK_SCAN_CHUNKS], tk[TK_SCAN_WAVES], tk[TK_SCAN_ROUNDS], tk[TK_SCAN_B_ONE], tk[TK_SCAN_B_LE4],
          tk[TK_SCAN_B_LE8], tk[TK_SCAN_B_MORE]);
  // walk-ahead (round 14): steps whose walk ran in PRE1 / that PRE1 left to the rules phase / whose walk the
  // waves beside wave 0 finished and published there (counted by the publishing wave), those walkers' time
  // from arming to the last wave's count, steps in which wave 0 was done before them
  fprintf(stderr, "[k_plan] PRE1 publish us %.0f (%llu) | rules init us %.0f prefetch us %.0f publish us %.0f (%llu)"
          " | walk-ahead steps in PRE1 %llu left to RULES %llu done in RULES %llu walkers us %.0f wave 0 first %llu\n",
          us(TK_PRE1_PUBLISH), tk[TK_PRE1_PUBLISHES], us(TK_RULES_INIT), us(TK_RULES_PREFETCH), us(TK_RULES_PUBLISH),
          tk[TK_RULES_PUBLISHES], tk[TK_WALK_IN_PRE1], tk[TK_WALK_LEFT], tk[TK_WALK_IN_RULES], us(TK_WALKERS),
          tk[TK_WALK_WAVE0_FIRST]);
  fprintf(stderr, "[k_plan] wave rules kcycles: load %.0f stale %.0f fast %.0f update %.0f slow %.0f rot %.0f | "
          "loads %llu fast firings %llu | rotations %llu, settle kcycles: successors %.0f walk %.0f\n",
          kcyc(TK_WR_LOAD), kcyc(TK_WR_STALE), kcyc(TK_WR_FAST), kcyc(TK_WR_UPDATE), kcyc(TK_WR_SLOW), kcyc(TK_WR_ROT),
          tk[TK_WR_LOADS], tk[TK_WR_FAST_FIRINGS], tk[TK_R4_ROTATIONS], kcyc(TK_SETTLE_SUCC), kcyc(TK_SETTLE_WALK));
  fprintf(stderr, "[k_plan] wave rules batches %llu (longest walks %llu hops) kcycles: marks %.0f walks %.0f apply %.0f\n",
          tk[TK_WB_BATCHES], tk[TK_WB_HOPS], kcyc(TK_WB_MARKS), kcyc(TK_WB_WALKS), kcyc(TK_WB_APPLY));
  fprintf(stderr, "[k_plan] steps %u rule rounds %u move rounds %u launches %llu | move passes us %.0f %.0f %.0f"
          " | rule-3 walk hops %llu rotations %llu | rules scan %.0f fire %.0f relabel %.0f\n", k.steps_run, k.rule_rounds,
          k.move_rounds, (unsigned long long)launches, us(TK_MOVE_PASS1), us(TK_MOVE_PASS2), us(TK_MOVE_PASS3),
          tk[TK_R3_WALK_HOPS], tk[TK_R4_ROTATIONS], us(TK_RULES_SCAN), us(TK_RULES_FIRE), us(TK_RULES_RELABEL));
  if (coop) coop_debug_report(c);
  return TSW_OK;
}

// PlanCtl::err as the call's return code and error string (PLAN_ERR_TABLE, tsw_plan.h); TSW_OK: no error.
static int plan_error(tsw_ctx* c, const PlanCtl& k) {
  const PlanErrRow* row = plan_err_row(k.err);
  if (!row) return TSW_OK;
  if (row->msg) RET(row->code, row->msg);
  char buf[256];
  if (row->bits == ERR_ABORT) {
    if (c->tun.plan_debug) plan_debug_stop(c);
    snprintf(buf, sizeof buf,
             "planner stopped by the watchdog (no timestep for %u ms): t %u section %u cursor %u, %u rule rounds, "
             "%u move rounds", c->watchdog_ms, k.t, k.section, k.i, k.rule_rounds, k.move_rounds);
  } else {
    snprintf(buf, sizeof buf, "plan kernel error bits 0x%x", k.err);
  }
  RET(row->code, buf);
}

// Drive k_plan from `init` until it reports done. Coop mode: one dispatch runs the planner and the K3 workers;
// a planner that gave up waiting has its needed queue resolved here and is relaunched. Exit mode: each
// NEED_QUERIES exit runs K3 on the queued pairs. After a watchdog firing a coop call goes on in exit mode.
// Every return happens after the dispatch has drained (workers included): nothing of this call keeps
// running into the next one. setup: D is built here (a later segment of the same call reuses it).
static int run_plan_impl(tsw_ctx* c, PlanArgs& P, Dispatch& D, bool setup, const PlanCtl& init) {
  TRY(upload_ctl(c, init));
  if (setup) TRY(setup_dispatch(c, P, &D));
  uint64_t bound = 16ull * P.n + 4096ull * (init.max_t + 1);  // launches without reaching the end
  // PlanCtl's relabel counters run on through the relaunches of a call (and the segments of an online plan): the
  // stats take each launch's increase, not its running total
  uint32_t full0 = init.relabel_full, inc0 = init.relabel_inc;
  for (uint64_t launches = 0;;) {
    if (launches > bound) RET(TSW_EINVAL, "plan kernel made no progress");
    const bool coop = P.coop != 0;
    TRY(reset_dispatch(c, P, D.serve));
    {
      Timer t(c, CAT_WALK);
      HIPCHK(launch_plan(P, c->d_pargs, coop ? &D.W : nullptr, D.wblocks, D.lds, D.block, c->s));
      c->st.plan_block = D.block;
    }
    ++launches;
    c->st.walker_launches++;
    if (coop) c->st.astar_launches++;
    HIPCHK(hipMemcpyAsync(c->h_ctl, c->d_ctl, sizeof(PlanCtl), hipMemcpyDeviceToHost, c->s));
    TRY(wait_dispatch(c, D.serve));
    HIPCHK(hipStreamSynchronize(c->s));
    if (coop) TRY(harvest_coop(c, D.W));
    const PlanCtl k = *c->h_ctl;
    TRY(plan_error(c, k));
    c->st.relabels_full += k.relabel_full - full0;
    c->st.relabels_inc += k.relabel_inc - inc0;
    full0 = k.relabel_full, inc0 = k.relabel_inc;
    if (k.status == PLAN_DONE) {
      c->chase_id = k.chase_id;
      c->st.rule_rounds += k.rule_rounds;
      c->st.move_rounds += k.move_rounds;
      if (c->tun.plan_debug) TRY(plan_debug_report(c, k, launches, coop));
      // exit mode: pairs the prefetch queued but no firing needed — resolve them so no table entry
      // is left PENDING for later calls (coop mode: the workers drained the needed queue)
      if (!coop && k.qcount > 0) {
        if (k.qcount > P.qcap) RET(TSW_EINVAL, "plan kernel queue overflow");
        TRY(resolve_queue(c, c->d_Q, k.qcount));
      }
      return TSW_OK;
    }
    c->st.plan_exits[std::min<uint32_t>(k.section, 7u)]++;
    if (!coop) {
      if (k.status != PLAN_NEED_QUERIES || k.qcount == 0 || k.qcount > P.qcap)
        RET(TSW_EINVAL, "plan kernel stopped without resolvable next hops");
      TRY(resolve_queue(c, c->d_Q, k.qcount));
      continue;
    }
    if (k.status != PLAN_NEED_QUERIES) RET(TSW_EINVAL, "plan kernel stopped without resolvable next hops");
    if (c->h_flags[HF_ABORT]) {
      // watchdog fired: finish this call in exit mode (host-side K3 passes at planner exits), from where
      // the planner stopped; pairs the aborted workers left queued are unqueued first
      HIPCHK(launch_reset_pending(c->d_nh, (uint64_t)c->tab_count * c->tstride, c->s));
      HIPCHK(hipStreamSynchronize(c->s));
      P.coop = 0;
      PlanCtl resume = k;
      resume.status = PLAN_RUNNING;
      resume.qcount = 0;
      TRY(upload_ctl(c, resume));
      TRY(setup_dispatch(c, P, &D));
      bound = 16ull * P.n + 4096ull * (resume.max_t + 1);
      launches = 0;
      continue;
    }
    // the planner gave up waiting (no worker left — they exit after an idle spell — or a pair stayed
    // pending): resolve its needed queue on the host side before relaunching, so every relaunch makes
    // progress whatever the workers of the next dispatch do (exact codes; resolved ones rewrite the same)
    if (k.qcount > 0) {
      if (k.qcount > P.qcap) RET(TSW_EINVAL, "plan kernel queue overflow");
      TRY(run_astar(c, c->d_Q, k.qcount, true, nullptr, nullptr));
      TRY(check_err(c));
    }
  }
}

// Any failure after k_plan queued pairs leaves their codes PENDING: reset them.
static int run_plan(tsw_ctx* c, PlanArgs& P, const PlanCtl& init) {
  Dispatch D;
  return reset_pending_after(c, run_plan_impl(c, P, D, true, init));
}

// The K4 spatial index (TaskIndex, tsw_ctx.h) of the tasks' pickup points.
static TaskIndex build_task_index(const std::vector<uint32_t>& pxy) {
  constexpr uint32_t KCHH = 32;
  const uint32_t m = (uint32_t)pxy.size(), nch = std::max<uint32_t>((m + KCHH - 1u) / KCHH, 1u);
  TaskIndex ix{std::vector<uint32_t>((size_t)nch * KCHH, TASK_TAKEN), std::vector<uint32_t>((size_t)nch * KCHH, 0xFFFFFFFFu),
               std::vector<uint32_t>(std::max<uint32_t>(m, 1u)), std::vector<uint32_t>(nch, 0u),
               std::vector<uint2>(nch, make_uint2(0u, 0u))};
  std::vector<std::pair<uint32_t, uint32_t>> ord(m);
  for (uint32_t k = 0; k < m; ++k) ord[k] = {morton2(pxy[k] & 0xFFFFu, pxy[k] >> 16), k};
  std::sort(ord.begin(), ord.end());
  for (uint32_t pos = 0; pos < m; ++pos) {
    const uint32_t k = ord[pos].second, xy = pxy[k], ch = pos / KCHH;
    ix.live[pos] = xy;
    ix.klt[pos] = k;
    ix.kpos[k] = pos;
    const uint32_t x = xy & 0xFFFFu, y = xy >> 16;
    uint2& bx = ix.kbox[ch];
    if (ix.kcnt[ch] == 0u) {
      bx = make_uint2(xy, xy);
    } else {
      bx.x = std::min(bx.x & 0xFFFFu, x) | (std::min(bx.x >> 16, y) << 16);
      bx.y = std::max(bx.y & 0xFFFFu, x) | (std::max(bx.y >> 16, y) << 16);
    }
    ++ix.kcnt[ch];
  }
  return ix;
}

// The plan's records, written by k_plan timestep-major (t * n + i), into the caller's agent-major arrays.
static int download_records(tsw_ctx* c, uint32_t n, uint32_t t, size_t stride_t, tsw_rec* out, uint32_t* goal_out) {
  std::vector<uint64_t> rec((size_t)t * n);
  HIPCHK(hipMemcpyAsync(rec.data(), c->d_rec, rec.size() * 8, hipMemcpyDeviceToHost, c->s));
  std::vector<uint32_t> grec;
  if (goal_out) {
    grec.resize((size_t)t * n);
    HIPCHK(hipMemcpyAsync(grec.data(), c->d_grec, grec.size() * 4, hipMemcpyDeviceToHost, c->s));
  }
  HIPCHK(hipStreamSynchronize(c->s));
  for (uint32_t tt = 0; tt < t; ++tt)
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t r = rec[(size_t)tt * n + i];
      tsw_rec& o = out[(size_t)i * stride_t + tt];
      o.x = (uint16_t)(r & 0xFFFF);
      o.y = (uint16_t)((r >> 16) & 0xFFFF);
      o.state = (uint8_t)((r >> 32) & 0xFF);
      o.pad[0] = o.pad[1] = o.pad[2] = 0;
      if (goal_out) goal_out[(size_t)i * stride_t + tt] = grec[(size_t)tt * n + i];
    }
  return TSW_OK;
}

// The plan's inputs on the device: agent and task state and the K4 index, their buffers grown first.
static int upload_plan_inputs(tsw_ctx* c, uint32_t n, uint32_t m, const std::vector<uint32_t>& vcell,
                              const std::vector<uint32_t>& pick, const std::vector<uint32_t>& dlv, const TaskIndex& ix) {
  const uint32_t nch = (uint32_t)ix.kcnt.size();
  TRY(ensure_agents(c, std::max<uint32_t>(n, 1)));
  if (!(c->d_live.holds(ix.live.size()) && c->d_pick.holds(ix.live.size()) && c->d_dlv.holds(ix.live.size()))) {
    HIPCHK(hipStreamSynchronize(c->s));
    HIPCHK(c->d_live.grow(ix.live.size()));
    HIPCHK(c->d_pick.grow(ix.live.size()));
    HIPCHK(c->d_dlv.grow(ix.live.size()));
    if (!c->d_unused) HIPCHK(c->d_unused.alloc(1));
  }
  if (!(c->d_klt.holds(ix.live.size()) && c->d_kpos.holds(ix.live.size()))) {
    HIPCHK(hipStreamSynchronize(c->s));
    HIPCHK(c->d_klt.grow(ix.live.size()));
    HIPCHK(c->d_kpos.grow(ix.live.size()));
  }
  if (!(c->d_kbox.holds(nch) && c->d_kcnt.holds(nch))) {
    HIPCHK(hipStreamSynchronize(c->s));
    HIPCHK(c->d_kbox.grow(nch));
    HIPCHK(c->d_kcnt.grow(nch));
  }
  c->kchunks = nch;
  if (n) {
    HIPCHK(hipMemcpyAsync(c->d_v, vcell.data(), n * 4ull, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_g, vcell.data(), n * 4ull, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemsetAsync(c->d_st, 0, n, c->s));
    HIPCHK(hipMemsetAsync(c->d_task, 0xFF, n * 4ull, c->s));
  }
  HIPCHK(hipMemcpyAsync(c->d_live, ix.live.data(), ix.live.size() * 4ull, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_klt, ix.klt.data(), ix.klt.size() * 4ull, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_kpos, ix.kpos.data(), ix.kpos.size() * 4ull, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_kbox, ix.kbox.data(), ix.kbox.size() * sizeof(uint2), hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_kcnt, ix.kcnt.data(), ix.kcnt.size() * 4ull, hipMemcpyHostToDevice, c->s));
  if (m) {
    HIPCHK(hipMemcpyAsync(c->d_pick, pick.data(), m * 4ull, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_dlv, dlv.data(), m * 4ull, hipMemcpyHostToDevice, c->s));
  }
  HIPCHK(hipMemcpyAsync(c->d_unused, &m, 4, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipStreamSynchronize(c->s));  // the host vectors may go once this returns
  return TSW_OK;
}

// Coop mode: every task's pickup -> delivery path, resolved hop by hop by the workers in the background
// (lowest priority): an agent that picks the task up finds its next hops already there. Also grows the hot
// and the predicted chains' queues. The chains are queued in task index order, or in `order` (m task
// indices); chain_at, when given, gets m + 1 entries: the chains among the first j tasks of that order.
static int queue_task_chains(tsw_ctx* c, uint32_t n, uint32_t m, const std::vector<uint32_t>& pick,
                             const std::vector<uint32_t>& dlv, const uint32_t* order, std::vector<uint32_t>* chain_at) {
  std::vector<AstarQuery> qt;
  qt.reserve(m);
  if (chain_at) chain_at->assign((size_t)m + 1u, 0u);
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t k = order ? order[j] : j;
    if (pick[k] != dlv[k] && pick[k] != CELL_BAD && dlv[k] != CELL_BAD) qt.push_back(AstarQuery{pick[k], dlv[k], c->h_goal_tab[dlv[k]], 0u});
    if (chain_at) (*chain_at)[j + 1u] = (uint32_t)qt.size();
  }
  if (qt.size() > c->d_QT.cap) {
    HIPCHK(hipStreamSynchronize(c->s));
    HIPCHK(c->d_QT.grow(qt.size()));
  }
  if (!qt.empty()) {
    HIPCHK(hipMemcpyAsync(c->d_QT, qt.data(), qt.size() * sizeof(AstarQuery), hipMemcpyHostToDevice, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  c->qt_count = (uint32_t)qt.size();
  if (c->tun.hot_chains) TRY(grow_synced(c, c->d_QH, m));
  // predictions: one per pickup (<= m) plus, with bit 1, one per goal change of a delivering agent;
  // a full queue only stops predicting
  const size_t qp = (size_t)m + 16u * (size_t)n * (c->tun.predict & 2u ? 8u : 0u);
  if (c->tun.hot_chains && c->tun.predict) TRY(grow_synced(c, c->d_QP, qp));
  return TSW_OK;
}

// ---- a MAPD plan call in parts (tsw_ctx.h): validate and index -> upload -> tables -> dispatch -> records ----
void plan_phase(tsw_ctx* c, const PlanCall& call, const char* what) {
  if (c->tun.plan_debug)
    fprintf(stderr, "[plan] %s at %.1f ms\n", what,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call.t0).count());
}

int plan_validate_index(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m, uint32_t max_t,
                        tsw_rec* out, uint32_t* goal_out, uint32_t* out_T, PlanCall* call) {
  call->t0 = std::chrono::steady_clock::now();
  if (!out_T || (n && (!starts || !out)) || (m && !tasks)) RET(TSW_EINVAL, "null argument");
  if (max_t > (1u << 20)) RET(TSW_EINVAL, "max_t too large");
  TRY(set_device(c));
  call->n = n, call->m = m, call->max_t = max_t;
  call->want_goals = goal_out != nullptr;
  std::vector<uint32_t>&vcell = call->vcell, &pick = call->pick, &dlv = call->dlv, &pxy = call->pxy, &goalset = call->goalset;
  vcell.assign(n, 0u), pick.assign(m, 0u), dlv.assign(m, 0u), pxy.assign(m, 0u);
  goalset.clear();
  goalset.reserve(n + 2 * (size_t)m);
  for (uint32_t i = 0; i < n; ++i) {
    if (!cell_ok(c, starts[i].x, starts[i].y, &vcell[i]))
      RET(TSW_EINVAL, "start position off-grid or blocked (reference panics at tswap.rs:94)");
    goalset.push_back(vcell[i]);
  }
  // Task cells are looked up only when the planner needs them — the pickup when the task is
  // assigned (pos2id[&task.pickup], tswap.rs:136), the delivery when its agent reaches the pickup
  // (:112) — so an off-grid or blocked one fails the call only then (k_plan ERR_BAD_*), exactly
  // where the reference panics. The assignment's Manhattan distance still uses the raw point
  // (:125-130); coordinates are clamped to 0xFFFE (0xFFFFFFFF marks a taken task), which cannot
  // change which task wins: any point past 0xFFFE is farther than every on-grid pickup (sides <=
  // 2048), and assigning it fails anyway.
  for (uint32_t k = 0; k < m; ++k) {
    if (!cell_ok(c, tasks[k].pickup.x, tasks[k].pickup.y, &pick[k])) pick[k] = CELL_BAD;
    if (!cell_ok(c, tasks[k].delivery.x, tasks[k].delivery.y, &dlv[k])) dlv[k] = CELL_BAD;
    pxy[k] = task_pxy(tasks[k]);
    if (pick[k] != CELL_BAD) goalset.push_back(pick[k]);
    if (dlv[k] != CELL_BAD) goalset.push_back(dlv[k]);
  }
  call->ix = build_task_index(pxy);
  return TSW_OK;
}

int plan_upload(tsw_ctx* c, PlanCall& call) {
  TRY(upload_plan_inputs(c, call.n, call.m, call.vcell, call.pick, call.dlv, call.ix));
  const size_t recs = ((size_t)call.max_t + 1) * std::max<uint32_t>(call.n, 1);
  TRY(grow_synced(c, c->d_rec, recs));
  if (call.want_goals) TRY(grow_synced(c, c->d_grec, recs));
  plan_phase(c, call, "inputs uploaded");
  return TSW_OK;
}

int plan_tables(tsw_ctx* c, PlanCall& call, const uint32_t* chain_order, std::vector<uint32_t>* chain_at) {
  const uint32_t n = call.n, m = call.m;
  TRY(build_occ(c, n));
  TRY(ensure_tables(c, call.goalset, true));
  HIPCHK(hipStreamSynchronize(c->s));
  plan_phase(c, call, "tables built");
  TRY(ensure_queue(c, 4 * (size_t)n + 4096));  // needed pairs (<= 2n per exit) + speculative prefetch (qcap/2)
  c->qt_count = 0;
  if (chain_at) chain_at->clear();
  if (c->tun.coop && !c->resolver && !eager_policy(c, 0)) {
    TRY(ensure_coop(c, n, call.max_t));
    if (c->tun.task_chains && m) TRY(queue_task_chains(c, n, m, call.pick, call.dlv, chain_order, chain_at));
  }
  call.P = plan_args(c, n, m, MODE_MAPD, call.want_goals);
  call.dispatched = false;
  return TSW_OK;
}

int plan_segment(tsw_ctx* c, PlanCall& call, const PlanCtl& init) {
  const bool setup = !call.dispatched;
  call.dispatched = true;
  return reset_pending_after(c, run_plan_impl(c, call.P, call.D, setup, init));
}

int plan_download(tsw_ctx* c, PlanCall& call, uint32_t t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T) {
  c->st.steps += t;
  *out_T = t;
  if (call.n) TRY(download_records(c, call.n, t, (size_t)call.max_t + 1, out, goal_out));
  resolve_timing(c);
  c->st.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call.t0).count();
  return TSW_OK;
}

static int plan_impl(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m,
              uint32_t max_t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T) {
  PlanCall call;
  TRY(plan_validate_index(c, starts, n, tasks, m, max_t, out, goal_out, out_T, &call));
  TRY(plan_upload(c, call));
  TRY(plan_tables(c, call));
  PlanCtl init{};
  init.section = SEC_ASSIGN;
  init.unused = m;
  init.max_t = max_t;
  init.chase_id = c->chase_id;
  init.move_rounds = c->tun.move_round0;
  plan_phase(c, call, "plan dispatch starts");
  TRY(plan_segment(c, call, init));
  plan_phase(c, call, "plan dispatch done");
  return plan_download(c, call, c->h_ctl->t, out, goal_out, out_T);
}

}  // namespace tsw

extern "C" {

int tsw_plan_mapd(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m,
                  uint32_t max_t, tsw_rec* out, uint32_t* out_T) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  return plan_impl(c, starts, n, tasks, m, max_t, out, nullptr, out_T);
}

int tsw_plan_mapd_trace(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m,
                        uint32_t max_t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  return plan_impl(c, starts, n, tasks, m, max_t, out, goal_out, out_T);
}

int tsw_plan_mapd_resolved(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m,
                           uint32_t max_t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T, tsw_resolve_fn resolve,
                           void* user) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (!resolve) RET(TSW_EINVAL, "null resolver");
  c->resolver = resolve;
  c->resolver_user = user;
  const int rc = plan_impl(c, starts, n, tasks, m, max_t, out, goal_out, out_T);
  c->resolver = nullptr;
  c->resolver_user = nullptr;
  return rc;
}

int tsw_step(tsw_ctx* c, uint32_t* v, uint32_t* g, uint32_t n) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (n == 0) return TSW_OK;
  if (!v || !g) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  std::vector<uint32_t> goals;
  goals.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (!cell_id_ok(c, v[i]) || !cell_id_ok(c, g[i])) RET(TSW_EINVAL, "agent cell off-grid or blocked");
    goals.push_back(g[i]);
  }
  TRY(ensure_agents(c, n));
  HIPCHK(hipMemcpyAsync(c->d_v, v, n * 4ull, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_g, g, n * 4ull, hipMemcpyHostToDevice, c->s));
  TRY(build_occ(c, n));
  TRY(ensure_tables(c, goals, true));
  TRY(ensure_queue(c, 4 * (size_t)n + 4096));  // needed pairs (<= 2n per exit) + speculative prefetch (qcap/2)
  if (c->tun.coop && !eager_policy(c, 0)) TRY(ensure_coop(c, n));
  PlanArgs P = plan_args(c, n, 0, MODE_STEP, false);
  PlanCtl init{};
  init.section = SEC_PRE1;
  init.chase_id = c->chase_id;
  init.move_rounds = c->tun.move_round0;
  TRY(run_plan(c, P, init));
  HIPCHK(hipMemcpyAsync(v, c->d_v, n * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(g, c->d_g, n * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  c->st.steps++;
  resolve_timing(c);
  return TSW_OK;
}

}  // extern "C"
