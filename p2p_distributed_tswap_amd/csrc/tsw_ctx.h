// tsw_ctx.h — the host runtime's context (struct tsw_ctx behind include/tswap.h) and what its
// translation units share: tsw_ctx.hip (create / destroy, tunables, stats), tsw_tables.hip (K1 and the
// goal-table store), tsw_query.hip (K3 scratch, queue and passes), tsw_plan_host.hip (the plan runner and
// its host A* service), tsw_online_host.hip (the plan with release times, run in segments),
// tsw_fleet_host.hip (decide and the fleet entry points), tsw_audit_host.hip (the
// audit of plan records), tsw_timeline_host.hip (the task timeline) and tsw_st_astar_host.hip (the space-time
// A* with reservations). Host code only; every
// device buffer of the context is a DevBuf / PinnedBuf member (tsw_buf.h) and is freed with it.
// Nothing here depends on the build flavour: only tsw_ctx.hip is compiled per flavour.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "tsw_buf.h"
#include "tsw_host_astar.h"
#include "tsw_internal.h"
#include "tsw_launch.h"
#include "tsw_plan.h"
#include "tswap.h"

using namespace tsw;  // as the sources that include this header have always had it

namespace tsw {

struct DevStatus {
  uint32_t err;
  uint32_t done;
  uint32_t qcount;
  uint32_t novf;  // LDS A*: queries handed to the global-heap kernel
  uint32_t novf2;  // second tier (LDS heap, global g_scores): queries handed on to k_astar
  uint32_t work;  // k_bfs_wave goal dequeue counter
  uint32_t qnext;  // k_astar_lds / k_astar_wave dynamic query dequeue counter
  uint32_t qnext2;  // k_astar_wave second tier
};

enum { CAT_BFS = 0, CAT_ASTAR = 1, CAT_WALK = 2, CAT_ASSIGN = 3, NCAT = 4 };

// Diagnostic / A-B knobs. The production library (libtswap_hip.so) never reads the environment:
// these are its fixed defaults, and the only caller-visible options are tsw_opts (include/tswap.h).
// The diagnostic build (libtswap_hip_diag.so, -DTSW_DIAG, __graft_entry__.build) reads the TSW_*
// variables below ONCE when a context is created — kernel A/B variants, instrumentation, and
// TSW_BFS_DBG, which drops work and writes WRONG tables (measurement only).
struct Tunables {
  uint32_t bfs_mode = 0;          // TSW_BFS_KERNEL: 0 auto, 1 wave (row words), 2 block, 3 blk (8x8), 4 big, 5 mg
  uint32_t bfs_cap = 512;         // TSW_BFS_LISTCAP: k_bfs_wave LDS list entries
  uint32_t blk_cap = 576;         // TSW_BFS_BLKCAP: k_bfs_blk LDS list entries
  uint32_t bfs_waves = 16;        // TSW_BFS_WAVES: waves per K1 workgroup cap
  bool bfs_order = true;          // TSW_BFS_ORDER=0: keep the caller's goal order (no LPT)
  bool bfs_prof = false;          // TSW_BFS_PROF: print K1 cycle split per launch
  bool bfs_nostage = false;       // TSW_BFS_NOSTAGE: k_bfs_blk writes rows lane-strided (no LDS staging)
  uint32_t bfs_dbg = 0;           // TSW_BFS_DBG: k_bfs_blk diagnostics (BlkBfsArgs::dbg)
  uint32_t bfs_wls = 0;           // TSW_BFS_WLS: k_bfs_blk west-step blocks in LDS
  uint32_t bfs_pair = 0;          // TSW_BFS_PAIR: k_bfs_blk two goals per wave (one per 32-lane half)
  uint32_t wave_hcap = 0;         // TSW_ASTAR_WAVE_HCAP: k_astar_wave LDS heap entries (0 = default)
  int astar_global_gs = -1;       // TSW_ASTAR_GLOBAL_GS: -1 auto, 0 LDS g-scores, 1 global slots
  bool astar_tier2 = true;        // TSW_ASTAR_NO_TIER2: skip the LDS-heap/global-g second tier
  uint32_t astar_diag = 0;        // TSW_ASTAR_SERIAL / TSW_ASTAR_PROF (ASTAR_DIAG_*)
  bool prefetch = true;           // TSW_NO_PREFETCH: no speculative next-hop prefetch
  uint32_t wave_rules_max = 0xFFFFFFFFu;  // TSW_WAVE_RULES_MAX: wave-0 rules rounds when n <= this
  uint32_t walk_cap = 16;  // TSW_WALK_CAP: successor-walk hops of a batched rules firing (longer ones fire alone)
  uint32_t wide_prefetch = 8;     // TSW_WIDE_PREFETCH: resolved hops walked ahead (0 = candidates only)
  uint32_t wide_hi = 32, wide_lo = 8;  // TSW_WIDE_HI / TSW_WIDE_LO: coop step-start walk-ahead hops (grids <= 2^18 cells with a small backlog / grids > 2^18 cells); round 5, busy instances: 16 -> 32 and 4 -> 8 (profiles/r5/retune_busy_ab.txt)
  bool hot_chains = true;         // TSW_HOT_CHAINS=0: no planner-fed chains of just-assigned tasks (A/B)
  uint32_t chain_hops = 0;        // TSW_CHAIN_HOPS: hops resolved per task chain (0: the whole path)
  uint32_t move_round0 = 0;       // TSW_MOVE_ROUND0 (test knob): movement-round counter at the plan start (forces the MU32 tag wrap)
  bool walk_cache = true;         // TSW_WALK_CACHE=0: the step-start walk-ahead re-reads every code from the agent's next cell
  uint32_t walk_step = 4;         // TSW_WALK_STEP: new hops a step-start walk reads past its cached frontier per timestep (0: no budget, the whole depth at once; round 10, profiles/r10/walk_step_sweep.txt)
  uint32_t predict = 1;           // TSW_PREDICT: predicted task chains, bit 0 at pickups, bit 1 at delivery-goal changes (0: off)
  uint32_t urgent_hops = 1;       // TSW_URGENT_HOPS: walk-ahead pairs this close are queued as needed (0: off)
  uint32_t dag_width = 4;         // TSW_DAG_WIDTH: cells per DAG prefetch level (<= 16)
  uint32_t dag_prefetch = 3;      // TSW_DAG_PREFETCH: DAG levels queued past the walk-ahead's first unresolved cell (round 2, frozen C3: 2 -> 6 levels, 465 -> 450 ms; round 5, busy instances with 32 / 8-hop walks: 3 best, profiles/r5/retune_busy_ab.txt)
  uint32_t prefetch_ext = 7;      // TSW_PREFETCH_EXT: bit 0 DAG from an agent's own unresolved cell, bit 1 walk past the pickup, bit 2 walk-ahead for agents a firing changed (C3 476 -> 409 ms with bits 0-1)
  bool flinks_lds = true;         // TSW_NO_FLINKS_LDS: pointer-doubling buffers stay global
  uint32_t part_lds = 0x7F;       // TSW_PART_LDS: PART_* agent arrays allowed in LDS one by one (tsw_plan.h)
  bool agents_lds = true;         // TSW_AGENTS_LDS=0 (test knob): the agent arrays never go to LDS as a whole set, however small n (the !AG k_plan instantiations at small n)
  bool occ_split = true;          // TSW_OCC_SPLIT=0: the occupancy grid goes to LDS only together with MU
  uint32_t plan_block = 0;        // TSW_PLAN_BLOCK: k_plan workgroup size (0 = auto)
  bool plan_debug = false;        // TSW_PLAN_DEBUG: k_plan sub-phase ticks printed per plan
  bool coop = true;               // TSW_COOP=0: K3 as host-launched passes at planner exits (round-1 mode)
  bool task_chains = true;        // TSW_TASK_CHAINS=0: no task-chain jobs for the coop workers
  bool avoid_xcc = true;          // TSW_WORKER_AVOID_XCD=0: coop workers also run on the planner's XCD
  bool chain_preempt = true;      // TSW_CHAIN_PREEMPT=0: chain workers finish a chain before serving queued pairs
  int worker_gs = -1;             // TSW_WORKER_GS: coop workers' g-score placement (0 global, 1 LDS u32, 2 LDS bytes)
  int worker_fb = -1;             // TSW_WORKER_FB=0 / 1: global-g-score workers without / with the staged free bitmap (-1: by waves per CU)
  bool dag_exit = true;           // TSW_DAG_EXIT=0: coop workers' A* runs to the goal's pop (no DAG early exit)
  uint32_t dag_mask = 0;          // TSW_DAG_MASK: the DAG early-exit test runs every (mask + 1) pops (0: auto)
  uint32_t ab_flags = 0;          // TSW_AB_FLAGS (A/B): 1 no 2-cycle fast path, 2 no end-of-rules prefetch, 4 one agent per K4 batch, 8 no batched rules walks, 16 K4 batches of at most 8, 32 K4 scan list of 4 entries, 64 the step-start walk-ahead stays in PRE1 (not on the idle waves of the rules rounds)
  uint32_t t0_delay_us = 0;       // TSW_T0_DELAY_US (A/B): the planner idles this long after step 0's assignment
  uint32_t stale_steps = 16;      // TSW_SPEC_STALE: coop workers drop speculative pairs older than this many steps (0: never)
  uint32_t reg_heap = 63;         // TSW_ASTAR_REGHEAP: worker A* heaps up to this many entries in registers (0: LDS only)
  // idle-worker polling (tsw_worker.h worker_claim; profiles/r4/poll_ab.txt: C3 371-383 -> 355 ms)
  int chain_mask = -1;            // TSW_CHAIN_MASK: workers with (wid & mask) == mask walk task chains (-1: all)
  uint32_t wake_gate = 2;         // TSW_WAKE_GATE: log2 of the fast-poller subsets a publish rotates over (0: all)
  uint32_t slow_poll = 4;         // TSW_SLOW_POLL: log2 of 1 / (fraction of idle workers polling at full rate) (0: all)
  uint32_t slow_mult = 256;       // TSW_SLOW_MULT: the others' poll interval multiplier
  uint64_t worker_idle_us = 5000000;  // TSW_WORKER_IDLE_US: an idle coop worker exits after this long (test knob)
  int host_astar = -1;            // TSW_HOST_ASTAR: host A* service threads (0: off; -1: tsw_opts.host_astar)
  uint32_t host_delay_us = 0;     // TSW_HOST_ASTAR_DELAY_US (test knob): the host holds every reply back this long
  uint32_t host_ring = 0;         // TSW_HOST_ASTAR_RING (test knob): request / reply ring entries (0: HOST_RING_ENTRIES)
  uint32_t host_early = 1;        // TSW_HOST_ASTAR_EARLY: urgent pairs asked of the host when queued (0: off; 2: and coop_wait leaves the host alone)

  // space-time A* (tsw_st_astar_host.hip), test knobs: they force the paths a small case never takes
  uint32_t st_heap = 0;           // TSW_ST_HEAP: LDS heap entries per wave (0: st_astar_config's; a small one spills to the global heap early)
  uint32_t st_waves = 0;          // TSW_ST_WAVES: waves of a launch at most (0: what the device seats; a small one gives a wave several queries)
  uint32_t st_seg_words = 0;      // TSW_ST_SEG_WORDS: path-segment words of one batch at most (0: by the free memory; a small one cuts a call into batches)
  uint32_t st_tag0 = 1;           // TSW_ST_TAG0: the context's first visited-table tag (near 2^18 - 1: the tags wrap and the tables are wiped)

  static Tunables from_env();  // tsw_ctx.hip: the only reader of the environment
};

}  // namespace tsw

struct tsw_ctx {
  int device = 0;
  hipStream_t s = nullptr;
  std::string err;
  uint32_t flags = 0;
  Tunables tun;
  DevGrid G{};
  std::vector<uint8_t> h_nbmask;
  DevBuf<uint8_t> d_nbmask;
  DevBuf<uint32_t> d_freebits;
  int max_lds = 65536, num_cu = 256;
  // K1 v2 (k_bfs_wave) padded grid + per-wave scratch
  uint32_t Wp = 0, npw = 0;
  DevBuf<uint32_t> d_frp;
  // K1 v3 (k_bfs_blk) 8x8-block grid
  uint32_t BW = 0, BH = 0, Bp = 0, nbp = 0;
  DevBuf<uint64_t> d_frb;
  DevBuf<uint32_t> d_abase;  // k_bfs_blk run-start numbering
  uint32_t nrs = 0;
  uint32_t nfree = 0;                   // free cells (k_bfs_mg: u16 levels need <= 65535)
  // K1 v5 (k_bfs_mg): goal groups of the current launch order (bfs_order), per-workgroup scratch
  std::vector<uint32_t> h_mg_grp;
  DevBuf<uint32_t> d_mg_grp;
  DevBuf<uint32_t> d_mg_wl;
  DevBuf<uint16_t> d_mg_anch;
  uint32_t mg_wgs = 0;  // workgroups d_mg_wl / d_mg_anch hold scratch for
  DevBuf<unsigned long long> d_wlg;  // k_bfs_blk per-wave WL scratch
  uint64_t wlg_waves = 0;            // ... waves it holds
  DevBuf<uint16_t> d_anch;
  DevBuf<uint16_t> d_lovf;
  uint64_t wave_scratch = 0;  // waves d_anch / d_lovf hold, of scratch_words / scratch_lwords each
  size_t scratch_words = 0, scratch_lwords = 0;
  DevBuf<unsigned long long> d_bprof;  // TSW_BFS_PROF=1: k_bfs_wave cycle split, printed per launch

  // goal-table store: slots 0 .. tab_count-1 have been handed out at least once; a slot is live
  // iff h_tab_goal[slot] != NO_GOAL. Slots of evicted tables sit on tab_free for reuse.
  uint64_t tstride = 0;
  uint32_t tab_cap = 0, tab_count = 0, tab_live = 0;  // tab_cap: slots d_dt / d_nh hold
  DevBuf<uint8_t> d_dt;       // detour bytes per (slot, cell) (tsw_internal.h), 1 B / cell / goal
  DevBuf<uint8_t> d_nh;       // next-hop codes per (slot, cell), 1 B / cell / goal
  DevBuf<uint16_t> d_ktmp;    // K1 output of one build batch (u16 tables, tstride each), classified into the store
  DevBuf<int32_t> d_goal_tab;
  std::vector<int32_t> h_goal_tab;
  std::vector<uint32_t> h_tab_goal;
  std::vector<uint64_t> h_tab_stamp;  // call counter of the slot's last use (LRU eviction)
  // 1: the slot's goal is farther than u16 distances reach from some cell (K1 overflow): it is kept
  // WITHOUT a distance table (all TSW_DIST_INF) and every next hop toward it comes from the exact
  // A* (K3, 20-bit g) — get_path's usize g-scores (tswap.rs:288-390) have no such limit
  std::vector<uint8_t> h_tab_tableless;
  DevBuf<uint8_t> d_govf;  // K1 per-goal overflow flags
  std::vector<uint32_t> tab_free;
  uint64_t call_stamp = 0;
  uint64_t table_budget = 0;
  uint64_t evictions = 0;

  // A* scratch
  uint32_t nslots = 0, hcap = 0;  // nslots: slots d_heaps / d_gs / d_epochs hold
  DevBuf<uint64_t> d_heaps;
  DevBuf<uint32_t> d_gs;
  DevBuf<uint32_t> d_epochs;
  uint32_t nslots16 = 0;  // LDS-heap A* (small grids)
  DevBuf<uint16_t> d_gs16;
  DevBuf<uint32_t> d_ep16;
  DevBuf<AstarQuery> d_ovf;
  DevBuf<AstarQuery> d_ovf2;  // second-tier overflow list (same capacity as d_ovf)
  std::vector<uint32_t> h_lpt_goals, h_lpt_slots;  // K1 launch-order staging (bfs_lpt_order)

  // query queue
  DevBuf<AstarQuery> d_Q;
  DevBuf<uint8_t> d_res;
  DevBuf<int32_t> d_lens;

  // coop mode: K3 workers in the plan dispatch beside the planner (control block, queues)
  DevBuf<CoopCtl> d_cc;
  PinnedBuf<CoopCtl> h_cc;
  DevBuf<AstarQuery> d_QS;
  DevBuf<AstarQuery> d_QT;    // task chains of the current plan (host-filled)
  DevBuf<AstarQuery> d_QH;    // hot task chains (planner-filled at assignment), one slot per task
  DevBuf<uint2> d_QP;         // predicted task chains (planner-filled at pickups), PlanArgs::QP
  DevBuf<uint32_t> d_pred;    // TSW_PLAN_DEBUG: per-agent last predicted task
  DevBuf<uint4> d_wf;         // per-agent walk-ahead frontier (PlanArgs::wf)
  uint32_t qt_count = 0;
  // coherent, mapped (.dev: PlanArgs::hflags): HF_WORDS words, named by HostFlag (tsw_plan.h)
  PinnedBuf<uint32_t> h_flags;
  uint64_t coop_aborts = 0;
  uint32_t watchdog_ms = 10000;  // tsw_opts.watchdog_ms
  // host A* service (coop mode): while k_plan runs, the calling thread (and host_threads - 1 parked
  // helpers) answer the planner's needed pairs from the request ring (PlanArgs::hreq) with the host A*
  PinnedBuf<unsigned long long> h_hreq;  // coherent, mapped: hring entries
  PinnedBuf<uint32_t> h_hrep;            // coherent, mapped: hring reply words
  uint32_t hring = 0;
  DevBuf<unsigned long long> d_hask;  // early asks: two remembered request words per agent (PlanArgs::hask)
  uint32_t host_threads = 0;  // 0: service off
  std::vector<HostAstar> host_scratch;  // one per serving thread ([0]: the calling thread)
  std::atomic<uint64_t> host_queries{0}, host_busy_ns{0};
  struct HostPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t epoch = 0;  // one per dispatch
    bool quit = false;
    std::atomic<bool> active{false};
    std::atomic<int> running{0};
  } host_pool;
  // tsw_plan_mapd_resolved: the caller resolves the exit batches (exit mode, lazy next hops)
  tsw_resolve_fn resolver = nullptr;
  void* resolver_user = nullptr;

  DevBuf<DevStatus> d_stat;
  PinnedBuf<DevStatus> h_stat;  // D2H
  DevBuf<PlanCtl> d_ctl;
  PinnedBuf<PlanCtl> h_ctl;
  DevBuf<PlanArgs> d_pargs;  // k_plan reads its arguments from here
  DevBuf<unsigned long long> d_ticks;
  DevBuf<uint32_t> d_dtag;  // TSW_PLAN_DEBUG: per-agent change tags (PlanArgs::dtag)
  int wall_khz = 100000;
  uint32_t chase_id = 0;

  // agents: the arrays of ensure_agents hold acap agents (0 after a failed growth)
  size_t acap = 0;
  DevBuf<uint32_t> d_v, d_g, d_cnt, d_succ, d_ap;
  DevBuf<int32_t> d_gt;
  DevBuf<uint8_t> d_dec;
  DevBuf<uint8_t> d_onc;
  DevBuf<uint8_t> d_candc;
  DevBuf<uint32_t> d_f1;
  DevBuf<uint32_t> d_f2;
  DevBuf<uint64_t> d_mu;
  DevBuf<uint32_t> d_dups;
  PinnedBuf<uint32_t> h_dups;
  DevBuf<uint8_t> d_st;
  DevBuf<int32_t> d_task;
  DevBuf<uint32_t> d_occ;
  DevBuf<uint8_t> d_nhc;
  // tasks
  DevBuf<uint32_t> d_live, d_pick, d_dlv, d_unused;
  // K4 spatial index (PlanArgs::klt / kpos / kbox / kcnt), rebuilt by every plan call
  DevBuf<uint32_t> d_klt, d_kpos, d_kcnt;
  DevBuf<uint2> d_kbox;
  uint32_t kchunks = 0;
  // tsw_plan_mapd_online: the tasks in release order and their clamped pickup points, uploaded once per call
  DevBuf<uint32_t> d_rel_order, d_pxy;
  // records
  DevBuf<uint64_t> d_rec;
  DevBuf<uint32_t> d_grec;
  // temporaries
  DevBuf<uint32_t> d_tmp_a, d_tmp_b, d_tmp_c;
  // tsw_nearby / tsw_decide_fleet scratch (grow-only, laid out by tsw_layout.h): [0] bins, counts and offsets (sized by the fleet
  // and the grid), [1] the lists and k_decide's arrays (sized by the lists' total)
  // [2] tsw_fleet_run's records (v_rec | g_rec) or tsw_fleet_mapd's (out | goal_out | task_out)
  DevBuf<uint32_t> d_fleet[3];
  PinnedBuf<uint32_t> h_fleet;  // staging of tsw_decide_fleet: v | g up, act | cell | partner | part_off down
  // tsw_audit_records scratch (grow-only): the uploaded records (T per row), the column-major transpose
  // pass A writes (T * n words), first | col | agent (the outputs), pass B's occupancy tables outside LDS
  DevBuf<unsigned long long> d_aud_rec;
  DevBuf<uint32_t> d_aud_cid, d_aud_out;
  DevBuf<unsigned long long> d_aud_tab;
  // tsw_task_timeline scratch (grow-only): pass A's event table (T * n bytes) and every word array of a
  // call in one block (timeline_layout, tsw_layout.h); records that come from the host go up into d_aud_rec,
  // the audit's (upload_records). tl_last: what tsw_probe_timeline reports of the last call.
  DevBuf<uint8_t> d_tl_ev;
  DevBuf<uint32_t> d_tl_w;
  double tl_last[5] = {};
  // tsw_astar_reserved scratch (grow-only, tsw_st_astar_host.hip): the reservation set, the running waves'
  // visited tables and overflow heaps, one block of words per batch (queries up, results down), the batch's
  // path segments with their offsets, and the packed paths. st_vis_words / st_vis_wiped / st_tag: the table
  // geometry the tags in d_st_vis belong to, how many tables of it have been wiped, and the next unused tag.
  // st_last: what tsw_probe_st_astar reports of the last call.
  DevBuf<uint64_t> d_st_res, d_st_vis, d_st_heap, d_st_segoff;
  DevBuf<uint32_t> d_st_w, d_st_seg, d_st_path;
  uint64_t st_vis_words = 0;
  uint32_t st_vis_wiped = 0, st_tag = 1;
  double st_last[5] = {};

  // stats / timing
  tsw_stats st{};
  bool timing = true;
  struct Ev {
    int cat;
    hipEvent_t a, b;
  };
  std::vector<Ev> pending;
  std::vector<hipEvent_t> pool;

  tsw_ctx() = default;
  // joins the host A* pool, drains and destroys the stream and the events; the buffers free themselves
  ~tsw_ctx();
};

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      c->err = std::string(#expr) + " failed: " + hipGetErrorString(e_);             \
      return TSW_EHIP;                                                                \
    }                                                                                 \
  } while (0)

#define RET(code, msg)   \
  do {                   \
    c->err = (msg);      \
    return (code);       \
  } while (0)

// a tsw_plan_mapd_resolved resolver must not call back into the planning context (its
// queue, result buffers and table store are in use by the suspended plan): every entry point that
// touches the context refuses such a call.
#define NOT_FROM_RESOLVER(c)                                                                         \
  do {                                                                                               \
    if ((c)->resolver) RET(TSW_EINVAL, "re-entrant call on a context inside its own next-hop resolver"); \
  } while (0)

#define TRY(expr)           \
  do {                       \
    int r_ = (expr);         \
    if (r_ != TSW_OK) return r_; \
  } while (0)

namespace tsw {

// The helpers that cross translation units; everything else is static in its file.

// tsw_ctx.hip
hipEvent_t ev_get(tsw_ctx* c);
void resolve_timing(tsw_ctx* c);
int set_device(tsw_ctx* c);
bool cell_ok(const tsw_ctx* c, uint32_t x, uint32_t y, uint32_t* cell);
bool cell_id_ok(const tsw_ctx* c, uint32_t cell);

// tsw_tables.hip
int ensure_tmp(tsw_ctx* c, size_t k);
int ensure_tables(tsw_ctx* c, const std::vector<uint32_t>& goals_in, bool tableless_ok = false);

// tsw_query.hip
int ensure_astar_scratch(tsw_ctx* c, uint32_t need = 0);
int ensure_queue(tsw_ctx* c, size_t need);
int check_err(tsw_ctx* c);
int run_astar(tsw_ctx* c, const AstarQuery* Q, uint32_t nq, bool to_tables, uint8_t* res, int32_t* lens);
int reset_pending_after(tsw_ctx* c, int rc);
int resolve_all_unknown(tsw_ctx* c, const std::vector<uint32_t>& goals, const std::vector<uint32_t>& slots);
bool eager_policy(const tsw_ctx* c, size_t new_tables);
int resolve_queue(tsw_ctx* c, const AstarQuery* Q, uint32_t nq);

// tsw_plan_host.hip: a MAPD plan call in parts (plan_impl runs them once; tsw_online_host.hip runs the
// dispatch part once per segment)
// What one k_plan launch needs beside PlanArgs. Rebuilt when a call falls back from coop to exit mode.
struct Dispatch {
  size_t lds = 0;      // the planner block's dynamic LDS
  uint32_t block = 0;  // its threads
  WorkerArgs W{};      // coop mode: the K3 workers of workgroups 1..wblocks
  uint32_t wblocks = 0;
  bool serve = false;  // host A* service on
};

// K4 spatial index: the tasks in Morton order of their (clamped) pickup points pxy (x | y << 16), cut into
// chunks of 32 entries (k_plan's KCH) with static bounding boxes and counts (tsw_plan.h PlanArgs::kbox).
// Padding entries of the last chunk stay TASK_TAKEN; no task still gives one (empty) chunk.
struct TaskIndex {
  std::vector<uint32_t> live, klt, kpos, kcnt;
  std::vector<uint2> kbox;
};

struct PlanCall {
  std::chrono::steady_clock::time_point t0;  // the call's start (tsw_stats plan_ms)
  uint32_t n = 0, m = 0, max_t = 0;
  bool want_goals = false;
  std::vector<uint32_t> vcell, pick, dlv, pxy;  // start cells; task cells (CELL_BAD: looked up lazily); pickup points
  std::vector<uint32_t> goalset;                // every cell that can become a goal
  TaskIndex ix;
  PlanArgs P{};
  Dispatch D;
  bool dispatched = false;  // D is set up (the first segment does it)
};
// the argument checks, the cells of starts and tasks, the K4 index over all m tasks
int plan_validate_index(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m, uint32_t max_t,
                        tsw_rec* out, uint32_t* goal_out, uint32_t* out_T, PlanCall* call);
// agent and task state and the index on the device; the record buffers sized for max_t + 1 columns
int plan_upload(tsw_ctx* c, PlanCall& call);
// occupancy, goal tables, queues, coop buffers and task chains; PlanArgs. chain_order (m task indices) /
// chain_at (out: m + 1 entries, chains among the first j tasks of the order): the chains in that order
int plan_tables(tsw_ctx* c, PlanCall& call, const uint32_t* chain_order = nullptr, std::vector<uint32_t>* chain_at = nullptr);
// k_plan from `init` until it reports done (one segment); failures reset pending codes
int plan_segment(tsw_ctx* c, PlanCall& call, const PlanCtl& init);
// t columns into the caller's arrays, *out_T, the call's stats
int plan_download(tsw_ctx* c, PlanCall& call, uint32_t t, tsw_rec* out, uint32_t* goal_out, uint32_t* out_T);
void plan_phase(tsw_ctx* c, const PlanCall& call, const char* what);  // TSW_PLAN_DEBUG: host-side phases

// A grow-only buffer of the context that kernels of earlier calls may still use: the stream is drained
// before the old block goes (DevBuf::grow itself never synchronises).
template <class T>
int grow_synced(tsw_ctx* c, DevBuf<T>& b, size_t need) {
  if (b.holds(need)) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  HIPCHK(b.grow(need));
  return TSW_OK;
}

// The same for the scratch of the audit, the timeline and the space-time A*: a block that does not fit is
// TSW_ENOMEM, not TSW_EHIP, and the message reads "<label> scratch (<what>): <the HIP error>".
template <class T>
int scratch_grow(tsw_ctx* c, DevBuf<T>& b, size_t need, const char* label, const char* what) {
  if (b.holds(need)) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  if (hipError_t e = b.grow(need); e != hipSuccess) {
    (void)hipGetLastError();  // the failed allocation is reported by the code, not left pending
    RET(e == hipErrorOutOfMemory ? TSW_ENOMEM : TSW_EHIP, std::string(label) + " scratch (" + what + "): " + hipGetErrorString(e));
  }
  return TSW_OK;
}

// tsw_audit_host.hip: columns 0 .. T - 1 of every row of the caller's records (n rows of `stride`) packed into
// d_aud_rec, T records per row, on the stream; label: scratch_grow's
int upload_records(tsw_ctx* c, const tsw_rec* rec, uint32_t n, uint32_t T, uint32_t stride, const char* label);

// The pickup point the nearest-pickup choice measures to, x | y << 16: the raw point with its coordinates
// clamped to 0xFFFE (plan_validate_index says why that cannot change the winner). tsw_task_timeline replays
// the choice from the same word.
inline uint32_t task_pxy(const tsw_task& t) {
  return std::min<uint32_t>(t.pickup.x, 0xFFFEu) | (std::min<uint32_t>(t.pickup.y, 0xFFFEu) << 16);
}

// Morton (Z-order) key of a point: the low 16 bits of x and y interleaved, x in the even bits.
inline uint32_t morton2(uint32_t x, uint32_t y) {
  uint32_t z = 0;
  for (uint32_t b = 0; b < 16u; ++b) z |= ((x >> b) & 1u) << (2u * b) | ((y >> b) & 1u) << (2u * b + 1u);
  return z;
}

struct Timer {
  tsw_ctx* c;
  int cat;
  hipEvent_t a = nullptr, b = nullptr;
  Timer(tsw_ctx* c_, int cat_) : c(c_), cat(cat_) {
    if (c->timing) {
      a = ev_get(c);
      b = ev_get(c);
      hipEventRecord(a, c->s);
    }
  }
  ~Timer() {
    if (a) {
      hipEventRecord(b, c->s);
      c->pending.push_back({cat, a, b});
    }
  }
};

// The passes of one call timed apart, for the tsw_probe_* of a call: N events from the pool while the context
// times (none otherwise), mark(k) on the stream between the passes, elapsed(k) from mark k to mark k + 1 once the
// stream is drained (0 without timing). The events go back to the pool on every way out of the call.
template <int N>
struct PassTimer {
  tsw_ctx* c;
  hipEvent_t ev[N] = {};
  explicit PassTimer(tsw_ctx* c_) : c(c_) {
    if (c->timing)
      for (hipEvent_t& e : ev) e = ev_get(c);
  }
  PassTimer(const PassTimer&) = delete;
  PassTimer& operator=(const PassTimer&) = delete;
  ~PassTimer() {
    for (hipEvent_t e : ev)
      if (e) c->pool.push_back(e);
  }
  void mark(int k) {
    if (ev[k]) hipEventRecord(ev[k], c->s);
  }
  double elapsed(int k) const {
    float ms = 0.f;
    if (ev[k] && ev[k + 1] && hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) ms = 0.f;
    return ms;
  }
};

}  // namespace tsw
