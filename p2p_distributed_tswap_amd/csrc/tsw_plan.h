// tsw_plan.h — arguments and resumable control block of the persistent plan kernel.
#pragma once
#include <chrono>
#include <cstddef>

#include "tsw_internal.h"
#include "tswap.h"

// What the planner and the host share by convention alone is plain C++ and comes first (tests/host/*.cpp build it
// with the host compiler alone): the host A* request ring's word layout and match test, the slots of
// PlanArgs::hflags and PlanArgs::sec_ticks, the watchdog rule and the error table. Everything below needs HIP.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TSW_RING_HD __host__ __device__ __forceinline__
#else
#define TSW_RING_HD inline
#endif

#include "tsw_place.h"

namespace tsw {

// ---- host A* service: request words (PlanArgs::hreq / hrep / hask) ----------------------------
constexpr uint32_t HOST_RING_MAX_TICKETS = 0xFFFFF0u;  // seq fits 24 bits (hrep keeps 8 for the code)

// The request word of ticket t for the pair (v, goal): seq << 40 | v << 20 | goal with seq = t + 1, so a
// zeroed word is no request (cells < 2^20).
TSW_RING_HD unsigned long long host_req_word(uint32_t ticket, uint32_t v, uint32_t goal) {
  return ((unsigned long long)(ticket + 1u) << 40) | ((unsigned long long)v << 20) | (unsigned long long)goal;
}

// Is the remembered request word w an outstanding request for (v, goal)? `tickets` = tickets taken so far
// this launch, `ring` = ring entries. False for a zeroed word, a word for another pair, a ticket not taken
// yet, and a ticket older than the ring window (ticket t's slot belongs to ticket t + ring once that is
// taken). *ticket (if given) receives the word's ticket.
TSW_RING_HD bool host_req_live(unsigned long long w, uint32_t v, uint32_t goal, uint32_t tickets, uint32_t ring,
                               uint32_t* ticket = nullptr) {
  const uint32_t seq = (uint32_t)(w >> 40);
  if (seq == 0u || seq > tickets || seq > HOST_RING_MAX_TICKETS || tickets - (seq - 1u) > ring) return false;
  if ((w & 0xFFFFFFFFFFull) != (((unsigned long long)v << 20) | (unsigned long long)goal)) return false;
  if (ticket) *ticket = seq - 1u;
  return true;
}

// Does the reply word r (seq << 8 | code, read from the slot of w's ticket) answer the pair (v, goal) the
// remembered request word w asked for? True only when w is live for (v, goal) (host_req_live), r carries
// w's seq — not that of a ticket that reused the slot after the ring wrapped, nor zero — and a code
// <= NH_STAY, which *code then receives.
TSW_RING_HD bool host_reply_match(unsigned long long w, uint32_t r, uint32_t v, uint32_t goal, uint32_t tickets,
                                  uint32_t ring, uint8_t* code) {
  if (!host_req_live(w, v, goal, tickets, ring)) return false;
  if ((r >> 8) != (uint32_t)(w >> 40) || (r & 0xFFu) > NH_STAY) return false;
  *code = (uint8_t)(r & 0xFFu);
  return true;
}

// ---- PlanArgs::hflags: host-visible (pinned, system-coherent) words, cleared by the host before every dispatch ----
enum HostFlag : int {
  HF_RESIDENT = 0,      // set by the planner block once it runs; nothing reads it
  HF_ABORT = 1,         // host watchdog: planner waits give up, its round loops exit with ERR_ABORT, workers leave
  HF_HEARTBEAT = 2,     // the planner's timestep count (PlanCtl::steps_run), stored at every step end
  HF_HOST_TAIL = 3,     // host A* service: request-ring entries the host has claimed so far (written by the host)
  HF_BAR_MISMATCH = 4,  // -DTSW_PBAR: first barrier mismatch, wave 0's line << 16 | the other wave's
  HF_BAR_LINE = 8,      // -DTSW_PBAR, + wave: the barrier's line, | 0x10000 once passed
  HF_BAR_COUNT = 24,    // -DTSW_PBAR, + wave: barriers passed
  HF_WORDS = 40,
};
constexpr int PLAN_WAVES_MAX = 16;  // waves of the planner block (PLAN_BLOCK_MAX / 64): the per-wave words above

// ---- PlanArgs::sec_ticks: the planner's diagnostic slots (TSW_PLAN_DEBUG), named for what k_plan writes ----------
// Ticks are wall-clock ticks (100 MHz) unless they say shader cycles. The first TK_STICK_COUNT slots are
// accumulated in LDS (k_plan's s_tick) and added at the planner's exit, the others are added to in place.
enum TickSlot : int {
  TK_SECTION = 0,  // + SEC_* (7: entry / copy-in): ticks per section
  TK_SECTIONS = 8,
  TK_MOVE_PASS1 = 8,      // movement rounds: ticks of the three passes
  TK_R3_WALK_HOPS = 9,    // rules: hops of rule 3's cycle walks
  TK_MOVE_PASS2 = 10,
  TK_R4_ROTATIONS = 11,   // rules: rule-4 rotations
  TK_MOVE_PASS3 = 12,
  TK_RULES_SCAN = 13,     // rules rounds: ticks of the scan, the firing, the relabel
  TK_RULES_FIRE = 14,
  TK_RULES_RELABEL = 15,
  TK_WR_LOAD = 16,        // wave rules rounds: shader cycles per part of the loop
  TK_WR_STALE = 17,
  TK_WR_FAST = 18,
  TK_WR_UPDATE = 19,
  TK_WR_SLOW = 20,
  TK_WR_ROT = 21,
  TK_WR_LOADS = 22,         // ... chunk loads
  TK_WR_FAST_FIRINGS = 23,  // ... firings on the batched / fast path
  TK_PRE1_PUBLISH = 24,     // PRE1: ticks and count of coop_publish
  TK_PRE1_PUBLISHES = 25,
  TK_RULES_INIT = 26,       // rules start: ticks of rules_init, rules_prefetch, coop_publish, and its count
  TK_RULES_PREFETCH = 27,
  TK_RULES_PUBLISH = 28,
  TK_RULES_PUBLISHES = 29,
  TK_SETTLE_SUCC = 30,      // rules settle: shader cycles of the successors pass and the walk
  TK_SETTLE_WALK = 31,
  TK_ASG_TRANSITIONS = 32,  // ASSIGN: ticks per part
  TK_ASG_COMPACT = 33,
  TK_ASG_SCAN = 34,
  TK_ASG_ACCEPT = 35,
  TK_ASG_UPDATE = 36,
  TK_ASG_BATCHES = 37,      // ... batches, agents accepted, sections
  TK_ASG_ACCEPTED = 38,
  TK_ASG_SECTIONS = 39,
  TK_WB_MARKS = 40,         // wave rules batches: shader cycles of marks, walks, apply
  TK_WB_WALKS = 41,
  TK_WB_APPLY = 42,
  TK_WB_BATCHES = 43,       // ... batches, the sum of their longest walks (hops)
  TK_WB_HOPS = 44,
  TK_WALK_IN_PRE1 = 45,     // step-start walk-ahead: steps walked in PRE1 / left to the rules phase
  TK_WALK_LEFT = 46,
  TK_WALK_WAVE0_FIRST = 47, // ... steps in which wave 0 was done before the walkers
  TK_STICK_COUNT = 48,
  TK_SCAN_INDEX = 48,       // K4 scan: ticks of its parts (the index part is no longer written)
  TK_SCAN_BOUND = 49,
  TK_SCAN_ENTRIES = 50,
  TK_SCAN_REDUCE = 51,
  TK_SCAN_PAIRS = 52,       // ... chunk-agent pairs, chunks, waves with an entry
  TK_SCAN_CHUNKS = 53,
  TK_SCAN_WAVES = 54,
  TK_SCAN_B_ONE = 55,       // ... batches of 1, 2-4, 5-8, more agents
  TK_SCAN_B_LE4 = 56,
  TK_SCAN_B_LE8 = 57,
  TK_SCAN_B_MORE = 58,
  TK_SCAN_ROUNDS = 60,      // ... rounds over the list
  TK_WALKERS = 61,          // walk-ahead on the rules rounds' idle waves: ticks from arming to the last wave's count
  TK_WALK_IN_RULES = 62,    // ... steps whose walk they finished
  TK_COUNT = 64,
};

// ---- the watchdog rule of one dispatch -----------------------------------------------------------------------
// The planner publishes its timestep count (HF_HEARTBEAT). If it stops moving for more than watchdog_ms while
// the dispatch runs, the host raises HF_ABORT, once: check() says when. A heartbeat that moves re-arms the
// timer but not the latch, and an abort word that is already set never fires again.
struct PlanWatchdog {
  using Clock = std::chrono::steady_clock;
  std::chrono::milliseconds limit;
  uint32_t last;
  Clock::time_point seen;
  bool fired = false;
  PlanWatchdog(uint32_t watchdog_ms, uint32_t heartbeat, Clock::time_point now)
      : limit(watchdog_ms), last(heartbeat), seen(now) {}
  bool check(uint32_t heartbeat, uint32_t abort_word, Clock::time_point now) {
    if (heartbeat != last) {
      last = heartbeat;
      seen = now;
      return false;
    }
    if (fired || abort_word || !(now - seen > limit)) return false;
    fired = true;
    return true;
  }
};

// ---- PlanCtl::err -> return code -----------------------------------------------------------------------------
// Tested in this order: the first row sharing a bit with err gives the call's code. msg: the fixed error
// string; nullptr where the host composes one (the stopped planner's position, the raw bits).
struct PlanErrRow {
  uint32_t bits;
  int code;
  const char* msg;
};
constexpr PlanErrRow PLAN_ERR_TABLE[] = {
    {ERR_ABORT, TSW_EINVAL, nullptr},
    {ERR_BAD_PICKUP, TSW_EINVAL, "assigned task's pickup is off-grid or blocked (reference panics at tswap.rs:136)"},
    {ERR_BAD_DELIVERY, TSW_EINVAL,
     "reached pickup's task delivery is off-grid or blocked (reference panics at tswap.rs:112)"},
    {ERR_NO_TABLE, TSW_EINVAL, nullptr},
    {0xFFFFFFFFu, TSW_EOVERFLOW, nullptr},
};
inline const PlanErrRow* plan_err_row(uint32_t err) {  // nullptr: no error
  for (const PlanErrRow& r : PLAN_ERR_TABLE)
    if (err & r.bits) return &r;
  return nullptr;
}

}  // namespace tsw

#if defined(__HIPCC__)

namespace tsw {

enum : uint32_t {
  SEC_ASSIGN = 0,
  SEC_PRE1 = 1,
  SEC_RULES = 2,
  SEC_PRE2 = 3,
  SEC_MOVE = 4,
  SEC_RECORD = 5,
  SEC_DONE = 6,
};
enum : uint32_t { PLAN_RUNNING = 0, PLAN_NEED_QUERIES = 1, PLAN_DONE = 2, PLAN_ERROR = 3 };
enum : uint32_t { MODE_MAPD = 0, MODE_STEP = 1 };
// k_plan's workgroup size cap (its __launch_bounds__). The planner's live state peaks at ~195 VGPRs; at
// 1,024 threads (4 waves per SIMD) a wave gets 128, so ~60 VGPRs spill, but its latency-bound per-agent
// passes (K4 scan, walk-ahead, movement rounds) run one agent per thread on C3. Round 6 measured the
// spill-free 512-thread bound 3-6 % slower end to end (ASSIGN +25 ms, PRE1 +40 ms per busy C3 plan:
// two agents per thread, one after the other), profiles/r6/ab_r6_pg.txt.
constexpr uint32_t PLAN_BLOCK_MAX = 1024;
constexpr uint32_t TASK_TAKEN = 0xFFFFFFFFu;  // PlanArgs::live entry of an assigned task

// Persisted in device memory between launches (exact resume point).
struct PlanCtl {
  uint32_t t;         // timesteps recorded so far
  uint32_t section;   // SEC_*
  uint32_t i;         // rules: cursor (first agent not yet scanned); movement: DEC initialised
  uint32_t in_chase;  // (unused, kept for layout)
  uint32_t b;
  uint32_t ap_len;
  uint32_t chase_id;
  uint32_t status;    // PLAN_*
  uint32_t qcount;    // pairs enqueued for K3
  uint32_t err;       // ERR_* bits
  uint32_t unused;    // tasks not yet used
  uint32_t max_t;     // stop when t > max_t
  uint32_t miss;      // serial movement scan: 1 = unresolved next hop, 2 = goal without table
  uint32_t steps_run;
  uint32_t rule_rounds;  // first-firing rounds executed (rules phase)
  uint32_t move_rounds;  // decidability rounds executed (movement phase)
  uint32_t relabel_full;  // rules-phase relabels by block-wide pointer doubling
  uint32_t relabel_inc;   // ... and incremental ones (walks from the changed agents)
};

struct PlanArgs {
  uint32_t n, m, W, ncell;
  uint32_t mode, agents_lds, occ_lds, tasks_lds;
  uint32_t has_dups, prefetch;  // prefetch: enqueue rules-round next hops up front (rules_prefetch)
  uint32_t f_lds;               // F1/F2 carved in LDS although the agent arrays are global
  uint32_t mu_lds;              // occ_lds and the movement rounds' MU words in LDS too
  uint32_t part_lds;            // !agents_lds: PART_* agent arrays carved in LDS anyway (flat accesses)
  uint32_t wave_rules_max;      // rules rounds run in wave 0 alone when n <= this
  uint32_t walk_cap;            // wave rules batches: longest successor walk a batched firing may take
  uint32_t wide_prefetch;       // 0: off; else also (succ cell, goal) of every agent, path walked this many hops ahead
  uint32_t wide_hi, wide_lo;    // coop mode: step-start walk-ahead hops when the speculative backlog is small / large
  uint32_t spec_hi;             // coop mode: backlog (queued, unclaimed speculative pairs) counted as small up to this
  uint32_t dag_prefetch;        // walk-ahead also queues the shortest-path successors of the first unresolved cell
  uint32_t dag_width;           // ... at most this many cells per DAG level (0: 4)
  uint32_t urgent_hops;         // coop: walk-ahead pairs within this many hops (pickup pairs within + 1) go to the needed queue
  uint32_t ab_flags;            // diagnostic A/B switches (Tunables::ab_flags; 0 in the product build)
  uint32_t t0_delay_ticks;      // diagnostic: idle after step 0's assignment (100 MHz ticks)
  uint32_t prefetch_ext;        // bit 0: DAG from an agent's own unresolved cell; bit 1: walk on past the pickup
  const uint8_t* dt;            // detour bytes of the table store (nstride per slot; tsw_internal.h), for dag_prefetch
  const uint8_t* nbmask;        // per cell: bit d = neighbour in direction d is free
  uint32_t* v;
  uint32_t* g;
  uint8_t* st;
  int32_t* task;
  int32_t* gt;    // per agent goal-table slot (global copy, used when agents are not in LDS)
  uint32_t* succ; // per agent successor / target cell (global copy)
  uint8_t* nhc;   // per agent next-hop code (global copy)
  uint8_t* dec;   // per agent movement-round state (persisted across relaunches)
  uint8_t* onc;   // per agent rule-4 cycle label (global copy)
  uint8_t* candc; // per agent rule-3 next-hop prefetch (global copy)
  uint32_t* f1;   // pointer-doubling buffers, n + 1 entries each (global copy)
  uint32_t* f2;
  uint32_t* mk;   // per agent batch marks of the wave rules rounds (global copy, n + 1 entries)
  uint32_t* occ;  // per cell occupancy
  uint64_t* mu;   // per cell round-tagged lowest undecided targeting agent (global copy)
  // K4 spatial index (tsw_plan_host.hip plan_impl): the tasks in Morton order of their pickup points (coordinates
  // clamped to 0xFFFE). live[pos] = pickup point (x | y << 16) while unused, TASK_TAKEN once assigned; klt[pos] =
  // the task index; kpos[task] = its position; chunks of KCH positions have a static bounding box kbox
  // (x0 | y0 << 16, x1 | y1 << 16) and a count of untaken entries kcnt. Padding entries are TASK_TAKEN.
  uint32_t* live;
  const uint32_t* klt;
  const uint32_t* kpos;
  const uint2* kbox;
  uint32_t* kcnt;
  uint32_t kchunks;
  const uint32_t* pick;
  const uint32_t* dlv;
  const int32_t* goal_tab;
  uint8_t* nh;
  uint64_t nstride;
  AstarQuery* Q;
  uint32_t qcap;
  uint64_t* rec;
  uint32_t* grec;
  PlanCtl* ctl;
  unsigned long long* sec_ticks;  // [TK_COUNT] diagnostics: ticks per section, sub-phase ticks and counters (TickSlot)
  uint32_t dbg;                   // sub-phase ticks on (TSW_PLAN_DEBUG)
  uint32_t* dtag;                 // diagnostics (TSW_PLAN_DEBUG): per agent, what changed it since PRE1 (CoopCtl::dbg_tag)
  // coop mode: K3 runs concurrently in the dispatch's worker workgroups (tsw_worker.h); Q is the needed queue (qcap entries for the
  // whole launch), QS the speculative one; missing next hops are waited for instead of exiting
  uint32_t coop;
  AstarQuery* QS;
  uint32_t qscap;
  AstarQuery* QH;  // hot task chains: (pickup, delivery) of every task as it is assigned (qhcap = m entries)
  uint32_t qhcap;
  // predicted task chains: (delivery cell, agent) of an agent that picks up a task (and, with bit 1 of
  // predict, of a delivering agent whose goal a rule changed); a worker predicts the task the agent will
  // be assigned at that cell — the nearest untaken pickup now — and walks that task's chain (tsw_worker.h)
  uint2* QP;
  uint32_t qpcap;
  uint32_t predict;     // bit 0: at pickups, bit 1: at goal changes of delivering agents
  uint32_t* pred;       // diagnostics (TSW_PLAN_DEBUG): per agent, the task last predicted for it
  uint4* wf;            // per agent: step-start walk-ahead frontier (cell at the walk, goal, stopping cell, its hop); nullptr: off
  CoopCtl* cc;
  uint32_t* hflags;  // [HF_WORDS] host-visible (pinned, system-coherent) words (HostFlag)
  // host A* service (coop mode, tsw_plan_host.hip host_serve_one): rings of hring entries (a power of two;
  // 0 = service off) in mapped coherent host memory. A planner thread waiting for a needed pair takes
  // ticket t (0, 1, ... per launch) and stores seq << 40 | v << 20 | goal into hreq[t % hring] with
  // seq = t + 1: one 64-bit system-scope store carries the whole request, so no head word and no
  // release (an L2 write-back) is needed — the host polls the next slot for its seq. The host answers
  // with seq << 8 | code in hrep[t % hring]. The planner never waits for the host: a missing, late or
  // foreign reply is ignored and the code arrives from a K3 worker as before.
  unsigned long long* hreq;
  uint32_t* hrep;
  uint32_t hring;
  // early asks (round 9): a pair the walk-ahead queues as urgent is put on the request ring at once, a
  // step before its code is read, and its request word is remembered per agent — hask[2k]: the
  // walk-ahead pair, hask[2k + 1]: the pickup-arrival pair (zeroed per launch; nullptr: off).
  // refresh_codes takes the reply when it finds the agent's code unresolved, coop_wait spins on the
  // remembered ticket instead of asking again (host_req_live / host_reply_match above).
  // hearly: TSW_HOST_ASTAR_EARLY (1; 2 = diagnostic: coop_wait neither asks nor polls the host, so
  // every host code taken came through refresh_codes).
  unsigned long long* hask;
  uint32_t hearly;
  // new hops a step-start walk reads past its cached frontier (wf) per timestep (0: no budget, the whole depth)
  uint32_t walk_step;
};

// The PART_* bits of part_lds and the placement's byte formulas (part_lds_bytes, plan_lds_bytes): tsw_place.h.
hipError_t launch_occ(const uint32_t* v, uint32_t n, uint32_t* occ, uint32_t* cnt, uint32_t ncell, uint32_t* dups,
                      hipStream_t s);
// Coop-mode K3 workers (tsw_worker.h) run in the workgroups 1.. of the plan dispatch: claim queued
// pairs from cc's queues (needed first), resolve them with the exact A* and write the next-hop code;
// exit when the planner has stopped and the needed queue is drained (speculative leftovers are
// abandoned).
struct WorkerArgs {
  DevGrid G;
  CoopCtl* cc;
  const AstarQuery* QN;
  const AstarQuery* QS;
  const AstarQuery* QT;  // task chains: (pickup, delivery) of every task, walked hop by hop
  const AstarQuery* QH;  // hot task chains: the same walk for tasks the planner has just assigned (first)
  const uint2* QP;       // predicted task chains: (delivery cell, agent); the chain of the predicted task (PlanArgs::QP)
  const uint32_t* klive;  // K4 spatial index (PlanArgs::live / klt / kbox / kcnt), read for predictions
  const uint32_t* klt;
  const uint2* kbox;
  const uint32_t* kcnt;
  uint32_t kchunks;
  const uint32_t* pick;
  const uint32_t* dlv;
  const int32_t* goal_tab;
  uint32_t* pred;         // diagnostics: per agent, the task last predicted for it (nullptr: off)
  uint8_t* nh;
  uint64_t nstride;
  uint32_t hcap;      // LDS heap entries
  uint32_t gs_lds;    // 0: u32 g-scores in the global slots, 1: u32 in LDS, 2: bytes in LDS
  uint32_t stage_fb;  // free-cell bitmap staged in LDS (else read from global memory / L2)
  uint32_t tmask;     // workers with (blockIdx & tmask) == tmask also take task-chain jobs
  uint32_t preempt;   // chain workers serve queued needed / speculative pairs between hops
  uint32_t chain_hops;  // hops a chain worker resolves per task chain (0: the whole pickup -> delivery path)
  const uint32_t* hflags;  // host watchdog words (HF_ABORT)
  uint32_t* gs_all;   // per-wave global g-score slots (tier 2 / tier 3), ncell u32 each
  uint32_t* epochs;   // per-slot tag epochs
  uint64_t* heaps;    // per-wave global heaps (tier 3), ghcap entries each
  uint32_t ghcap;
  uint32_t avoid_xcc;  // workers placed on the planner's XCD exit at once (its L2 stays the planner's)
  uint32_t wpb;        // worker waves per workgroup (each owns lds_per_wave bytes of the dynamic LDS)
  uint32_t lds_per_wave;
  uint32_t nworkers;   // worker waves in the dispatch (<= the global g-score / heap slots)
  // exact DAG early exit of the A* (tsw_astar.h): 0 off, 1 the goal's detour bytes staged in this
  // wave's LDS (after the free bitmap), 2 the goal's detour bytes read from the table store
  uint32_t dag;
  const uint8_t* dt;     // detour bytes of the table store, nstride per goal slot
  uint32_t dag_mask;     // the DAG test runs when (pops & dag_mask) == 0
  uint32_t stale_steps;  // speculative entries queued more than this many timesteps ago are dropped (0: never)
  uint32_t reg_heap;     // A* heaps up to this many entries live in registers (0: LDS array only; <= 63)
  uint32_t wake_gate;    // idle workers with (wid & wake_gate) == (pub & wake_gate) rescan at once on a publish
  uint32_t slow_mask, slow_mult;  // idle workers with (wid & slow_mask) != 0 poll slow_mult times less often
  unsigned long long idle_ticks;  // a worker idle this long (100 MHz ticks) exits (5 s)
};
// Worker placement (WorkerCfg, worker_config, worker_layout): tsw_place.h.

// The plan dispatch: workgroup 0 runs k_plan's planner (block threads, lds bytes of dynamic LDS);
// with W (coop mode) workgroups 1..worker_blocks run W->wpb K3 worker waves each.
hipError_t launch_plan(const PlanArgs& P, PlanArgs* d_args, const WorkerArgs* W, uint32_t worker_blocks, size_t lds,
                       uint32_t block, hipStream_t s);
// One instantiation of k_plan, launched. AG: every agent array in LDS; OC: the occupancy grid; MUL: with OC, the
// movement rounds' MU words too; PG (!AG): the fixed subset PART_PG of the agent arrays. Defined in tsw_plan_kernel.h
// and explicitly instantiated once per flag tuple, each in a translation unit of its own (tsw_plan_v0 .. v6.hip: an
// instantiation takes minutes of hipcc, and the build compiles them in parallel). launch_plan's ladder is the one
// place that maps a PlanArgs to its tuple; a tuple without a translation unit does not link.
template <bool AG, bool OC, bool MUL, bool PG>
hipError_t launch_plan_t(const PlanArgs* P, const WorkerArgs& W, uint32_t grid, size_t lds, uint32_t block,
                         hipStream_t s);

}  // namespace tsw

#endif  // __HIPCC__
