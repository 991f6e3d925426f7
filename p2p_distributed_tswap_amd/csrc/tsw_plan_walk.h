// tsw_plan_walk.h — k_plan's speculative prefetches: the rules phase's candidate pairs, the shortest-path DAG past an
// unresolved cell, and the step-start walk-ahead along every agent's path (in PRE1, or on the idle waves of the rules
// rounds).
#pragma once
#include "tsw_plan_queue.h"

namespace tsw {

namespace {

// Parallel, after rules_init: the next hops a firing of this rules round (or the movement phase
// after it) could need. A rule-3
// swap hands succ(k) the goal of k (tswap.rs:199-202); a rule-4 rotation hands every cycle
// member the goal of its predecessor on the cycle (:241-249) — both are the pair
// (cell of succ(k), goal of k) for a firing candidate k. Every unresolved such pair is queued
// speculatively (no exit): the planner exits only when a firing actually needs a code, and
// that one K3 launch then resolves everything queued so far. Half the queue stays free for the
// pairs an exit needs.
__device__ void rules_prefetch(const PlanArgs& P, const Arrays& S, uint32_t* s_q) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  for (uint32_t k = tid; k < P.n; k += bd) {
    if (spec_full(P, s_q)) break;
    const int32_t tab = S.GT[k];
    if (tab < 0) continue;
    // k's own next hop from the cell it moves to: read by the movement phase when k moved
    // earlier in the same step (tswap.rs:263-273, later agents see earlier moves) and by the
    // next step's refresh
    const uint8_t c = S.NHC[k];
    if (c < NH_STAY && S.V[k] != S.G[k]) {
      const uint32_t u = step_cell(S.V[k], c, P.W);
      if (u != S.G[k] && P.nh[(uint64_t)tab * P.nstride + u] == NH_UNKNOWN) prefetch_pair(P, u, S.G[k], tab, s_q);
    }
    const uint32_t s = S.SUCC[k];
    if (s == SUCC_TERM || s == k) continue;
    if (!P.wide_prefetch && !(S.ONC[k] || S.V[s] == S.G[s])) continue;
    const uint32_t vs = S.V[s];
    if (P.nh[(uint64_t)tab * P.nstride + vs] == NH_UNKNOWN) prefetch_pair(P, vs, S.G[k], tab, s_q);
  }
  PBAR();
}

// rules_prefetch restricted to the agents a firing changed (rule 3: b and s, rule 4: the cycle):
// only their goals, hence their next hops and successors, moved, so only their pairs are new.
// After rules_init (SUCC valid).
__device__ uint32_t walk_prefetch(const PlanArgs& P, uint32_t* s_q, uint32_t u, uint32_t g, int32_t tab,
                                  uint32_t hops, unsigned long long* hslot, uint32_t h0 = 0u, uint32_t* end = nullptr,
                                  uint32_t* endh = nullptr);
__device__ void dag_prefetch(const PlanArgs& P, uint32_t* s_q, uint32_t u, uint32_t g, int32_t tab);

// coop mode: agent k will be idle at `cell` (its delivery): a worker predicts its next task and walks that
// task's pickup -> delivery chain ahead of the assignment (s_q[Q_PRED]: entries queued, PlanArgs::QP)
__device__ __forceinline__ void predict_push(const PlanArgs& P, uint32_t* s_q, uint32_t cell, uint32_t k) {
  const uint32_t qi = atomicAdd(&s_q[Q_PRED], 1u);
  if (qi < P.qpcap) P.QP[qi] = make_uint2(cell, k);
}

__device__ __forceinline__ void prefetch_changed(const PlanArgs& P, const Arrays& S, uint32_t* s_q, uint32_t k) {
  // delivering: a rule handed the agent another delivery cell, so its next task changes with it
  if ((P.predict & 2u) && P.QP && P.st[k] == ST_TO_DELIVERY) predict_push(P, s_q, S.G[k], k);
  if (spec_full(P, s_q)) return;
  // heading to a pickup: its new goal is where the state machine switches it to the delivery
  // (tswap.rs:113-118) — the (goal cell, delivery) pair, a step before nextnext_prefetch would queue it
  if (P.mode != MODE_STEP && P.m > 0 && P.st[k] == ST_TO_PICKUP) {
    const int32_t tk = P.task[k];
    if (tk >= 0 && (uint32_t)tk < P.m) {
      const uint32_t pc = S.G[k], dc = P.dlv[tk];
      const int32_t dt = dc == CELL_BAD ? -1 : P.goal_tab[dc];
      if (dt >= 0 && pc != dc && P.nh[(uint64_t)dt * P.nstride + pc] == NH_UNKNOWN) prefetch_pair(P, pc, dc, dt, s_q);
    }
  }
  const int32_t tab = S.GT[k];
  if (tab < 0) return;
  const uint8_t c = S.NHC[k];
  if (S.V[k] != S.G[k] && (P.prefetch_ext & 4u)) {
    // the agent's new path: walked ahead (and the DAG past its first unresolved cell) now, a step
    // before the next step's walk-ahead would queue it
    if (c < NH_STAY)
      walk_prefetch(P, s_q, step_cell(S.V[k], c, P.W), S.G[k], tab, P.wide_prefetch ? P.wide_prefetch : 1u,
                    P.hask ? P.hask + 2u * k : nullptr);
    else if (c > NH_STAY && P.dag_prefetch) dag_prefetch(P, s_q, S.V[k], S.G[k], tab);
  } else if (c < NH_STAY && S.V[k] != S.G[k]) {
    const uint32_t u = step_cell(S.V[k], c, P.W);
    if (u != S.G[k] && P.nh[(uint64_t)tab * P.nstride + u] == NH_UNKNOWN) prefetch_pair(P, u, S.G[k], tab, s_q);
  }
  const uint32_t s = S.SUCC[k];
  if (s == SUCC_TERM || s == k) return;
  const uint32_t vs = S.V[s];
  if (P.nh[(uint64_t)tab * P.nstride + vs] == NH_UNKNOWN) prefetch_pair(P, vs, S.G[k], tab, s_q);
}

__device__ void rules_prefetch_list(const PlanArgs& P, const Arrays& S, uint32_t* s_q, const uint32_t* lst,
                                    uint32_t cnt) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  for (uint32_t i = tid; i < cnt; i += bd) prefetch_changed(P, S, s_q, lst[i]);
  PBAR();
}

// The shortest-path DAG toward goal g past cell u (u's own pair is queued by the caller): whichever
// neighbour u's code picks lies one step closer to the goal (every get_path is a shortest path), so
// the DAG ahead of u is where the agent goes next. Its cells are queued level by level (frontier
// capped at DAG_WIDTH; a resolved cell contributes only the cell its code points at), so a path
// resolves several cells per A* latency instead of one.
__device__ void dag_prefetch(const PlanArgs& P, uint32_t* s_q, uint32_t u, uint32_t g, int32_t tab) {
  constexpr uint32_t DAG_WIDTH = 16;  // array bound; P.dag_width caps the frontier (default 4)
  const uint32_t dwid = P.dag_width ? min(P.dag_width, DAG_WIDTH) : 4u;
  const uint8_t* dtb = P.dt + (uint64_t)tab * P.nstride;
  const uint8_t* ht = P.nh + (uint64_t)tab * P.nstride;
  const uint32_t gy = g / P.W, gx = g - gy * P.W;
  // K1 distance from the detour byte: |c - g|_1 + 2 * detour, ~0 when unknown (blocked / unreachable /
  // saturated: the speculative walk stops there)
  auto dist_of = [&](uint32_t c) -> uint32_t {
    const uint32_t b = dtb[c];
    if (b == DT_NONE) return 0xFFFFFFFFu;
    const uint32_t y = c / P.W, x = c - y * P.W;
    return (x > gx ? x - gx : gx - x) + (y > gy ? y - gy : gy - y) + 2u * b;
  };
  uint32_t fr[DAG_WIDTH], nf = 1;
  fr[0] = u;
  for (uint32_t lv = 0; lv < P.dag_prefetch && nf > 0u; ++lv) {
    uint32_t nx[DAG_WIDTH], nn = 0;
    auto add = [&](uint32_t w) {
      for (uint32_t i = 0; i < nn; ++i)
        if (nx[i] == w) return;
      if (nn < dwid) nx[nn++] = w;
    };
    for (uint32_t i = 0; i < nf; ++i) {
      const uint32_t x = fr[i];
      const uint8_t cx = ht[x];
      if (cx < NH_STAY) {  // resolved: the agent's path continues at one cell
        const uint32_t w = step_cell(x, cx, P.W);
        if (w != g) add(w);
        continue;
      }
      if (cx == NH_STAY) continue;
      const uint32_t dx = dist_of(x);
      if (dx == 0xFFFFFFFFu) continue;
      const uint8_t nb = P.nbmask[x];
#pragma unroll
      for (uint32_t d = 0; d < 4u; ++d) {
        if (!((nb >> d) & 1u)) continue;
        const uint32_t w = step_cell(x, d, P.W);
        if (w == g || dist_of(w) + 1u != dx) continue;
        if (ht[w] == NH_UNKNOWN) prefetch_pair(P, w, g, tab, s_q);
        add(w);
      }
    }
    for (uint32_t i = 0; i < nn; ++i) fr[i] = nx[i];
    nf = nn;
  }
}

// Walk the resolved codes toward g from cell u, which lies h0 resolved hops past the agent's next cell,
// until hop `hops`; queue the first unresolved pair (and the DAG past it). Returns the hops left when the
// walk reached g, else 0. *end / *endh (if given): the cell the walk stopped at and its hop index.
// hslot: the walking agent's early-ask slot (PlanArgs::hask) — an urgent pair is then also asked of the host
// now (host_ask_early) — or nullptr where the walk is no agent's own path or early asks are off.
__device__ uint32_t walk_prefetch(const PlanArgs& P, uint32_t* s_q, uint32_t u, uint32_t g, int32_t tab,
                                  uint32_t hops, unsigned long long* hslot, uint32_t h0, uint32_t* end, uint32_t* endh) {
  uint32_t h = h0;
  uint32_t left = 0;
  for (; h < hops; ++h) {
    if (u == g) {
      left = hops - h;
      break;
    }
    const uint8_t cu = P.nh[(uint64_t)tab * P.nstride + u];
    if (cu == NH_UNKNOWN || cu == NH_PENDING || cu == NH_PENDING_S) {
      // a pair the agent reads within urgent_hops steps goes to the needed queue (served before the
      // speculative backlog, which on wh10k holds ~500 pairs when a wait starts); farther ones are speculative
      if (P.coop && h < P.urgent_hops) {
        urgent_pair(P, u, g, tab, s_q, cu);
        if (hslot) host_ask_early(P, s_q, u, g, hslot);
      } else if (cu == NH_UNKNOWN) prefetch_pair(P, u, g, tab, s_q);
      if (P.dag_prefetch) dag_prefetch(P, s_q, u, g, tab);
      break;
    }
    if (cu >= NH_STAY) break;  // a stay code
    u = step_cell(u, cu, P.W);
  }
  if (end) {
    *end = u;
    *endh = h;
  }
  return left;
}

// The walkers' last step (round 14) — publishing without wave 0, at the time the PRE1 walk publishes (thread 0,
// behind its barrier): each walker wave releases its stores (queue entries, PENDING marks) at workgroup scope —
// the wave's, whichever lanes wrote them — then adds 1 to the count s_q[Q_WALK_DONE] in LDS (acquire + release); the wave
// whose add completes the count has thereby acquired every walker's stores, and coop_publish's agent-scope
// release stores of the heads carry them to the workers. Only that lane touches s_q[2..9] now: the other walkers
// are done, wave 0 does not while it fires (see the call in the rules phase), and the block's next publish lies
// behind the barrier that closes the rounds' pass. It also clears the owed step: the rules section can be entered
// again in the same step (after a miss's refresh), and the walk is owed once. Called by every wave but wave 0
// after its walk (waves 1.. of the block are the walkers, all of them); a function of its own, out of line:
// inline in nextnext_prefetch its registers became that function's (88 VGPRs against 85), called from it 100.
__device__ __noinline__ void walk_done(const PlanArgs& P, uint32_t* s_q) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if ((threadIdx.x & 63u) == 0u && __hip_atomic_fetch_add(&s_q[Q_WALK_DONE], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) +
                                           2u == (blockDim.x >> 6)) {
    s_q[Q_WALK_OWED] = 0u;
    coop_publish(P, s_q);
    if (PLAN_DBG && P.sec_ticks) {  // diagnostics: armed -> the last walker wave's count, when that was, and
      const uint32_t now = (uint32_t)wall_clock64();  // one more walk finished and published in RULES
      atomicAdd(&P.sec_ticks[TK_WALKERS], (unsigned long long)(now - s_q[Q_WALK_ARMED_CLK]));
      atomicAdd(&P.sec_ticks[TK_WALK_IN_RULES], 1ull);
      s_q[Q_WALK_DONE_CLK] = now | 1u;
    }
  }
}

// Parallel: the next hop of every agent from the cell its resolved code points at (the pair the
// movement phase or the next step reads after the agent moves, tswap.rs:263-273), walked `hops`
// resolved cells ahead; speculative, bounded by half the queue like rules_prefetch.
//  * an agent whose own code is still unresolved (just assigned, goal swapped) gets the DAG past its
//    cell queued now, beside its needed pair, instead of one cell per step after each wait
//    (prefetch_ext bit 0);
//  * an agent heading to a pickup whose walk reaches it continues along the delivery leg: the
//    state machine switches its goal there (tswap.rs:113-118) (prefetch_ext bit 1).
// A range function: the calling thread walks agents first, first + stride, ...; no barrier here (the caller
// places it). Called by the whole block (PRE1) the range is (tid, blockDim).
// WALK_LIVE in hops: called by the waves that idle while wave 0 fires rules (round 14, the call in the rules
// phase says what may be read): the goal is read once, its table slot comes from goal_tab and never from GT, and
// an agent whose code reads dirty or unresolved is left to the phase's own prefetch. The walkers are waves 1..
// of the block, and together they cover every agent (wave 0's included): the range is (tid - 64, blockDim - 64);
// wave 0 does not call. The range is worked out here and the mode is a bit of the run-time hop count, not parameters: two more
// arguments cost the function three VGPRs (88 against the 85 its callers' allocation was measured with), and
// with a compile-time constant that differs between the two calls the compiler clones the function per call — a
// clone hipcc 7's back end rejects ("Illegal instruction detected" at prefetch_pair's volatile read of s_q).
constexpr uint32_t WALK_LIVE = 0x80000000u;
__device__ __noinline__ void nextnext_prefetch(const PlanArgs& P, const Arrays& S, uint32_t* s_q, uint32_t hops) {
  const bool live = (hops & WALK_LIVE) != 0u;
  hops &= ~WALK_LIVE;
  uint32_t first = threadIdx.x, stride = blockDim.x;
  if (live) {
    if (first < 64u) return;
    first -= 64u;
    stride -= 64u;
  }
  // both are the same in every lane of a wave: held in scalar registers, they make up for the two vector
  // registers the range costs (the function stays at the parent's 85)
  stride = (uint32_t)__builtin_amdgcn_readfirstlane((int)stride);
  hops = (uint32_t)__builtin_amdgcn_readfirstlane((int)hops);
  for (uint32_t k = first; k < P.n; k += stride) {
    if (spec_full(P, s_q)) break;
    // heading to a pickup: the pair the state machine needs on arrival (goal := delivery,
    // tswap.rs:113-118) is known since the assignment — (arrival cell, delivery goal). The arrival
    // cell is the agent's current goal: rule-3/4 swaps may have traded the task's pickup cell away.
    const uint32_t gk = *(volatile const uint32_t*)&S.G[k];  // the agent's goal: this one read (see `live`)
    uint32_t pc = 0, dc = 0;
    int32_t dtab = -1;
    if (P.mode != MODE_STEP && P.m > 0 && P.st[k] == ST_TO_PICKUP) {
      const int32_t tk = P.task[k];
      if (tk >= 0 && (uint32_t)tk < P.m) {
        pc = gk;
        dc = P.dlv[tk];
        const int32_t dt = dc == CELL_BAD ? -1 : P.goal_tab[dc];
        if (dt >= 0 && pc != dc) {
          dtab = dt;
          const uint8_t cp = P.nh[(uint64_t)dt * P.nstride + pc];
          const uint32_t vk = S.V[k], W = P.W;
          const uint32_t vx = vk % W, vy = vk / W, px = pc % W, py = pc / W;
          const uint32_t man = (vx > px ? vx - px : px - vx) + (vy > py ? vy - py : py - vy);
          // arriving within urgent_hops + 1 steps (Manhattan bounds the path from below): needed queue
          if (P.coop && man <= P.urgent_hops + 1u && (cp == NH_UNKNOWN || cp == NH_PENDING_S)) {
            urgent_pair(P, pc, dc, dt, s_q, cp);
            if (P.hask) host_ask_early(P, s_q, pc, dc, P.hask + 2u * k + 1u);
          } else if (cp == NH_UNKNOWN) prefetch_pair(P, pc, dc, dt, s_q);
        }
      }
    }
    const int32_t tab = live ? P.goal_tab[gk] : S.GT[k];
    const uint8_t c = S.NHC[k];
    if (tab < 0 || S.V[k] == gk || c == NH_STAY) continue;
    if (c > NH_STAY) {  // own pair unresolved (queued as needed by the refresh); live: the agent fired just now
      if (!live && (P.prefetch_ext & 1u) && P.dag_prefetch) dag_prefetch(P, s_q, S.V[k], gk, tab);
      continue;
    }
    // Resolved codes never change, so the path from the agent's next cell is fixed while its goal is: the
    // walk resumes at last step's stopping cell (P.wf: cell at that walk, goal, stopping cell, its hop
    // index). An agent that moved since went one hop along that path, so the index drops by one.
    uint32_t u0 = step_cell(S.V[k], c, P.W), h0 = 0;
    const uint32_t vk = S.V[k];
    if (P.wf) {
      const uint4 f = P.wf[k];
      // moved: exactly one hop along the cached path (goals can change and change back in between)
      bool on = f.y == gk && f.x == vk;
      if (f.y == gk && f.x != vk && f.x < P.ncell) {
        const uint8_t cf = P.nh[(uint64_t)tab * P.nstride + f.x];
        on = cf < NH_STAY && step_cell(f.x, cf, P.W) == vk;
      }
      if (on) {
        const uint32_t hp = f.x == vk ? f.w : (f.w > 0u ? f.w - 1u : 0u);
        if (hp > 0u) {
          u0 = f.z;
          h0 = hp;
        }
      }
    }
    // A hop budget per step (round 10): the walk reads at most walk_step hops past its cached frontier and goes
    // on next step, up to the same depth; the agent moves one hop per step, so the frontier gains walk_step - 1.
    // The delivery-leg continuation below is not cached, so it gets what is left of this step's budget: at most
    // walk_step hops past the pickup (the workers' task chains resolve that leg as well).
    uint32_t ue = u0, he = h0;
    const uint32_t hlim = (P.walk_step && P.wf) ? min(hops, h0 + P.walk_step) : hops;
    const uint32_t left =
        h0 >= hops ? 0u : walk_prefetch(P, s_q, u0, gk, tab, hlim, P.hask ? P.hask + 2u * k : nullptr, h0, &ue, &he);
    if (P.wf) P.wf[k] = make_uint4(vk, gk, ue, he);
    if (left > 0u && dtab >= 0 && (P.prefetch_ext & 2u)) walk_prefetch(P, s_q, pc, dc, dtab, left, nullptr);
  }
}

}  // namespace

}  // namespace tsw
