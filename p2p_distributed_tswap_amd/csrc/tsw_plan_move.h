// tsw_plan_move.h — k_plan's movement phase: the serial scan for instances with shared start cells (walk_move) and the
// MOVE section's decidability rounds.
#pragma once
#include "tsw_plan_queue.h"

namespace tsw {

namespace {

// Serial movement phase (tswap.rs:257-285) — used when cells are shared by several agents
// (duplicate start cells); false on an unresolved next hop.
__device__ bool walk_move(const PlanArgs& P, const Arrays& S, PlanCtl& ctl) {
  const uint32_t n = P.n, W = P.W;
  uint32_t i = ctl.i;
  for (; i < n; ++i) {
    const uint32_t vi = S.V[i], gi = S.G[i];
    if (vi == gi) continue;
    const int code = lookup_code(P, S, i);
    if (code < 0) {
      ctl.miss = code == -2 ? 2u : 1u;
      ctl.i = i;
      return false;
    }
    const uint32_t u = step_cell(vi, (uint32_t)code, W);
    const uint32_t o = S.OCC[u];
    if (o == OCC_NONE) {  // rule 2: move
      S.V[i] = u;
      S.NHC[i] = NHC_DIRTY;
      S.OCC[u] = i;
      if (S.OCC[vi] & OCC_FLAG) occ_rescan(P, S, vi);
      else S.OCC[vi] = OCC_NONE;
    } else if ((o & OCC_IDX) != i) {
      const uint32_t j = o & OCC_IDX;
      const uint32_t vj = S.V[j], gj = S.G[j];
      if (vj != gj) {
        const int cj = lookup_code(P, S, j);
        if (cj < 0) {
          ctl.miss = cj == -2 ? 2u : 1u;
          ctl.i = i;
          return false;
        }
        if (step_cell(vj, (uint32_t)cj, W) == vi) {  // mutual swap (:273-278)
          S.V[i] = vj;
          S.V[j] = vi;
          S.NHC[i] = NHC_DIRTY;
          S.NHC[j] = NHC_DIRTY;
          if (S.OCC[vi] & OCC_FLAG) occ_rescan(P, S, vi);
          else S.OCC[vi] = j;
          if (o & OCC_FLAG) occ_rescan(P, S, vj);
          else S.OCC[vj] = i;
        }
      }
    }
  }
  ctl.i = n;
  return true;
}

// ---- MOVE: the movement phase without shared cells, as decidability rounds. MUL: the rounds' MU words lie in LDS (MU32)
template <bool MUL>
__device__ __forceinline__ SecNext sec_move(const PlanArgs& P, const Arrays& S, PlanCtl& s_ctl, uint32_t* s_q,
                                            uint32_t* list, uint32_t* s_wcount, uint32_t& s_need, uint32_t& s_flag,
                                            uint32_t& s_best, uint32_t& s_miss, uint32_t& s_exit, uint32_t& s_abort,
                                            unsigned long long* s_tick, unsigned long long& s_tp, bool kdbg) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x, lane = tid & 63u, wid = tid >> 6, nwaves = bd >> 6;
  const uint32_t n = P.n, W = P.W;
  // ---- movement phase as decidability rounds (see header) -----------------
  if (s_ctl.i == 0) {
    for (uint32_t k = tid; k < n; k += bd) S.DEC[k] = (S.V[k] == S.G[k]) ? DEC_DONE : DEC_OPEN;
    PBAR();
    if (tid == 0) s_ctl.i = 1;  // DEC initialised for this step (survives relaunches)
  }
  // Round passes as per-agent bodies, run either block-wide (k = tid, tid + bd, ...) or, in
  // the tail, by wave 0 alone over a compact list of the still-open agents.
  uint64_t tag = 0;
  uint32_t tag16 = 0;  // MUL: the round's 16-bit tag (1..65535; MU32 is cleared when it wraps to 1)
  auto set_tag = [&](uint32_t r) {
    tag = (uint64_t)r << 32;
    tag16 = (r - 1u) % 65535u + 1u;
  };
  // pass 1: target cell of an open agent; MU[c] = lowest open agent targeting c, as a
  // round-tagged max of ~k (no reset pass: entries of older rounds are stale)
  auto pass1 = [&](uint32_t k) -> bool {
    if (S.DEC[k] != DEC_OPEN) return false;
    const int code = lookup_code(P, S, k);
    if (code < 0) {
      if (code == -2) atomicOr(&P.ctl->err, ERR_NO_TABLE);
      else enqueue_pair(P, S.V[k], S.G[k], S.GT[k], s_q);
      s_miss = 1;
      S.SUCC[k] = NO_CELL;
      return true;
    }
    const uint32_t u = step_cell(S.V[k], (uint32_t)code, W);
    S.SUCC[k] = u;
    if constexpr (MUL) atomicMax(&S.MU32[u], (tag16 << 16) | (0xFFFFu - k));
    else atomicMax(reinterpret_cast<unsigned long long*>(&S.MU[u]), (unsigned long long)(tag | (uint32_t)~k));
    return true;
  };
  auto mu_of = [&](uint32_t c) -> uint32_t {  // lowest open agent targeting c this round
    if constexpr (MUL) {
      const uint32_t x = S.MU32[c];
      return (x >> 16) == tag16 ? 0xFFFFu - (x & 0xFFFFu) : NO_AGENT;
    } else {
      const uint64_t x = S.MU[c];
      return (x >> 32) == (tag >> 32) ? ~(uint32_t)x : NO_AGENT;
    }
  };
  // pass 2: tentatively decide an open agent whose turn can be replayed from the round-start
  // state. What k reads at its turn is OCC[u] (u = its target), the occupant j's cell, goal
  // and next hop, and its own cell; an undecided agent a < k changes one of them only by
  // targeting u (MU[u] != k), by being the occupant (j < k still open) or by targeting k's
  // cell (MU[v] < k). That alone is not enough: an open agent k whose open occupant b < k is
  // its mutual-swap partner is carried to b's cell before its turn and then targets a cell
  // nobody can name yet, so no agent above the lowest such k (s_best) may commit this
  // round. The same pass finds it.
  auto pass2 = [&](uint32_t k) {
    if (S.DEC[k] != DEC_OPEN) return;
    const uint32_t u = S.SUCC[k], v = S.V[k];
    const uint32_t o = S.OCC[u];
    if (o != OCC_NONE) {
      const uint32_t b = o & OCC_IDX;
      if (b < k && S.DEC[b] != DEC_DONE && S.SUCC[b] == v) {
        atomicMin(&s_best, k);
        return;
      }
    }
    if (mu_of(u) != k) return;
    if (mu_of(v) < k) return;
    uint8_t act;
    if (o == OCC_NONE) {
      act = DEC_MOVE;  // rule 2
    } else {
      const uint32_t j = o & OCC_IDX;
      if (j == k) {
        act = DEC_STAY;
      } else {
        if (j < k && S.DEC[j] != DEC_DONE) return;  // occupant still open below k
        if (S.V[j] == S.G[j]) {
          act = DEC_STAY;
        } else {
          const int cj = lookup_code(P, S, j);
          if (cj < 0) {
            if (cj == -2) atomicOr(&P.ctl->err, ERR_NO_TABLE);
            else enqueue_pair(P, S.V[j], S.G[j], S.GT[j], s_q);
            s_miss = 1;
            return;
          }
          act = step_cell(S.V[j], (uint32_t)cj, W) == v ? DEC_SWAP : DEC_STAY;  // :273
        }
      }
    }
    S.DEC[k] = act;
  };
  // pass 3: commit below s_best (disjoint cells by construction); undo the rest
  auto pass3 = [&](uint32_t k, uint32_t spmin) {
    const uint8_t d = S.DEC[k];
    if (d < DEC_STAY) return;
    if (k >= spmin) {
      S.DEC[k] = DEC_OPEN;
      return;
    }
    S.DEC[k] = DEC_DONE;
    if (d == DEC_STAY) return;
    const uint32_t u = S.SUCC[k], v = S.V[k];
    DTAG(k, 8u);
    if (d == DEC_MOVE) {
      S.V[k] = u;
      S.OCC[u] = k;
      S.OCC[v] = OCC_NONE;
      S.NHC[k] = NHC_DIRTY;
    } else {
      const uint32_t j = S.OCC[u] & OCC_IDX;
      DTAG(j, 8u);
      S.V[k] = u;
      S.V[j] = v;
      S.OCC[u] = k;
      S.OCC[v] = j;
      S.NHC[k] = NHC_DIRTY;
      S.NHC[j] = NHC_DIRTY;
    }
  };
  // Within a round DEC only goes OPEN -> {STAY, MOVE, SWAP} (own entry, pass 2) and the
  // commit pass turns those into DONE (or back to OPEN), so "open at round start" reads
  // as DEC != DEC_DONE for every other agent throughout the round.
  bool tail = false;  // block-uniform: the remaining rounds run in wave 0
  for (;;) {
    if (tid == 0) {
      s_miss = 0;
      s_best = NO_AGENT;
      s_ctl.move_rounds += 1;
      if (kdbg) s_tp = wall_clock64();
      if ((s_ctl.move_rounds & 1023u) == 0u && plan_abort(P)) s_abort = 1;
    }
    PBAR();
    if (s_abort) break;
    set_tag(s_ctl.move_rounds);
    if (MUL && tag16 == 1u && s_ctl.move_rounds > 1u) {  // the 16-bit tag wrapped: old entries would match
      for (uint32_t c = tid; c < P.ncell; c += bd) S.MU32[c] = 0u;
      PBAR();
    }
    int open = 0;
    for (uint32_t k = tid; k < n; k += bd) open |= pass1(k) ? 1 : 0;
    // one agent per thread: the count is exact and decides the switch to the wave tail
    const int nopen = n <= bd ? __syncthreads_count(open) : __syncthreads_or(open);
    PLAN_TICK(TK_MOVE_PASS1);
    if (!nopen) break;
    if (s_miss) break;  // exit to K3 below
    if (n <= bd && nopen <= 64) {
      // compact the open agents (index order) into `list` for the wave tail
      const uint64_t bal = __ballot(open != 0);
      if (lane == 0) s_wcount[wid] = (uint32_t)__popcll(bal);
      PBAR();
      if (open) {
        uint32_t off = 0;
        for (uint32_t w = 0; w < wid; ++w) off += s_wcount[w];
        list[off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = tid;
      }
      PBAR();
      tail = true;
      break;
    }
    for (uint32_t k = tid; k < n; k += bd) pass2(k);
    PBAR();
    PLAN_TICK(TK_MOVE_PASS2);
    const uint32_t spmin = s_best;
    for (uint32_t k = tid; k < n; k += bd) pass3(k, spmin);
    PBAR();
    PLAN_TICK(TK_MOVE_PASS3);
    if (s_miss) break;
  }
  if (tail) {
    // Wave tail: <= 64 open agents, one per lane of wave 0. The round that switched has
    // run pass 1; every pass boundary is a wave-level fence (LDS is in order per wave).
    if (wid == 0) {
      uint32_t nl = 0;
      for (uint32_t w = 0; w < nwaves; ++w) nl += s_wcount[w];
      const uint32_t k = lane < nl ? list[lane] : NO_AGENT;
      uint32_t kk = k;
      for (bool first = true;; first = false) {
        if (!first) {
          if (lane == 0) {
            s_miss = 0;
            s_best = NO_AGENT;
            s_ctl.move_rounds += 1;
            if ((s_ctl.move_rounds & 1023u) == 0u && plan_abort(P)) s_abort = 1;
          }
          __threadfence_block();
          if (*(volatile uint32_t*)&s_abort) break;
          __threadfence_block();
          set_tag(*(volatile uint32_t*)&s_ctl.move_rounds);
          if (MUL && tag16 == 1u) {  // wrapped (wave 0 alone here)
            for (uint32_t c = lane; c < P.ncell; c += 64u) S.MU32[c] = 0u;
            __threadfence_block();
          }
          const bool op = kk != NO_AGENT && pass1(kk);
          __threadfence_block();
          if (__ballot(op) == 0ull) break;
          if (*(volatile uint32_t*)&s_miss) break;
        }
        if (kk != NO_AGENT) pass2(kk);
        __threadfence_block();
        const uint32_t spmin = *(volatile uint32_t*)&s_best;
        if (kk != NO_AGENT) pass3(kk, spmin);
        __threadfence_block();
        if (*(volatile uint32_t*)&s_miss) break;
        if (kk != NO_AGENT && S.DEC[kk] != DEC_OPEN) kk = NO_AGENT;  // committed: leaves the tail
      }
    }
    PBAR();
  }
  if (s_abort) return SEC_LOOP;  // watchdog: exit at the top of the section loop, position kept
  if (s_miss) {
    // the missing codes are queued (pass 1 / pass 2) and their agents' codes are dirty
    if (s_q[Q_NEEDED] > 0 && coop_resolve(P, S, s_q, &s_need, &s_flag, s_ctl.section)) return SEC_LOOP;  // replay the open rounds
    exit_need_queries(s_ctl, s_q, s_exit, s_q[Q_NEEDED] > 0 ? PLAN_NEED_QUERIES : PLAN_ERROR);  // none queued: a goal without a table
    PBAR();
    return SEC_LEAVE;
  }
  if (tid == 0) {
    s_ctl.section = SEC_RECORD;
    s_ctl.i = 0;
  }
  PBAR();
  return SEC_LOOP;
}

}  // namespace

}  // namespace tsw
