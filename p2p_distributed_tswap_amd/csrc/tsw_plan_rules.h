// tsw_plan_rules.h — the rules phase's block-wide helpers: successors and cycle labels by pointer doubling (rules_init)
// and the incremental relabel after a firing. The RULES section itself stands in k_plan (tsw_plan_kernel.h).
#pragma once
#include "tsw_plan_queue.h"

namespace tsw {

namespace {

// Parallel (whole block): succ of every agent, the rule-4 labels and the rule-3 prefetch.
// The chase of tswap.rs:205-238 started at j = succ(i) returns to i exactly when i lies on
// a cycle (length >= 2) of succ over not-at-goal agents. Pointer doubling: after R rounds
// with 2^R > n, F(k) = succ^(2^R)(k) sits on the cycle k drains into (or the sink n), and
// succ^(2^R) permutes each cycle, so {F(k)} is exactly the set of cycle members.
// pf (phase start, wide prefetch): rules_prefetch fused into the first pass — the pair (cell of
// succ(k), goal of k) is the CANDC load itself, and k's own next pair is one more load — saving the
// separate block-wide pass and its repeated table reads.
__device__ void rules_init(const PlanArgs& P, const Arrays& S, uint32_t* pf = nullptr) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x, n = P.n;
  for (uint32_t k = tid; k < n; k += bd) {
    const uint32_t s = succ_of(P, S, k);
    S.SUCC[k] = s;
    S.F1[k] = s == SUCC_TERM ? n : s;
    S.ONC[k] = 0;
    uint8_t cc = NHC_DIRTY;
    const int32_t tab = S.GT[k];
    if (s != SUCC_TERM && s != k && tab >= 0)
      cc = P.nh[(uint64_t)tab * P.nstride + S.V[s]];
    S.CANDC[k] = cc;
    if (pf && tab >= 0 && !spec_full(P, pf)) {  // as rules_prefetch (wide mode: no ONC filter)
      const uint8_t c = S.NHC[k];
      const uint32_t g = S.G[k];
      if (c < NH_STAY && S.V[k] != g) {
        const uint32_t u = step_cell(S.V[k], c, P.W);
        if (u != g && P.nh[(uint64_t)tab * P.nstride + u] == NH_UNKNOWN) prefetch_pair(P, u, g, tab, pf);
      }
      if (cc == NH_UNKNOWN) prefetch_pair(P, S.V[s], g, tab, pf);
    }
  }
  if (tid == 0) {
    S.F1[n] = n;
    S.F2[n] = n;
  }
  PBAR();
  uint32_t* a = S.F1;
  uint32_t* b = S.F2;
  for (uint32_t r = 1; r <= n; r <<= 1) {
    for (uint32_t k = tid; k < n; k += bd) b[k] = a[a[k]];
    PBAR();
    uint32_t* t = a;
    a = b;
    b = t;
  }
  for (uint32_t k = tid; k < n; k += bd) {
    const uint32_t c = a[k];
    if (c != n) S.ONC[c] = 1;
  }
  PBAR();
}

// Incremental rules relabel (thread 0) after a firing changed the goals of the `cnt` agents in
// `lst` (rule-4 rotation: every member of the rotated cycle; rule-3 swap: b and s) and the refresh
// re-looked-up their next hops. In the rules phase nobody moves (OCC is fixed), so only these
// agents' successors changed: SUCC / CANDC are recomputed for them alone, and a cycle that appears
// must pass through one of them while a cycle that disappears contained one (all of a rotated
// cycle's members are in `lst`, and rule 3 only extends the chain of s, which was terminal). So
// each changed agent's cycle label is a walk along SUCC from it: back to itself = on a cycle (label
// the cycle), TERM / a self-loop / an agent on another cycle = not. Walks average ~2 hops on the
// warehouse grids, against a block-wide pointer doubling over every agent. Returns false (caller
// relabels in full) if a walk runs past `limit` hops.
// one changed agent's successor, cleared label and CANDC (independent per agent)
__device__ __forceinline__ void relabel_reset(const PlanArgs& P, const Arrays& S, uint32_t k) {
  const uint32_t s = succ_of(P, S, k);
  S.SUCC[k] = s;
  S.ONC[k] = 0;
  uint8_t cc = NHC_DIRTY;
  if (s != SUCC_TERM && s != k && S.GT[k] >= 0) cc = P.nh[(uint64_t)S.GT[k] * P.nstride + S.V[s]];
  S.CANDC[k] = cc;
}

// the walks of rules_relabel_changed, after relabel_reset of every agent in lst
__device__ bool relabel_walks(const PlanArgs& P, const Arrays& S, const uint32_t* lst, uint32_t cnt, uint32_t limit);

__device__ bool rules_relabel_changed(const PlanArgs& P, const Arrays& S, const uint32_t* lst, uint32_t cnt,
                                      uint32_t limit) {
  for (uint32_t i = 0; i < cnt; ++i) relabel_reset(P, S, lst[i]);
  return relabel_walks(P, S, lst, cnt, limit);
}

__device__ bool relabel_walks(const PlanArgs& P, const Arrays& S, const uint32_t* lst, uint32_t cnt, uint32_t limit) {
  for (uint32_t i = 0; i < cnt; ++i) {
    const uint32_t a = lst[i];
    if (S.ONC[a]) continue;  // labelled by an earlier walk of this loop
    uint32_t x = S.SUCC[a];
    uint32_t steps = 0;
    while (x != SUCC_TERM && x != a) {
      if (S.ONC[x]) {
        // x is labelled: a cycle that still stands (every member of a cycle that broke is in
        // `lst` and was cleared above). It may contain a itself — `lst` accumulates every agent
        // changed since the last labelling, including members of a cycle a rule-3 swap closed
        // and labelled in fire() — so go once around it: meeting a puts a on it, back at x
        // without a means a only drains into it. A walk that does neither means a stale label:
        // relabel in full.
        uint32_t y = S.SUCC[x];
        while (y != x && y != a) {
          if (y == SUCC_TERM || S.SUCC[y] == y || ++steps > limit) return false;
          y = S.SUCC[y];
        }
        x = y;  // == a: on the cycle (labelled below); == x: not
        break;
      }
      const uint32_t nx = S.SUCC[x];
      if (nx == x) break;    // self-loop (stay code): a chain end
      x = nx;
      if (++steps > limit) return false;
    }
    if (x == a) {
      uint32_t y = a;
      do {
        S.ONC[y] = 1;
        y = S.SUCC[y];
      } while (y != a);
    }
  }
  return true;
}

}  // namespace

}  // namespace tsw
