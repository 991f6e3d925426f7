// tsw_plan_assign.h — k_plan's ASSIGN section (K4): the state machine and the nearest-pickup assignment, with the
// scan over the listed task chunks.
#pragma once
#include "tsw_plan_walk.h"

namespace tsw {

namespace {

// K4: the block reads the nl chunks of the scan's list (two words an entry: chunk, mask of the batch agents it
// matters to) with one lane per index entry — half a wave per chunk, SCAN_GRP list entries per half-wave at a
// time with their loads in flight together — and merges each agent's minimum of (distance, task index) into
// bestk with one 64-bit LDS atomicMin per wave. Out of line, so that its registers are a call's clobber set
// (below nextnext_prefetch's) and not part of the planner body's allocation.
__device__ __noinline__ void scan_walk(const uint32_t* slist, uint32_t nl, const uint32_t* apos, uint64_t* bestk,
                                       const uint32_t* live, const uint32_t* klt, unsigned long long* dbg_ticks) {
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (uint32_t e0 = 0; e0 < nl; e0 += SCAN_GRP * 2u * nwaves) {  // block-uniform
    uint32_t cm0[SCAN_GRP], xy[SCAN_GRP], tk[SCAN_GRP];
#pragma unroll
    for (uint32_t q = 0; q < SCAN_GRP; ++q) {
      const uint32_t ei = e0 + q * 2u * nwaves + 2u * wid + (lane >> 5);
      cm0[q] = 0u;
      xy[q] = TASK_TAKEN;
      tk[q] = 0xFFFFFFFFu;
      if (ei < nl) {
        const size_t ep = (size_t)slist[2u * ei] * KCH + (lane & 31u);
        cm0[q] = slist[2u * ei + 1u];
        xy[q] = live[ep];
        tk[q] = klt[ep];
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < SCAN_GRP; ++q) {
      uint32_t um = (uint32_t)__builtin_amdgcn_readlane((int)cm0[q], 0) |
                    (uint32_t)__builtin_amdgcn_readlane((int)cm0[q], 32);
      if (dbg_ticks && lane == 0 && um != 0u) atomicAdd(&dbg_ticks[TK_SCAN_WAVES], 1ull);  // diagnostics: waves with an entry
      const uint32_t cm = xy[q] == TASK_TAKEN ? 0u : cm0[q];
      const uint32_t tx = xy[q] & 0xFFFFu, ty = xy[q] >> 16;
      while (um != 0u) {  // wave-uniform: the agents either half's chunk matters to
        const uint32_t b = (uint32_t)__builtin_ctz(um);
        um &= um - 1u;
        const uint32_t pa = apos[b];
        const uint32_t d = ((cm >> b) & 1u) ? __usad(pa & 0xFFFFu, tx, __usad(pa >> 16, ty, 0u)) : 0xFFFFFFFFu;
        const uint32_t dm = __ockl_wfred_min_u32(d);
        if (dm == 0xFFFFFFFFu) continue;
        const uint32_t tm = __ockl_wfred_min_u32(d == dm ? tk[q] : 0xFFFFFFFFu);
        if (lane == 0)
          atomicMin(reinterpret_cast<unsigned long long*>(&bestk[b]), ((unsigned long long)dm << 32) | tm);
      }
    }
  }
}

// ---- ASSIGN: the state machine and the task assignment of one timestep
__device__ __forceinline__ SecNext sec_assign(const PlanArgs& P, const Arrays& S, PlanCtl& s_ctl, uint32_t* s_q,
                                              uint32_t* list, uint32_t* s_ap, uint32_t* s_wcount, uint32_t& s_cnt,
                                              uint32_t& s_exit, uint32_t& s_doit, uint32_t& s_badat, uint32_t& s_bad,
                                              uint32_t& s_nassign, uint32_t& s_npick, uint64_t* s_bestk,
                                              uint32_t* s_apos, uint32_t* s_acct, uint32_t* s_ub, uint32_t& s_cnt2,
                                              uint32_t& s_lcnt, uint32_t& s_more, unsigned long long* s_tick,
                                              unsigned long long& s_tp, unsigned long long& s_tp2, bool kdbg,
                                              uint32_t kab) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x, lane = tid & 63u, wid = tid >> 6, nwaves = bd >> 6;
  const uint32_t n = P.n, W = P.W;
  // ---- K4: state machine + task assignment (tswap.rs:106-139) -------------
  // The reference walks agents in index order: an agent at its goal advances its state (ToPickup ->
  // ToDelivery with g := delivery, :107-118; ToDelivery -> Idle, :119-121), then an Idle agent takes
  // the nearest unused pickup (:123-138). Transitions touch only their own agent, so they run in
  // parallel. The assignments depend on each other (a task taken by an earlier agent is gone): the
  // idle agents are taken in index order in adaptive batches of up to ABATCH. One block-wide pass
  // computes every batch agent's first minimum of (Manhattan distance, task index) over the Morton
  // index, reading only chunks whose box lower bound is within the agent's current bound; wave 0
  // then accepts the minima in agent order up to the first agent whose task an earlier batch agent
  // took (it and the rest re-run in the next batch). An accepted minimum was taken over a superset of
  // the tasks unused at its sequential turn and is still unused, so it is min_by_key's lowest-index
  // first minimum (tswap.rs:125-130). The first
  // agent whose delivery cell is bad (pos2id panics, :112) ends the step there: assignments of
  // agents below it still happen (and may panic first, :136), none above it.
  if (tid == 0) {
    s_nassign = s_npick = s_bad = 0;
    if (kdbg) {
      s_tp = wall_clock64();
      s_tick[TK_ASG_SECTIONS] += 1;  // diagnostics: ASSIGN sections (sub-phase ticks in TK_ASG_*)
    }
  }
  PBAR();
  for (uint32_t base = 0; base < n && !s_bad; base += bd) {
    const uint32_t i = base + tid;
    bool idle = false;
    if (tid == 0) s_badat = NO_AGENT;  // lowest agent of this chunk with a bad delivery cell
    PBAR();
    if (i < n) {
      uint8_t st = P.st[i];
      if (S.V[i] == S.G[i] && st != ST_IDLE) {
        if (st == ST_TO_PICKUP) {
          st = ST_TO_DELIVERY;
          atomicAdd(&s_npick, 1u);
          if (kdbg) S.DEC[i] = 0x41;  // diagnostics tag (MOVE re-initialises DEC)
          DTAG(i, 32u);
          const int32_t tk = P.task[i];
          if (tk >= 0) {
            const uint32_t ng = P.dlv[tk];
            if (ng == CELL_BAD) {  // pos2id[&task.delivery] panics (tswap.rs:112)
              atomicMin(&s_badat, i);
            } else {
              S.G[i] = ng;
              S.GT[i] = P.goal_tab[ng];
              S.NHC[i] = NHC_DIRTY;
              if ((P.predict & 1u) && P.QP) predict_push(P, s_q, ng, i);
            }
          }
        } else {  // ST_TO_DELIVERY
          st = ST_IDLE;
          P.task[i] = -1;
        }
        P.st[i] = st;
      }
      idle = st == ST_IDLE;
    }
    const uint64_t bal = __ballot(idle);
    if (lane == 0) s_wcount[wid] = (uint32_t)__popcll(bal);
    PBAR();
    PLAN_TICK(TK_ASG_TRANSITIONS);
    if (idle) {
      uint32_t off = 0;
      for (uint32_t w = 0; w < wid; ++w) off += s_wcount[w];
      off += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      list[off] = i;
    }
    if (tid == 0) {
      uint32_t c = 0;
      for (uint32_t w = 0; w < nwaves; ++w) c += s_wcount[w];
      s_cnt = c;
    }
    PBAR();
    PLAN_TICK(TK_ASG_COMPACT);
    const uint32_t cnt = s_cnt, bad_at = s_badat;
    // Assignments in batches of up to ABATCH agents (index order): one block-wide pass computes every
    // batch agent's first minimum over the unused tasks at once, then wave 0 accepts them in agent
    // order up to the first agent whose task an earlier agent of the batch took (that agent and the
    // rest re-run in the next batch, against the updated LIVE array). An accepted agent's minimum was
    // taken over a superset of what was unused at its sequential turn and its task is still unused,
    // so it IS the sequential first minimum (min_by_key, tswap.rs:125-130).
    // batch size adapts: it doubles after a batch without a conflict and drops to the accepted count
    // after one (the t = 0 burst of a dense instance conflicts often; a busy step's handful rarely)
    const uint32_t wmax = (kab & 4u) ? 1u : (kab & 16u) ? 8u : ABATCH;  // (A/B, diagnostic build: 4, 16)
    uint32_t bcur = wmax;
    // The scan's chunk list: what `list` leaves free behind the step's idle agents (C3: ~12 of its 1,024 words
    // in a busy step, so ~500 entries), else the SCAN_CAP entries of s_ap (a t = 0 burst fills `list`).
    // (A/B 32: 4 entries, so that small instances take several rounds over the list too.)
    const bool ltail = !(kab & 32u) && (LIST_CAP - cnt) / 2u > SCAN_CAP;  // block-uniform
    uint32_t* const slist = ltail ? list + cnt : s_ap;
    const uint32_t lcap = (kab & 32u) ? 4u : ltail ? (LIST_CAP - cnt) / 2u : SCAN_CAP;
    auto box_lb = [](uint32_t pa, uint32_t lo, uint32_t hi) -> uint32_t {  // distance from pa to a box
      const uint32_t px = pa & 0xFFFFu, py = pa >> 16;
      const uint32_t x0 = lo & 0xFFFFu, y0 = lo >> 16, x1 = hi & 0xFFFFu, y1 = hi >> 16;
      const uint32_t dx = px < x0 ? x0 - px : (px > x1 ? px - x1 : 0u);
      const uint32_t dy = py < y0 ? y0 - py : (py > y1 ? py - y1 : 0u);
      return dx + dy;
    };
    // Index words. A thread's first KPT chunks (every chunk while kchunks <= KPT * block) stay in
    // registers for the whole step: the boxes are static, and the counts change only through this
    // block's own atomicSub in a batch's update, after whose barrier they are read again (the load is
    // in flight while the next batch is set up). Any further chunks are re-read where they are used.
    const uint32_t nch = P.kchunks;
    uint32_t kc[KPT];
    uint2 kb[KPT];
#pragma unroll
    for (uint32_t s = 0; s < KPT; ++s) {
      const uint32_t c = tid + s * bd;
      kc[s] = (cnt != 0u && c < nch) ? P.kcnt[c] : 0u;
      kb[s] = (cnt != 0u && c < nch) ? P.kbox[c] : make_uint2(0u, 0u);
    }
    for (uint32_t kk = 0; kk < cnt && !s_bad;) {
      const uint32_t B = min(bcur, cnt - kk);
      if (tid < ABATCH) {
        uint32_t ap = 0u;
        if (tid < B) {
          const uint32_t v = S.V[list[kk + tid]];
          ap = (v % W) | ((v / W) << 16);
        }
        s_apos[tid] = ap;
        s_bestk[tid] = ~0ull;
        s_ub[tid] = 0xFFFFFFFFu;
      }
      if (tid == 0) s_lcnt = s_more = 0u;
      PBAR();
      if (kdbg && tid == 0) {
        s_tp2 = wall_clock64();
        SCAN_COUNT(B == 1u ? TK_SCAN_B_ONE : B <= 4u ? TK_SCAN_B_LE4 : B <= 8u ? TK_SCAN_B_LE8 : TK_SCAN_B_MORE, 1);
      }
      // Spatially pruned scan. The host orders the tasks along a Morton curve of their pickup points and
      // cuts that order into chunks of KCH entries with a bounding box each (static) and a count of
      // untaken entries (KCNT). Phase A: a chunk with an untaken entry holds one within
      // lb + diam of an agent (lb: distance to its box), so U_b = min over such chunks of lb + diam
      // bounds agent b's minimum from above. Phase B: only chunks with lb <= U_b can hold a task at
      // the minimum distance (ties included). The threads that own such a chunk append (chunk, mask
      // of the batch agents it matters to) to a list in LDS, and the block then reads the listed
      // chunks with one lane per entry: half a wave per chunk, LIVE and KLT loaded coalesced, each
      // lane's entry compared as (distance, task index) for the agents of its chunk's mask, a wave
      // minimum per agent and one 64-bit LDS atomicMin per wave and agent. The key alone orders the
      // result, so neither the list order nor the arrival order of the atomics matters.
      // Phase A, four batch agents at a time (entries of s_apos past B are zero and never stored)
      for (uint32_t b0 = 0; b0 < B; b0 += 4u) {  // block-uniform
        uint32_t u[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        const uint32_t pa[4] = {s_apos[b0], s_apos[b0 + 1u], s_apos[b0 + 2u], s_apos[b0 + 3u]};
        auto ub_chunk = [&](uint32_t ccnt, uint2 bx) {
          if (ccnt == 0u) return;
          const uint32_t diam = ((bx.y & 0xFFFFu) - (bx.x & 0xFFFFu)) + ((bx.y >> 16) - (bx.x >> 16));
#pragma unroll
          for (uint32_t j = 0; j < 4u; ++j) u[j] = min(u[j], box_lb(pa[j], bx.x, bx.y) + diam);
        };
#pragma unroll
        for (uint32_t s = 0; s < KPT; ++s) ub_chunk(kc[s], kb[s]);
        for (uint32_t c = tid + KPT * bd; c < nch; c += bd) ub_chunk(P.kcnt[c], P.kbox[c]);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
          const uint32_t wm = __ockl_wfred_min_u32(u[j]);
          if (lane == 0 && b0 + j < B) atomicMin(&s_ub[b0 + j], wm);
        }
      }
      PBAR();
      SCAN_TICK(TK_SCAN_BOUND);
      // Phase B. (sl, sc): this thread's next chunk to offer, sm: the batch agents it matters to
      uint32_t sl = 0, sc = tid, sm = 0;
      auto seek = [&]() {  // the thread's next chunk, from (sl, sc) on, within some batch agent's bound
        for (sm = 0u; sc < nch; ++sl, sc += bd) {
          uint32_t ccnt = 0;
          uint2 bx = make_uint2(0u, 0u);
          if (sl < KPT) {
#pragma unroll
            for (uint32_t s = 0; s < KPT; ++s)
              if (s == sl) {
                ccnt = kc[s];
                bx = kb[s];
              }
          } else {
            ccnt = P.kcnt[sc];
            if (ccnt != 0u) bx = P.kbox[sc];
          }
          if (ccnt == 0u) continue;
          for (uint32_t b0 = 0; b0 < B; b0 += 4u) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
              if (box_lb(s_apos[b0 + j], bx.x, bx.y) <= s_ub[b0 + j]) sm |= 1u << (b0 + j);
          }
          sm &= B >= 32u ? 0xFFFFFFFFu : (1u << B) - 1u;
          if (sm != 0u) {
            if (kdbg) {
              SCAN_COUNT(TK_SCAN_PAIRS, __popc(sm));
              SCAN_COUNT(TK_SCAN_CHUNKS, 1);
            }
            return;
          }
        }
      };
      seek();
      for (;;) {
        // append: a wave reserves a run of list entries for its lanes that hold a chunk; what does
        // not fit stays with its thread for the next round over the list (s_more)
        for (;;) {  // wave-uniform
          const uint64_t hb = __ballot(sm != 0u);
          if (hb == 0ull) break;
          uint32_t lb0 = 0;
          if (lane == 0) lb0 = atomicAdd(&s_lcnt, (uint32_t)__popcll(hb));
          lb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lb0);
          if (lb0 >= lcap) {
            if (lane == 0) s_more = 1u;
            break;
          }
          const uint32_t off = lb0 + lane_rank(hb);
          if (sm != 0u && off < lcap) {
            slist[2u * off] = sc;
            slist[2u * off + 1u] = sm;
            ++sl;
            sc += bd;
            seek();
          }
        }
        PBAR();
        const uint32_t nl = min(s_lcnt, lcap), more = s_more;  // written before the barrier above
        if (kdbg && tid == 0) SCAN_COUNT(TK_SCAN_ROUNDS, 1);
        scan_walk(slist, nl, s_apos, s_bestk, P.live, P.klt, (kdbg && P.sec_ticks) ? P.sec_ticks : nullptr);
        if (more == 0u) break;  // block-uniform
        PBAR();  // every thread has read s_lcnt / s_more and its list entries
        if (tid == 0) s_lcnt = s_more = 0u;
        PBAR();
      }
      SCAN_TICK(TK_SCAN_ENTRIES);
      PBAR();
      SCAN_TICK(TK_SCAN_REDUCE);
      PLAN_TICK(TK_ASG_SCAN);
      // Accept in agent order up to the first agent that must stop (past the first bad delivery, out
      // of tasks) or whose task an earlier batch agent took (it and the rest re-run in the next
      // batch): one lane of wave 0 per batch agent. Every agent below that first one is accepted, so
      // "an earlier accepted agent took my task" is "an earlier batch agent's minimum is my task".
      if (wid == 0) {
        const bool in = lane < B;
        const uint64_t key = in ? s_bestk[lane] : ~0ull;
        const uint32_t t = (uint32_t)(key & 0xFFFFFFFFu), un0 = s_ctl.unused;
        const bool halt = in && (list[kk + lane] > bad_at || lane >= un0 || key == ~0ull);
        bool dup = false;
        for (uint32_t e = 0; e + 1u < B; ++e) {  // wave-uniform
          const uint32_t te = (uint32_t)__builtin_amdgcn_readlane((int)t, (int)e);
          dup |= e < lane && te == t;
        }
        const uint64_t hm = __ballot(halt), fm = __ballot(in && (halt || dup));
        const uint32_t acc = fm != 0ull ? (uint32_t)__builtin_ctzll(fm) : B;
        if (lane < acc) s_acct[lane] = t;
        if (lane == 0) {
          s_ctl.unused = un0 - acc;
          s_cnt2 = acc;
          s_doit = (acc < B && ((hm >> acc) & 1ull)) ? 1u : 0u;  // this step assigns no more
          s_nassign += acc;
          if (kdbg) {
            s_tick[TK_ASG_BATCHES] += 1;    // batches
            s_tick[TK_ASG_ACCEPTED] += acc;  // agents accepted
          }
        }
      }
      PBAR();
      PLAN_TICK(TK_ASG_ACCEPT);
      const uint32_t acc = s_cnt2;
      if (tid < acc) {  // the accepted agents' updates in parallel (tswap.rs:132-136)
        const uint32_t ai = list[kk + tid], t = s_acct[tid];
        const uint32_t pos = P.kpos[t];  // the task's entry in the Morton order
        P.live[pos] = TASK_TAKEN;
        atomicSub(&P.kcnt[pos / KCH], 1u);
        P.task[ai] = (int32_t)t;
        P.st[ai] = ST_TO_PICKUP;
        if (P.pred) {  // diagnostics: was this the task last predicted for the agent?
          atomicAdd(&P.cc->pred_asg, 1u);
          const uint32_t pt = ld_agent(&P.pred[ai]);
          if (pt == t) atomicAdd(&P.cc->pred_hit, 1u);
          else if (pt == 0xFFFFFFFFu) atomicAdd(&P.cc->pred_none, 1u);
          __hip_atomic_store(&P.pred[ai], 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (kdbg) S.DEC[ai] = 0x40;
        DTAG(ai, 16u);
        const uint32_t ng = P.pick[t];
        if (ng == CELL_BAD) {  // pos2id[&task.pickup] panics (tswap.rs:136)
          atomicOr(&P.ctl->err, ERR_BAD_PICKUP);
          s_bad = 1;
        } else {
          S.G[ai] = ng;
          S.GT[ai] = P.goal_tab[ng];
          S.NHC[ai] = NHC_DIRTY;
          // the task's pickup -> delivery path goes to the workers now (hot chain), ahead of the
          // index-ordered walk of every task's chain: this one is about to be carried
          const uint32_t dc = P.dlv[t];
          if (P.QH && dc != CELL_BAD && dc != ng) {
            const int32_t dtab = P.goal_tab[dc];
            const uint32_t qi = atomicAdd(&s_q[Q_HOT], 1u);
            if (dtab >= 0 && qi < P.qhcap) {
              AstarQuery q;
              q.v = ng;
              q.goal = dc;
              q.tab = dtab;
              q.out = 0u;
              P.QH[qi] = q;
            } else if (dtab < 0 && qi < P.qhcap) {
              AstarQuery q;  // keep the slot well-formed: a chain without a table is skipped
              q.v = ng;
              q.goal = dc;
              q.tab = -1;
              q.out = 0u;
              P.QH[qi] = q;
            }
          }
        }
      }
      PBAR();
      PLAN_TICK(TK_ASG_UPDATE);
      if (s_doit) break;  // block-uniform
#pragma unroll
      for (uint32_t s = 0; s < KPT; ++s)  // the counts the update above lowered
        if (tid + s * bd < nch) kc[s] = P.kcnt[tid + s * bd];
      kk += acc;
      bcur = acc == B ? min(wmax, 2u * bcur) : max(acc, 1u);
    }
    if (bad_at != NO_AGENT && !s_bad) {  // block-uniform
      if (tid == 0) {
        atomicOr(&P.ctl->err, ERR_BAD_DELIVERY);
        s_bad = 1;
      }
      PBAR();
    }
  }
  if (P.t0_delay_ticks && s_ctl.t == 0u && tid == 0) {  // diagnostic A/B: workers get a head start
    const unsigned long long w0 = wall_clock64();
    while (wall_clock64() - w0 < P.t0_delay_ticks) __builtin_amdgcn_s_sleep(64);
  }
  if (s_bad) {  // block-uniform: stop with the error bit set, no record for this timestep
    if (tid == 0) {
      s_ctl.status = PLAN_ERROR;
      s_exit = 1;
    }
    PBAR();
    return SEC_LEAVE;
  }
  if (tid == 0) {
    s_ctl.section = SEC_PRE1;
    s_ctl.i = 0;
  }
  PBAR();
  return SEC_LOOP;
}

}  // namespace

}  // namespace tsw
