// tsw_plan_queue.h — k_plan's queues: the queue state s_q (QSlot), queueing a pair as needed, urgent or speculative,
// the host A* service's early asks, the refresh of the agents' next-hop codes, and coop mode: publishing to the
// concurrent K3 workers and waiting for them.
#pragma once
#include "tsw_plan_dev.h"

namespace tsw {

namespace {

// ---- k_plan's queue state: the sixteen words of its LDS array s_q, which every helper below that queues,
// publishes or asks the host takes as `s_q`. Zeroed at the launch (Q_SPEC_T: the launch's timestep).
enum QSlot : uint32_t {
  Q_NEEDED = 0,         // needed pairs queued since the launch began: the K3 queue of this launch (reported as qcount at every exit, DONE included)
  Q_SPEC = 1,           // speculative pairs queued (coop mode: their own queue QS)
  Q_PUBS = 2,           // publishes (coop mode)
  Q_PUB_NEEDED = 3,     // last published needed / speculative heads (coop mode)
  Q_PUB_SPEC = 4,
  Q_SPEC_T = 5,         // the timestep speculative entries are queued in (coop mode)
  Q_HOT = 6,            // hot task chains queued this launch (coop mode)
  Q_PUB_HOT = 7,        // ... last published head
  Q_PRED = 8,           // predicted task chains queued this launch (coop mode)
  Q_PUB_PRED = 9,       // ... last published head
  Q_HOST_TICKETS = 10,  // host A* service: request tickets taken this launch
  Q_HOST_LIMIT = 11,    // ... tickets below this fit the ring (claimed by the host + ring size: read at each wait, and by an early ask that reaches it)
  Q_WALK_OWED = 12,     // round 14: the timestep + 1 whose walk-ahead the rules phase owes (0: none)
  Q_WALK_DONE = 13,     // ... walker waves that have finished it
  Q_WALK_ARMED_CLK = 14,  // ... diagnostics: wall clock (low word) where it was armed
  Q_WALK_DONE_CLK = 15,   // ... diagnostics: wall clock where the last walker wave was done (0: no walk in this pass)
  Q_WORDS = 16,
};

__device__ __forceinline__ void put_query(const PlanArgs& P, uint8_t* p, uint32_t qi, uint32_t v, uint32_t g,
                                          int32_t tab) {
  *p = NH_PENDING;  // only once the slot is ours: a pending code is always really queued
  AstarQuery q;
  q.v = v;
  q.goal = g;
  q.tab = tab;
  // coop mode reads no result index: the entry carries its enqueue time (wall clock, low 32 bits)
  q.out = P.coop ? (uint32_t)wall_clock64() : qi;
  P.Q[qi] = q;
}

// A pair a step needs now: queue it if it is unresolved (the planner then exits for a host-side K3
// pass, or — coop mode — waits for the concurrent workers). Needed pairs are at most 2n per exit and
// the speculative ones stay below qcap/2, so the queue (qcap = 4n + 4096) cannot overflow; if it
// ever did, the pair is not marked and the host, seeing qcount > qcap, fails the call. In coop mode
// a pair already queued speculatively is promoted: queued again on the needed queue, which the
// workers serve first (the duplicate resolves to the same code).
// s_q[Q_NEEDED]: needed pairs queued since the launch began, s_q[Q_SPEC]: speculative ones (coop mode).
__device__ __forceinline__ void enqueue_pair(const PlanArgs& P, uint32_t v, uint32_t g, int32_t tab, uint32_t* s_q) {
  uint8_t* p = P.nh + (uint64_t)tab * P.nstride + v;
  const uint8_t c = *p;
  if (c != NH_UNKNOWN && !(P.coop && c == NH_PENDING_S)) return;  // queued (PENDING) or resolved
  const uint32_t qi = atomicAdd(&s_q[Q_NEEDED], 1u);
  if (qi < P.qcap) put_query(P, p, qi, v, g, tab);
}

// A pair wanted soon but not by this step (walk-ahead within urgent_hops, a pickup arrival within
// urgent_hops + 1): the needed queue while it has room to spare, else a speculative prefetch. In coop
// mode the needed queue is linear over the launch (qcap entries) and a needed pair it cannot hold stays
// UNKNOWN, so urgent pairs stop at half of it and the other half stays for the pairs a step waits on
// (ADVICE r5).
__device__ __forceinline__ void prefetch_pair(const PlanArgs& P, uint32_t v, uint32_t g, int32_t tab, uint32_t* s_q);
__device__ __forceinline__ void urgent_pair(const PlanArgs& P, uint32_t v, uint32_t g, int32_t tab, uint32_t* s_q,
                                            uint8_t code) {
  if (*(volatile const uint32_t*)&s_q[Q_NEEDED] < P.qcap / 2u) enqueue_pair(P, v, g, tab, s_q);
  else if (code == NH_UNKNOWN) prefetch_pair(P, v, g, tab, s_q);
}

// speculative queue full (no more prefetches this launch)
__device__ __forceinline__ bool spec_full(const PlanArgs& P, const uint32_t* s_q) {
  return P.coop ? *(volatile const uint32_t*)&s_q[Q_SPEC] >= P.qscap : *(volatile const uint32_t*)&s_q[Q_NEEDED] >= P.qcap / 2u;
}

// A speculative prefetch. Exit mode: the slot is reserved by CAS only while the queue holds fewer
// than qcap/2 pairs, so prefetches never take the room the needed pairs of an exit rely on. Coop
// mode: its own queue (QS), resolved by the workers after every needed pair.
__device__ __forceinline__ void prefetch_pair(const PlanArgs& P, uint32_t v, uint32_t g, int32_t tab, uint32_t* s_q) {
  uint8_t* p = P.nh + (uint64_t)tab * P.nstride + v;
  if (*p != NH_UNKNOWN) return;
  if (P.coop) {
    const uint32_t qi = atomicAdd(&s_q[Q_SPEC], 1u);
    if (qi >= P.qscap) return;
    *p = NH_PENDING_S;
    AstarQuery q;
    q.v = v;
    q.goal = g;
    q.tab = tab;
    q.out = s_q[Q_SPEC_T];  // enqueue timestep: the workers drop entries older than stale_steps
    P.QS[qi] = q;
    return;
  }
  const uint32_t lim = P.qcap / 2u;
  // a relaxed atomic load, not a volatile read (the same one LDS load): where a caller passes s_q through a generic
  // pointer the back end has rejected the volatile form ("Illegal instruction detected", a compare with
  // src_shared_base), so keep it this way
  uint32_t cur = __hip_atomic_load(&s_q[Q_NEEDED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  for (;;) {
    if (cur >= lim) return;
    const uint32_t prev = atomicCAS(&s_q[Q_NEEDED], cur, cur + 1u);
    if (prev == cur) break;
    cur = prev;
  }
  put_query(P, p, cur, v, g, tab);
}

// ---- host A* service, early asks (PlanArgs::hask; round 9) -------------------------------------
// A pair queued as urgent is read one step later; a worker wave needs ~0.85 ms for its A*, the host
// ~35 us. So the pair goes on the host request ring now, by coop_wait's protocol — a ticket from
// s_q[Q_HOST_TICKETS] against the room limit s_q[Q_HOST_LIMIT], one 64-bit system-scope store — and its request word is
// remembered in the agent's slot. Nothing is asked when the slot already holds the pair under a ticket
// inside the ring window (a blocked agent does not re-ask every step) or when the ring has no room.
// The room limit is the host's tail word + ring size; the tail only grows, so a stale limit is a safe
// lower bound and the system-scope load that refreshes it runs only when the tickets have reached it.
__device__ __noinline__ void host_ask_early(const PlanArgs& P, uint32_t* s_q, uint32_t v, uint32_t g,
                                            unsigned long long* slot) {
  uint32_t cur = *(volatile uint32_t*)&s_q[Q_HOST_TICKETS];
  if (host_req_live(*slot, v, g, cur, P.hring)) return;
  uint32_t lim = *(volatile uint32_t*)&s_q[Q_HOST_LIMIT];
  if (cur >= lim) {
    lim = min(__hip_atomic_load(&P.hflags[HF_HOST_TAIL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + P.hring,
              HOST_RING_MAX_TICKETS);
    atomicMax(&s_q[Q_HOST_LIMIT], lim);
  }
  for (;;) {
    if (cur >= lim) return;  // the ring is full: not asked
    const uint32_t prev = atomicCAS(&s_q[Q_HOST_TICKETS], cur, cur + 1u);
    if (prev == cur) break;
    cur = prev;
  }
  const unsigned long long w = host_req_word(cur, v, g);
  __hip_atomic_store(&P.hreq[cur & (P.hring - 1u)], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  *slot = w;
  atomicAdd(&P.cc->host_asked, 1u);
  atomicAdd(&P.cc->early_asked, 1u);
}

// The ticket of an outstanding early ask for agent k's pair (v, g), else ~0.
__device__ __forceinline__ uint32_t host_early_ticket(const PlanArgs& P, const uint32_t* s_q, uint32_t k, uint32_t v,
                                                      uint32_t g) {
  const uint32_t tickets = *(volatile const uint32_t*)&s_q[Q_HOST_TICKETS];
  uint32_t t = 0xFFFFFFFFu;
  if (!host_req_live(P.hask[2u * k], v, g, tickets, P.hring, &t)) host_req_live(P.hask[2u * k + 1u], v, g, tickets, P.hring, &t);
  return t;
}

// refresh_codes found agent k's code unresolved: if an early ask for its pair (v, g) has been answered,
// publish the code as coop_wait does (relaxed agent-scope byte store into the table store) and return
// the code, else NH_UNKNOWN. Never waits: a missing, late or foreign reply is no reply.
__device__ __noinline__ uint8_t host_take_early(const PlanArgs& P, const uint32_t* s_q, uint32_t k, uint32_t v, uint32_t g,
                                                int32_t tab) {
  const uint32_t tickets = *(volatile const uint32_t*)&s_q[Q_HOST_TICKETS];
  for (uint32_t j = 0; j < 2u; ++j) {
    const unsigned long long w = P.hask[2u * k + j];
    uint32_t t;
    if (!host_req_live(w, v, g, tickets, P.hring, &t)) continue;
    const uint32_t r = __hip_atomic_load(&P.hrep[t & (P.hring - 1u)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint8_t code;
    if (!host_reply_match(w, r, v, g, tickets, P.hring, &code)) continue;
    __hip_atomic_store(P.nh + (uint64_t)tab * P.nstride + v, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(&P.cc->host_used, 1u);
    atomicAdd(&P.cc->early_taken, 1u);
    return code;
  }
  return NH_UNKNOWN;
}

// parallel: refresh next-hop codes of agents whose code is dirty; unresolved pairs are
// appended to the launch's K3 queue (s_q counts every pair queued since the launch began,
// speculative prefetches included). Returns how many dirty agents still lack a code
// (block-uniform): the planner must exit for K3 iff that is nonzero.
__device__ uint32_t refresh_codes(const PlanArgs& P, const Arrays& S, uint32_t* s_q, uint32_t* s_need,
                                  uint32_t sec) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  if (tid == 0) *s_need = 0;
  PBAR();
  for (uint32_t k = tid; k < P.n; k += bd) {
    if (S.NHC[k] <= NH_STAY) continue;
    const uint32_t v = S.V[k], g = S.G[k];
    if (v == g) continue;
    const int32_t tab = S.GT[k];
    if (tab < 0) {
      atomicOr(&P.ctl->err, ERR_NO_TABLE);
      continue;
    }
    const uint8_t code = nh_code(P, tab, v);
    // unresolved: the host may have answered an early ask for this pair a step ago (the slots are read
    // only here, so a resolved step pays nothing); the agent then does not count as needing
    const uint8_t hcode = (code > NH_STAY && P.hask) ? host_take_early(P, s_q, k, v, g, tab) : code;
    if (hcode <= NH_STAY) {
      S.NHC[k] = hcode;
    } else {
      if (PLAN_DBG && P.coop && (code == NH_UNKNOWN || code == NH_PENDING_S)) {
        const uint32_t grp = sec == SEC_PRE1 ? 0u : sec == SEC_RULES ? 1u : 2u;
        atomicAdd(&P.cc->dbg_need[2u * grp + (code == NH_PENDING_S ? 1u : 0u)], 1u);
        // PRE1, never queued: assigned a task / picked up in this step's ASSIGN (DEC tag, diagnostics)
        if (sec == SEC_PRE1 && code == NH_UNKNOWN && (S.DEC[k] & 0x40u))
          atomicAdd(&P.cc->dbg_need[(S.DEC[k] & 1u) ? 7u : 6u], 1u);
      }
      enqueue_pair(P, v, g, tab, s_q);  // no-op if already queued (PENDING)
      atomicAdd(s_need, 1u);
    }
  }
  PBAR();
  return *s_need;
}

// ---- coop mode (concurrent K3 workers) ------------------------------------------------------
// Memory: the planner's queue entries and PENDING marks are plain stores published by one release
// store of the queue heads (agent scope: written back past this XCD's L2); workers read entries with
// agent-scope loads and write each code with an agent-scope store, which the planner polls with
// agent-scope loads. A code, once written, never changes, so a stale plain read of the table can
// only see an older state (UNKNOWN / PENDING) — a conservative "unresolved", never a wrong hop.
// (Write-through entries and PENDING marks with relaxed head stores instead were measured slower:
// every write-through drops the line from this XCD's L2, and the planner's next plain loads of
// those table lines missed — movement passes 3x slower.)
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// host watchdog (coop and exit mode): the planner polls this in every loop that can run long
__device__ __forceinline__ bool plan_abort(const PlanArgs& P) {
  return P.hflags && __hip_atomic_load(&P.hflags[HF_ABORT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
}

// thread 0: make every entry queued so far visible to the workers (caller: after a barrier). A publish
// whose heads equal the last published ones is skipped: no entry and no PENDING mark was written since
// (marks are only written with an entry), and the agent-scope release it would cost writes back this
// XCD's L2. s_q[Q_PUB_NEEDED] / s_q[Q_PUB_SPEC] hold the last published heads (0 = the launch's zeroed CoopCtl).
__device__ __forceinline__ void coop_publish(const PlanArgs& P, uint32_t* s_q) {
  const uint32_t hn = min(s_q[Q_NEEDED], P.qcap), hs = min(s_q[Q_SPEC], P.qscap), hh = min(s_q[Q_HOT], P.qhcap);
  const uint32_t hp = min(s_q[Q_PRED], P.qpcap);
  if (hn == s_q[Q_PUB_NEEDED] && hs == s_q[Q_PUB_SPEC] && hh == s_q[Q_PUB_HOT] && hp == s_q[Q_PUB_PRED]) return;
  s_q[Q_PUB_NEEDED] = hn;
  s_q[Q_PUB_SPEC] = hs;
  s_q[Q_PUB_HOT] = hh;
  s_q[Q_PUB_PRED] = hp;
  if (P.QP) __hip_atomic_store(&P.cc->head_p, hp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  if (P.QH) __hip_atomic_store(&P.cc->head_h, hh, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&P.cc->head_s, hs, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&P.cc->head_n, hn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  // wake idle workers, which poll only this word (a plain agent-scope store of a new value)
  s_q[Q_PUBS] += 1u;
  __hip_atomic_store(&P.cc->pub, s_q[Q_PUBS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// thread 0, while the other threads may be queueing speculative pairs: publish the needed queue's head
// only (no needed pair is queued concurrently; the speculative head waits for the next full publish,
// after a barrier, since a reserved speculative slot may not be written yet)
__device__ __forceinline__ void coop_publish_needed(const PlanArgs& P, uint32_t* s_q) {
  const uint32_t hn = min(s_q[Q_NEEDED], P.qcap);
  if (hn == s_q[Q_PUB_NEEDED]) return;
  s_q[Q_PUB_NEEDED] = hn;
  __hip_atomic_store(&P.cc->head_n, hn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  s_q[Q_PUBS] += 1u;
  __hip_atomic_store(&P.cc->pub, s_q[Q_PUBS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr unsigned long long COOP_NO_WORKER_TICKS = 100000ull;    // 1 ms at 100 MHz after the launch: no worker running
constexpr unsigned long long COOP_RETRY_TICKS = 2000000ull;      // 20 ms pending: queue the pair again
constexpr unsigned long long COOP_GIVE_UP_TICKS = 500000000ull;  // 5 s: safety valve
enum : int { COOP_OK = 0, COOP_GIVE_UP = 1, COOP_RETRY = 2 };

// Parallel (block-uniform result): publish, then wait until every agent whose next-hop code is dirty
// has it or is no longer pending (UNKNOWN: not queued — the caller's refresh queues it). Codes read
// here go straight into the agent's NHC. COOP_GIVE_UP: no worker alive, a worker error, or the
// safety limit (the caller exits to the host). COOP_RETRY: a pair stayed pending for 20 ms — more
// than any A* on these grids; the caller queues the still-pending pairs again (a duplicate query
// resolves to the same code), so a lost update can cost a retry but never a stall.
// With the host A* service on (P.hring != 0, PlanArgs::hreq) the pairs waited for are also asked of the
// host, and a wait ends on whichever answer arrives first; nothing here ever waits for the host.
__device__ int coop_wait(const PlanArgs& P, const Arrays& S, uint32_t* s_q, uint32_t* s_flag, uint32_t sec) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  if (tid == 0) {
    coop_publish(P, s_q);
    *s_flag = COOP_OK;
    if (PLAN_DBG) {
      const uint32_t hs = min(s_q[Q_SPEC], P.qscap), cs = ld_agent(&P.cc->claim_s);
      const uint32_t dep = hs > cs ? hs - cs : 0u;
      P.cc->dbg_depth += dep;
      P.cc->dbg_depth_max = max(P.cc->dbg_depth_max, dep);
    }
    if (P.hring)
      s_q[Q_HOST_LIMIT] = min(__hip_atomic_load(&P.hflags[HF_HOST_TAIL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + P.hring,
                    HOST_RING_MAX_TICKETS);
  }
  PBAR();
  const unsigned long long t0 = wall_clock64();
  // host A* service: the pairs this thread is about to spin on — its dirty agents whose code reads
  // pending (queued for the workers) right now — are also asked of the host, when their tickets fit the
  // ring; the loop below then takes whichever answer comes first. A dirty agent whose code is resolved or
  // not queued leaves the loop at its first read and is not asked (asking for every dirty agent kept one
  // host core busy with pairs nobody waited for). hmask: bit j = the thread's j-th dirty agent was asked
  // (the first 32 of them), its ticket is hbase + the number of asked ones before it.
  // A pair with an outstanding early ask (host_ask_early) takes no new ticket — the host runs one A* per
  // pair: emask marks it and the loop below spins on the remembered ticket's reply slot. hearly == 2
  // (diagnostic): nothing is asked or polled here.
  uint32_t hbase = 0, hmask = 0, emask = 0;
  if (P.hring && P.hearly != 2u) {
    uint32_t j = 0;
    for (uint32_t k = tid; k < P.n && j < 32u; k += bd) {
      if (S.NHC[k] <= NH_STAY || S.V[k] == S.G[k] || S.GT[k] < 0) continue;
      const uint8_t* p = P.nh + (uint64_t)S.GT[k] * P.nstride + S.V[k];
      const uint8_t c = (uint8_t)(ld_agent(reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3u)) >>
                                  (8u * (uint32_t)((uintptr_t)p & 3u)));
      if (c == NH_PENDING || c == NH_PENDING_S) {
        if (P.hask && host_early_ticket(P, s_q, k, S.V[k], S.G[k]) != 0xFFFFFFFFu) emask |= 1u << j;
        else hmask |= 1u << j;
      }
      ++j;
    }
    if (hmask) {
      const uint32_t cnt = (uint32_t)__builtin_popcount(hmask);
      uint32_t cur = *(volatile uint32_t*)&s_q[Q_HOST_TICKETS];
      bool got = false;
      while (cur + cnt <= s_q[Q_HOST_LIMIT]) {
        const uint32_t prev = atomicCAS(&s_q[Q_HOST_TICKETS], cur, cur + cnt);
        if (prev == cur) {
          hbase = cur;
          got = true;
          break;
        }
        cur = prev;
      }
      if (!got) hmask = 0;  // the ring is full: not asked
    }
    if (hmask) {
      uint32_t t = hbase;
      j = 0;
      for (uint32_t k = tid; k < P.n && j < 32u; k += bd) {
        if (S.NHC[k] <= NH_STAY || S.V[k] == S.G[k] || S.GT[k] < 0) continue;
        if ((hmask >> j) & 1u) {
          __hip_atomic_store(&P.hreq[t & (P.hring - 1u)], host_req_word(t, S.V[k], S.G[k]), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
          ++t;
        }
        ++j;
      }
      atomicAdd(&P.cc->host_asked, t - hbase);
    }
  }
  int st = COOP_OK;
  uint32_t hj = 0;  // index of the dirty agent at hand among this thread's
  for (uint32_t k = tid; k < P.n && st == COOP_OK; k += bd) {
    if (S.NHC[k] <= NH_STAY) continue;
    const uint32_t v = S.V[k];
    const int32_t tab = S.GT[k];
    const uint32_t gk = S.G[k];
    if (v == gk || tab < 0) continue;
    bool asked = hj < 32u && ((hmask >> hj) & 1u);
    uint32_t tk = hbase + (uint32_t)__builtin_popcount(hmask & ((1u << (hj & 31u)) - 1u));  // its ticket, if asked
    if (hj < 32u && ((emask >> hj) & 1u)) {  // asked early: that ticket (gone from its window meanwhile: not polled)
      tk = host_early_ticket(P, s_q, k, v, gk);
      asked = tk != 0xFFFFFFFFu;
    }
    ++hj;
    const unsigned long long hw = host_req_word(tk, v, gk);
    const uint8_t* p = P.nh + (uint64_t)tab * P.nstride + v;
    const uint32_t* w = reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3u);
    const uint32_t sh = 8u * (uint32_t)((uintptr_t)p & 3u);
    for (uint32_t spin = 0;; ++spin) {
      const uint8_t c = (uint8_t)(ld_agent(w) >> sh);
      if (c <= NH_STAY) {
        S.NHC[k] = c;
        break;
      }
      if (c == NH_UNKNOWN) break;
      if (asked) {
        // the host's reply for this ticket (another seq: an older or no reply): publish the code as a worker does
        const uint32_t r = __hip_atomic_load(&P.hrep[tk & (P.hring - 1u)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        uint8_t hc;
        if (host_reply_match(hw, r, v, gk, *(volatile uint32_t*)&s_q[Q_HOST_TICKETS], P.hring, &hc)) {
          __hip_atomic_store(const_cast<uint8_t*>(p), hc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          S.NHC[k] = hc;
          atomicAdd(&P.cc->host_used, 1u);
          break;
        }
      }
      const unsigned long long dt = wall_clock64() - t0;
      if (dt > COOP_GIVE_UP_TICKS || ld_agent(&P.cc->err) != 0u ||
          (ld_agent(&P.cc->alive) == 0u && wall_clock64() - S.t0 > COOP_NO_WORKER_TICKS) ||
          (P.hflags && __hip_atomic_load(&P.hflags[HF_ABORT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u)) {
        st = COOP_GIVE_UP;
        break;
      }
      if (dt > COOP_RETRY_TICKS) {
        st = COOP_RETRY;
        break;
      }
      if (spin < 64) __builtin_amdgcn_s_sleep(1);
      else __builtin_amdgcn_s_sleep(8);
    }
  }
  if (st != COOP_OK) atomicMax(s_flag, (uint32_t)(st == COOP_GIVE_UP ? 3 : st));
  PBAR();
  const uint32_t f = *s_flag;
  if (tid == 0) {
    const unsigned long long dt = wall_clock64() - t0;
    // diagnostics: PRE1 waits classed by what the step's ASSIGN did (5: assigned a task, 6: only
    // pickup arrivals, 7: neither — walking agents)
    {
      const uint32_t kslot[6] = {0u, 0u, 3u, 5u, 6u, 7u};
      sec = (PLAN_DBG && (sec >> 8)) ? kslot[sec >> 8] : min(sec & 0xFFu, 7u);
    }
    P.cc->waits += 1u;
    P.cc->wait_ticks += dt;
    P.cc->waits_sec[sec] += 1u;
    P.cc->wait_sec[sec] += dt;
  }
  PBAR();
  return f == 3u ? COOP_GIVE_UP : (int)f;
}

// COOP_RETRY: every dirty agent whose pair still reads pending is queued again on the needed queue
__device__ void coop_requeue(const PlanArgs& P, const Arrays& S, uint32_t* s_q) {
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  for (uint32_t k = tid; k < P.n; k += bd) {
    if (S.NHC[k] <= NH_STAY) continue;
    const uint32_t v = S.V[k];
    const int32_t tab = S.GT[k];
    if (v == S.G[k] || tab < 0) continue;
    uint8_t* p = P.nh + (uint64_t)tab * P.nstride + v;
    const uint32_t* w = reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3u);
    const uint8_t c = (uint8_t)(ld_agent(w) >> (8u * (uint32_t)((uintptr_t)p & 3u)));
    if (c != NH_PENDING && c != NH_PENDING_S) continue;
    const uint32_t qi = atomicAdd(&s_q[Q_NEEDED], 1u);
    if (qi < P.qcap) put_query(P, p, qi, v, S.G[k], tab);
  }
  PBAR();
}

// Next hops are missing (refresh_codes returned nonzero and queued them). Coop mode: wait for the
// workers and re-run the refresh until nothing is missing (true: continue in the kernel). Otherwise,
// or if the workers do not answer, false: the caller exits for a host-side K3 pass.
__device__ bool coop_resolve(const PlanArgs& P, const Arrays& S, uint32_t* s_q, uint32_t* s_need, uint32_t* s_flag,
                             uint32_t sec) {
  if (!P.coop) return false;
  for (int it = 0; it < 1024; ++it) {
    const int st = coop_wait(P, S, s_q, s_flag, sec);
    if (st == COOP_GIVE_UP) return false;
    if (st == COOP_RETRY) coop_requeue(P, S, s_q);
    if (refresh_codes(P, S, s_q, s_need, sec & 0xFFu) == 0u) return true;
  }
  return false;
}

// Thread 0 ends the launch at a resume point: the needed pairs queued so far are reported (qcount), the status says
// what the host is to do — PLAN_NEED_QUERIES: run K3 over them and relaunch; PLAN_ERROR where the caller found that
// nothing is queued that a relaunch could wait for — and the section loop leaves at its next head. The caller's
// barrier follows.
// (Its arguments, like every section's, are the shared objects themselves. The helpers in this file take s_q, s_need and
// s_flag as generic pointers and are compiled knowing that every caller passes the same LDS address; that knowledge
// passes through pointer and reference parameters but not through a struct of references, with which hipcc 7's back end
// rejects nextnext_prefetch — the "Illegal instruction detected" of the note at prefetch_pair. DESIGN.md, "The planner
// kernel's sources".)
__device__ __forceinline__ void exit_need_queries(PlanCtl& s_ctl, const uint32_t* s_q, uint32_t& s_exit,
                                                  uint32_t status = PLAN_NEED_QUERIES) {
  if (threadIdx.x == 0) {
    s_ctl.qcount = s_q[Q_NEEDED];
    s_ctl.status = status;
    s_exit = 1;
  }
}

}  // namespace

}  // namespace tsw
