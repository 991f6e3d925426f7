// tsw_fleet_host.hip — the decentralized tick of the host runtime (tsw_ctx.h): tsw_decide and its decision
// rounds, the fleet-wide nearby lists (K5), a tick's decisions applied (K5b), and the lock-step runs built on
// them (tsw_fleet_run, tsw_fleet_mapd). Host code only.
#include "tsw_ctx.h"
#include "tsw_fleet.h"
#include "tsw_fleet_mapd.h"
#include "tsw_layout.h"
#include "tsw_nearby.h"

extern "C" {

// k_decide's arrays on the device: what tsw_decide uploads and tsw_decide_fleet builds there
struct DecideDev {
  uint32_t n, tot;
  uint32_t *v, *g, *off, *nv, *ng;  // inputs: n, n, n + 1, max(tot, 1), max(tot, 1) words
  uint32_t *act, *cell, *par, *np;  // outputs: n words each
  uint32_t* part;                   // tot + n words (DecideArgs::part)
  uint32_t *q0, *q1, *cnt;          // the rounds' agent lists (n words each) and their 2 counters
};
static int decide_rounds(tsw_ctx* c, const DecideDev& D);

static int decide_impl(tsw_ctx* c, const uint32_t* my_v, const uint32_t* my_g, uint32_t n, const uint32_t* nb_off,
                       const uint32_t* nb_v, const uint32_t* nb_g, uint32_t* act, uint32_t* cell, uint32_t* partner,
                       uint32_t* npart, uint32_t* part) {
  if (!c) return TSW_EINVAL;
  if (n == 0) return TSW_OK;
  if (!my_v || !my_g || !nb_off || !act || !cell || !partner || !npart || !part) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  const uint32_t tot = nb_off[n];
  if (nb_off[0] != 0) RET(TSW_EINVAL, "nb_off[0] must be 0");
  for (uint32_t i = 0; i < n; ++i)
    if (nb_off[i + 1] < nb_off[i]) RET(TSW_EINVAL, "nb_off must be non-decreasing");
  if (tot && (!nb_v || !nb_g)) RET(TSW_EINVAL, "null nearby list");
  // goal tables for every goal a decision can route to: own goals and the nearby agents'
  // (those on free cells — a goal off the map stops the chase, agent.rs:389-393)
  std::vector<uint32_t> goals;
  goals.reserve(n + tot);
  for (uint32_t i = 0; i < n; ++i) {
    if (!cell_id_ok(c, my_v[i]) || !cell_id_ok(c, my_g[i]))
      RET(TSW_EINVAL, "agent cell or goal off-grid or blocked (reference panics at agent.rs:358)");
    goals.push_back(my_g[i]);
  }
  for (uint32_t k = 0; k < tot; ++k)
    if (cell_id_ok(c, nb_g[k]) && cell_id_ok(c, nb_v[k])) goals.push_back(nb_g[k]);
  TRY(ensure_tables(c, goals, true));
  // device copies: inputs, outputs, pending lists (ping-pong)
  const DecideLayout L = decide_layout(n, tot);
  DevBuf<uint32_t> buf;
  HIPCHK(buf.alloc(L.total));
  uint32_t* const d = buf.p;
  DecideDev D{};
  D.n = n;
  D.tot = tot;
  D.v = d + L.v;
  D.g = d + L.g;
  D.off = d + L.off;
  D.nv = d + L.nv;
  D.ng = d + L.ng;
  D.act = d + L.act;
  D.cell = d + L.cell;
  D.par = d + L.par;
  D.np = d + L.np;
  D.part = d + L.part;
  D.q0 = d + L.q0;
  D.q1 = d + L.q1;
  D.cnt = d + L.cnt;
  HIPCHK(hipMemcpyAsync(D.v, my_v, n * 4ull, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(D.g, my_g, n * 4ull, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(D.off, nb_off, (n + 1) * 4ull, hipMemcpyHostToDevice, c->s));
  if (tot) {
    HIPCHK(hipMemcpyAsync(D.nv, nb_v, tot * 4ull, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(D.ng, nb_g, tot * 4ull, hipMemcpyHostToDevice, c->s));
  }
  TRY(decide_rounds(c, D));
  HIPCHK(hipMemcpyAsync(act, D.act, n * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(cell, D.cell, n * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(partner, D.par, n * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(npart, D.np, n * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(part, D.part, ((size_t)tot + n) * 4ull, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  resolve_timing(c);
  return TSW_OK;
}

// The decision rounds over device-resident lists, shared by tsw_decide and tsw_decide_fleet: k_decide
// over every agent, K3 over the pairs it queued, k_decide again over the agents it parked, until none
// is pending. The outputs stay on the device; the stream is idle when this returns TSW_OK.
static int decide_rounds(tsw_ctx* c, const DecideDev& D) {
  const uint32_t n = D.n, tot = D.tot;
  std::vector<uint32_t> idx(n);
  for (uint32_t i = 0; i < n; ++i) idx[i] = i;
  HIPCHK(hipMemcpyAsync(D.q0, idx.data(), n * 4ull, hipMemcpyHostToDevice, c->s));
  TRY(ensure_queue(c, std::max<size_t>(2 * ((size_t)n + tot), 1024)));
  DecideArgs A{};
  A.W = c->G.W;
  A.ncell = c->G.ncell;
  A.my_v = D.v;
  A.my_g = D.g;
  A.nb_off = D.off;
  A.nb_v = D.nv;
  A.nb_g = D.ng;
  A.nbmask = c->d_nbmask;
  A.goal_tab = c->d_goal_tab;
  A.nh = c->d_nh;
  A.nstride = c->tstride;
  A.act = D.act;
  A.cell = D.cell;
  A.partner = D.par;
  A.npart = D.np;
  A.part = D.part;
  A.Q = c->d_Q;
  A.qcap = (uint32_t)c->d_Q.cap;
  A.err = &c->d_stat->err;
  uint32_t nq = n;
  uint32_t* qin = D.q0;
  uint32_t* qout = D.q1;
  for (int round = 0; nq > 0; ++round) {
    if (round > 1 + 2 * (int)std::min<uint64_t>((uint64_t)tot + n, 1u << 20)) RET(TSW_EINVAL, "decision made no progress");
    A.qidx = qin;
    A.nq = nq;
    A.pending_out = qout;
    A.qcount = D.cnt;
    A.npending = D.cnt + 1;
    HIPCHK(hipMemsetAsync(D.cnt, 0, 8, c->s));
    HIPCHK(launch_decide(A, c->s));
    uint32_t h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, D.cnt, 8, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    TRY(check_err(c));
    if (h[1] == 0) break;
    if (h[0] == 0 || h[0] > c->d_Q.cap) RET(TSW_EINVAL, "decision stalled on an unresolvable next hop");
    TRY(run_astar(c, c->d_Q, h[0], true, nullptr, nullptr));
    nq = h[1];
    std::swap(qin, qout);
  }
  return TSW_OK;
}

int tsw_decide(tsw_ctx* c, const uint32_t* my_v, const uint32_t* my_g, uint32_t n, const uint32_t* nb_off,
               const uint32_t* nb_v, const uint32_t* nb_g, uint32_t* act, uint32_t* cell, uint32_t* partner,
               uint32_t* npart, uint32_t* part) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  // a failed round may leave queued pairs PENDING: reset them before returning the error
  return reset_pending_after(c, decide_impl(c, my_v, my_g, n, nb_off, nb_v, nb_g, act, cell, partner, npart, part));
}

// ---- K5: fleet-wide nearby lists (tsw_nearby.hip) and the decentralized tick built on them ----------

// pinned host staging (grow-only): one copy each way instead of one pageable copy per array
static int fleet_hgrow(tsw_ctx* c, size_t words) {
  if (c->h_fleet.holds(words)) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  HIPCHK(c->h_fleet.alloc(words));
  return TSW_OK;
}

// The first half of both entry points: v (and g) on the device, the bins, every list's length and the
// offsets (A.off = nb_off, on the device), with the lists' total and the longest list read back.
struct FleetLists {
  NearbyArgs A{};
  uint32_t *v = nullptr, *g = nullptr;  // device copies (g only when given)
  uint32_t* pad = nullptr;              // the spare word of the head's read-back (fleet_lists_count)
  uint32_t total = 0, maxlen = 0;
};
// The buffers of the count pass in d_fleet[0] (sized by the fleet and the grid), with `extra` more words
// behind them (*extra_out: tsw_fleet_run keeps its apply state there, next to the resident v | g).
static int fleet_lists_setup(tsw_ctx* c, uint32_t n, uint32_t radius, FleetLists* S, size_t extra = 0,
                             uint32_t** extra_out = nullptr) {
  const uint32_t ncell = c->G.ncell;
  const FleetListsLayout L = fleet_lists_layout(n, ncell, std::max(nb_scan_blocks(ncell), nb_scan_blocks(n)), extra);
  TRY(grow_synced(c, c->d_fleet[0], L.total));
  TRY(fleet_hgrow(c, 4 * (size_t)n + 4));
  uint32_t* d = c->d_fleet[0];
  NearbyArgs& A = S->A;
  A.total64 = reinterpret_cast<unsigned long long*>(d + L.total64);
  A.maxlen = d + L.maxlen;
  S->pad = d + L.pad;
  A.cell_start = d + L.cell_start;
  S->v = d + L.v;
  S->g = d + L.g;
  A.rank = d + L.rank;
  A.sorted = d + L.sorted;
  A.off = d + L.off;
  A.bsum = d + L.bsum;
  if (extra_out) *extra_out = d + L.extra;
  A.W = c->G.W;
  A.H = c->G.H;
  A.n = n;
  A.radius = std::min(radius, c->G.W + c->G.H);  // farther than any two cells of the grid are apart
  A.v = S->v;
  return TSW_OK;
}

// The count pass over the device-resident S->v, with the lists' total and the longest list read back.
// pad_src (device, may be nullptr) -> *pad: one more word for the host in the pad slot of the same 16-byte
// read-back (tsw_fleet_run: the previous tick's "changed" word, so a tick adds no synchronise for it).
static int fleet_lists_count(tsw_ctx* c, FleetLists* S, const uint32_t* pad_src = nullptr, uint32_t* pad = nullptr) {
  HIPCHK(launch_nearby_count(S->A, c->s));
  if (pad_src) HIPCHK(hipMemcpyAsync(S->pad, pad_src, 4, hipMemcpyDeviceToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->h_fleet, S->A.total64, 16, hipMemcpyDeviceToHost, c->s));  // total64, maxlen, pad
  HIPCHK(hipStreamSynchronize(c->s));
  unsigned long long tot64 = 0;
  std::memcpy(&tot64, c->h_fleet, 8);
  S->maxlen = c->h_fleet[2];
  if (pad) *pad = c->h_fleet[3];
  if (tot64 > 0xFFFFFFFFull) RET(TSW_EOVERFLOW, "the nearby lists hold more than 2^32 - 1 entries");
  S->total = (uint32_t)tot64;
  return TSW_OK;
}

static int nearby_offsets(tsw_ctx* c, const uint32_t* v, const uint32_t* g, uint32_t n, uint32_t radius, FleetLists* S) {
  TRY(fleet_lists_setup(c, n, radius, S));
  // v | g through the staging buffer in one copy (S->g follows S->v on the device); the stream orders
  // the read-back of the count pass behind it, so the same buffer takes the count pass's head words
  std::memcpy(c->h_fleet, v, n * 4ull);
  if (g) std::memcpy(c->h_fleet + n, g, n * 4ull);
  HIPCHK(hipMemcpyAsync(S->v, c->h_fleet, (g ? 2ull : 1ull) * n * 4ull, hipMemcpyHostToDevice, c->s));
  return fleet_lists_count(c, S);
}

int tsw_nearby(tsw_ctx* c, const uint32_t* v, uint32_t n, uint32_t radius, uint32_t* nb_off, uint32_t* nb_idx,
               uint32_t cap, uint32_t* total) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (!nb_off || !total) RET(TSW_EINVAL, "null argument");
  nb_off[0] = 0;
  *total = 0;
  if (n == 0) return TSW_OK;
  if (!v) RET(TSW_EINVAL, "null argument");
  for (uint32_t i = 0; i < n; ++i)
    if (v[i] >= c->G.ncell) RET(TSW_EINVAL, "agent cell off-grid");
  TRY(set_device(c));
  FleetLists S;
  TRY(nearby_offsets(c, v, nullptr, n, radius, &S));
  HIPCHK(hipMemcpyAsync(nb_off, S.A.off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  *total = S.total;
  if (S.total > cap) RET(TSW_EOVERFLOW, "nb_idx is too small for the nearby lists (*total entries)");
  if (S.total == 0) return TSW_OK;
  if (!nb_idx) RET(TSW_EINVAL, "null nb_idx");
  TRY(grow_synced(c, c->d_fleet[1], S.total));
  HIPCHK(launch_nearby_fill(S.A, S.maxlen, c->d_fleet[1], nullptr, nullptr, nullptr, c->s));
  HIPCHK(hipMemcpyAsync(nb_idx, c->d_fleet[1], (size_t)S.total * 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  return TSW_OK;
}

// The device-resident middle of a tick, shared by tsw_decide_fleet and tsw_fleet_run: behind the count
// pass (S), the lists with their cells and goals, the decision rounds, and the translation of list
// indices to agent indices. The decisions stay on the device: D->act | D->cell | D->par | *d_poff (n + 1
// participant offsets) in one block, the participants in *d_pout (S.total + n words; written when
// part_off[n] <= part_cap).
static int fleet_decide_device(tsw_ctx* c, const FleetLists& S, uint32_t part_cap, DecideDev* Dp, uint32_t** d_poff_out,
                               uint32_t** d_pout_out) {
  const uint32_t n = S.A.n;
  const uint32_t tot = S.total;
  const FleetDecideLayout L = fleet_decide_layout(n, tot);
  TRY(grow_synced(c, c->d_fleet[1], L.total));
  uint32_t* const d = c->d_fleet[1];
  uint32_t* d_idx = d + L.idx;
  DecideDev& D = *Dp;
  D.n = n;
  D.tot = tot;
  D.v = S.v;
  D.g = S.g;
  D.off = S.A.off;
  D.nv = d + L.nv;
  D.ng = d + L.ng;
  D.act = d + L.act;
  D.cell = d + L.cell;
  D.par = d + L.par;
  uint32_t* d_poff = d + L.poff;  // n + 1: participant offsets
  D.np = d + L.np;
  D.part = d + L.part;
  D.q0 = d + L.q0;
  D.q1 = d + L.q1;
  D.cnt = d + L.cnt;
  uint32_t* d_pout = d + L.pout;  // tot + n: compacted participants (agent indices)
  // the lists, and in the same pass their cells and goals (nb_v / nb_g, what k_decide reads)
  HIPCHK(launch_nearby_fill(S.A, S.maxlen, d_idx, S.g, D.nv, D.ng, c->s));
  TRY(decide_rounds(c, D));
  // list indices -> agent indices; participants compacted behind the scan of npart (the kernel itself
  // compares part_off[n] with part_cap, so the common tick without a rotation ends in one synchronise)
  HIPCHK(hipMemcpyAsync(d_poff, D.np, n * 4ull, hipMemcpyDeviceToDevice, c->s));
  HIPCHK(launch_exclusive_scan(d_poff, n, S.A.bsum, c->s));
  HIPCHK(launch_fleet_finish(n, D.off, d_idx, D.par, D.np, D.part, d_poff, d_pout, part_cap, c->s));
  *d_poff_out = d_poff;
  *d_pout_out = d_pout;
  return TSW_OK;
}

static int decide_fleet_impl(tsw_ctx* c, const uint32_t* v, const uint32_t* g, uint32_t n, uint32_t radius,
                             uint32_t* act, uint32_t* cell, uint32_t* partner, uint32_t* part_off, uint32_t* part,
                             uint32_t part_cap) {
  std::vector<uint32_t> goals;
  goals.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (!cell_id_ok(c, v[i]) || !cell_id_ok(c, g[i]))
      RET(TSW_EINVAL, "agent cell or goal off-grid or blocked (reference panics at agent.rs:358)");
    goals.push_back(g[i]);
  }
  // every list entry is an agent of the fleet: the goals a decision can route to are the fleet's own
  TRY(ensure_tables(c, goals, true));
  FleetLists S;
  TRY(nearby_offsets(c, v, g, n, radius, &S));
  DecideDev D{};
  uint32_t *d_poff, *d_pout;
  TRY(fleet_decide_device(c, S, part_cap, &D, &d_poff, &d_pout));
  HIPCHK(hipMemcpyAsync(c->h_fleet, D.act, (4 * (size_t)n + 1) * 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  std::memcpy(act, c->h_fleet, n * 4ull);
  std::memcpy(cell, c->h_fleet + n, n * 4ull);
  std::memcpy(partner, c->h_fleet + 2 * (size_t)n, n * 4ull);
  std::memcpy(part_off, c->h_fleet + 3 * (size_t)n, ((size_t)n + 1) * 4);
  const uint32_t ptot = part_off[n];
  if (ptot > part_cap) {
    resolve_timing(c);
    RET(TSW_EOVERFLOW, "part is too small for the rotation participants (part_off[n] entries)");
  }
  if (ptot) {
    if (!part) RET(TSW_EINVAL, "null part");
    HIPCHK(hipMemcpyAsync(part, d_pout, (size_t)ptot * 4, hipMemcpyDeviceToHost, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  resolve_timing(c);
  return TSW_OK;
}

int tsw_decide_fleet(tsw_ctx* c, const uint32_t* v, const uint32_t* g, uint32_t n, uint32_t radius, uint32_t* act,
                     uint32_t* cell, uint32_t* partner, uint32_t* part_off, uint32_t* part, uint32_t part_cap) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (!part_off) RET(TSW_EINVAL, "null argument");
  part_off[0] = 0;
  if (n == 0) return TSW_OK;
  if (!v || !g || !act || !cell || !partner) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  // a failed round may leave queued pairs PENDING: reset them before returning the error
  return reset_pending_after(c, decide_fleet_impl(c, v, g, n, radius, act, cell, partner, part_off, part, part_cap));
}

// ---- K5b: a tick's decisions applied (tsw_fleet.hip), and the lock-step run built on both ------------

// the apply state of n agents at p (L: fleet_apply_layout(n, nb_scan_blocks(n)))
static void fleet_apply_state(FleetApplyArgs* A, uint32_t* p, const FleetApplyLayout& L, uint32_t n) {
  A->n = n;
  A->g0 = p + L.g0;
  A->owner = p + L.owner;
  A->opflag = p + L.opflag;
  A->ops = p + L.ops;
  A->bsum = p + L.bsum;
  A->changed = p + L.changed;
}

int tsw_fleet_apply(tsw_ctx* c, uint32_t* v, uint32_t* g, uint32_t n, const uint32_t* act, const uint32_t* cell,
                    const uint32_t* partner, const uint32_t* part_off, const uint32_t* part) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (n == 0) return TSW_OK;
  if (!v || !g || !act || !cell || !partner || !part_off) RET(TSW_EINVAL, "null argument");
  // everything a kernel would index with, checked before anything is launched
  for (uint32_t i = 0; i < n; ++i)
    if (part_off[i + 1] < part_off[i]) RET(TSW_EINVAL, "part_off must be non-decreasing");
  const uint32_t pbase = part_off[0], ptot = part_off[n] - pbase;
  std::vector<uint32_t> seen(n, 0u);  // seen[a] == i + 1: a is already a participant of rotation i
  for (uint32_t i = 0; i < n; ++i) {
    switch (act[i]) {
      case TSW_ACT_MOVE:
        if (!cell_id_ok(c, cell[i])) RET(TSW_EINVAL, "Move destination off-grid or blocked");
        break;
      case TSW_ACT_GOAL_SWAP:
        if (partner[i] >= n) RET(TSW_EINVAL, "goal-swap partner is not an agent of the fleet");
        break;
      case TSW_ACT_ROTATION: {
        if (part_off[i + 1] - part_off[i] < 2) RET(TSW_EINVAL, "rotation with fewer than 2 participants");
        if (!part) RET(TSW_EINVAL, "null part");
        for (uint32_t m = part_off[i]; m < part_off[i + 1]; ++m) {
          const uint32_t a = part[m];
          if (a >= n) RET(TSW_EINVAL, "rotation participant is not an agent of the fleet");
          if (seen[a] == i + 1) RET(TSW_EINVAL, "rotation lists a participant twice");
          seen[a] = i + 1;
        }
        break;
      }
      case TSW_ACT_WAIT: break;
      default: RET(TSW_EINVAL, "act is not one of the four actions (0 .. 3)");
    }
  }
  TRY(set_device(c));
  // one block up, the same in the staging buffer and on the device (part_off rebased to 0); the apply state
  // behind it on the device
  const FleetApplyInLayout I = fleet_apply_in_layout(n, ptot);
  const FleetApplyLayout L = fleet_apply_layout(n, nb_scan_blocks(n));
  TRY(grow_synced(c, c->d_fleet[1], I.total + L.total));
  TRY(fleet_hgrow(c, I.total));
  uint32_t* h = c->h_fleet;
  std::memcpy(h + I.v, v, n * 4ull);
  std::memcpy(h + I.g, g, n * 4ull);
  std::memcpy(h + I.act, act, n * 4ull);
  std::memcpy(h + I.cell, cell, n * 4ull);
  std::memcpy(h + I.partner, partner, n * 4ull);
  for (uint32_t i = 0; i <= n; ++i) h[I.part_off + i] = part_off[i] - pbase;
  if (ptot) std::memcpy(h + I.part, part + pbase, (size_t)ptot * 4);
  uint32_t* d = c->d_fleet[1];
  FleetApplyArgs A{};
  A.v = d + I.v;
  A.g = d + I.g;
  A.act = d + I.act;
  A.cell = d + I.cell;
  A.partner = d + I.partner;
  A.part_off = d + I.part_off;
  A.part = d + I.part;
  fleet_apply_state(&A, d + I.total, L, n);
  A.stamp = 1;
  HIPCHK(hipMemcpyAsync(d, h, I.total * 4, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemsetAsync(A.changed, 0, 4, c->s));
  HIPCHK(launch_fleet_apply(A, c->s));
  // v | g, and the changed word in the staging buffer's next slot (act's: the inputs are on the device by now)
  HIPCHK(hipMemcpyAsync(h + I.v, A.v, 2ull * n * 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipMemcpyAsync(h + I.act, A.changed, 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  if (h[I.act] == FLEET_STUCK) RET(TSW_EHIP, "internal: the goal-op rounds made no progress");
  std::memcpy(v, h + I.v, n * 4ull);
  std::memcpy(g, h + I.g, n * 4ull);
  return TSW_OK;
}

// The first `cols` of `stride` columns of each of n rows, elements of `elem` bytes, from the device's records to
// the caller's of the same stride, on the stream; the later columns stay as the caller left them.
static int download_columns(tsw_ctx* c, void* host, const void* dev, size_t n, size_t cols, size_t stride, size_t elem) {
  if (cols == stride)
    HIPCHK(hipMemcpyAsync(host, dev, n * stride * elem, hipMemcpyDeviceToHost, c->s));
  else
    HIPCHK(hipMemcpy2DAsync(host, stride * elem, dev, stride * elem, cols * elem, n, hipMemcpyDeviceToHost, c->s));
  return TSW_OK;
}

// v, g, *ticks_done and the records are written from the device state after `done` ticks; rc: the run's
// result so far (a failing tick's code is kept, whatever the copy back does).
static int fleet_run_finish(tsw_ctx* c, int rc, const FleetLists& S, FleetApplyArgs A, uint32_t moves_run, uint32_t done,
                            uint32_t ticks, uint32_t* v, uint32_t* g, uint32_t* v_rec, uint32_t* g_rec,
                            uint32_t* ticks_done) {
  const uint32_t n = S.A.n;
  const size_t stride = (size_t)ticks + 1;
  auto copy_back = [&]() -> int {
    if (moves_run == done) {  // column `done` is the state after the last tick: no moves kernel wrote it
      A.rec_col = done;
      HIPCHK(launch_fleet_record(A, c->s));
    }
    HIPCHK(hipMemcpyAsync(c->h_fleet, S.v, 2ull * n * 4, hipMemcpyDeviceToHost, c->s));
    uint32_t* host_rec[2] = {v_rec, g_rec};
    uint32_t* dev_rec[2] = {A.v_rec, A.g_rec};
    for (int k = 0; k < 2; ++k)  // columns 0 .. done
      if (host_rec[k]) TRY(download_columns(c, host_rec[k], dev_rec[k], n, (size_t)done + 1, stride, 4));
    HIPCHK(hipStreamSynchronize(c->s));
    std::memcpy(v, c->h_fleet, n * 4ull);
    std::memcpy(g, c->h_fleet + n, n * 4ull);
    *ticks_done = done;
    return TSW_OK;
  };
  if (rc == TSW_OK) return copy_back();
  if (rc != TSW_EHIP && done > 0) {  // done == 0: the caller's v and g are that state already
    const std::string msg = c->err;
    (void)copy_back();
    c->err = msg;
  }
  return rc;
}

static int fleet_run_impl(tsw_ctx* c, uint32_t* v, uint32_t* g, uint32_t n, uint32_t radius, uint32_t ticks,
                          uint32_t* v_rec, uint32_t* g_rec, uint32_t* ticks_done) {
  std::vector<uint32_t> goals;
  goals.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (!cell_id_ok(c, v[i]) || !cell_id_ok(c, g[i]))
      RET(TSW_EINVAL, "agent cell or goal off-grid or blocked (reference panics at agent.rs:358)");
    goals.push_back(g[i]);
  }
  // one validation and one ensure_tables for all ticks: swaps permute the goals and rotations copy
  // tick-start goals, so the goal set never grows; moves are next hops, so positions stay on free cells
  TRY(ensure_tables(c, goals, true));
  FleetLists S;
  uint32_t* extra = nullptr;
  const FleetApplyLayout L = fleet_apply_layout(n, nb_scan_blocks(n));
  TRY(fleet_lists_setup(c, n, radius, &S, L.total, &extra));
  FleetApplyArgs A{};
  fleet_apply_state(&A, extra, L, n);
  A.v = S.v;
  A.g = S.g;
  if (v_rec || g_rec) {
    const FleetRunRecLayout R = fleet_run_rec_layout((size_t)n * ((size_t)ticks + 1), v_rec != nullptr, g_rec != nullptr);
    TRY(grow_synced(c, c->d_fleet[2], R.total));
    A.v_rec = v_rec ? c->d_fleet[2] + R.v_rec : nullptr;
    A.g_rec = g_rec ? c->d_fleet[2] + R.g_rec : nullptr;
    A.rec_stride = ticks + 1;
  }
  std::memcpy(c->h_fleet, v, n * 4ull);
  std::memcpy(c->h_fleet + n, g, n * 4ull);
  HIPCHK(hipMemcpyAsync(S.v, c->h_fleet, 2ull * n * 4, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemsetAsync(A.changed, 0, 4, c->s));
  // tick t stamps the changed word with t + 1; tick t + 1's count pass brings the word to the host in
  // its own read-back, so a tick synchronises exactly as often as tsw_decide_fleet does
  uint32_t t = 0, done = 0;
  int rc = TSW_OK;
  bool fixed = false;
  for (; t < ticks; ++t) {
    uint32_t chg = 0;
    done = t;  // a tick that fails leaves the state after t ticks
    if ((rc = fleet_lists_count(c, &S, A.changed, &chg)) != TSW_OK) break;
    if (chg == FLEET_STUCK) {
      c->err = "internal: the goal-op rounds made no progress";
      rc = TSW_EHIP;
      break;
    }
    if (t > 0 && chg != t) {  // tick t - 1 changed nothing: a fixed point, not counted
      fixed = true;
      break;
    }
    DecideDev D{};
    uint32_t *d_poff, *d_pout;
    if ((rc = fleet_decide_device(c, S, 0xFFFFFFFFu, &D, &d_poff, &d_pout)) != TSW_OK) break;
    A.act = D.act;
    A.cell = D.cell;
    A.partner = D.par;
    A.part_off = d_poff;
    A.part = d_pout;
    A.stamp = t + 1;
    A.rec_col = t;
    hipError_t e = launch_fleet_apply(A, c->s);
    if (e != hipSuccess) {
      c->err = std::string("launch_fleet_apply failed: ") + hipGetErrorString(e);
      rc = TSW_EHIP;
      break;
    }
  }
  const uint32_t moves_run = t;  // ticks whose moves kernel ran (each wrote its own record column)
  if (rc == TSW_OK && fixed) done = t - 1;
  if (rc == TSW_OK && !fixed) {  // every tick ran: the last one's word has not been read yet
    done = ticks;
    if (ticks > 0) {
      HIPCHK(hipMemcpyAsync(c->h_fleet, A.changed, 4, hipMemcpyDeviceToHost, c->s));
      HIPCHK(hipStreamSynchronize(c->s));
      if (c->h_fleet[0] == FLEET_STUCK) RET(TSW_EHIP, "internal: the goal-op rounds made no progress");
      if (c->h_fleet[0] != ticks) done = ticks - 1;
    }
  }
  rc = fleet_run_finish(c, rc, S, A, moves_run, done, ticks, v, g, v_rec, g_rec, ticks_done);
  resolve_timing(c);
  return rc;
}

int tsw_fleet_run(tsw_ctx* c, uint32_t* v, uint32_t* g, uint32_t n, uint32_t radius, uint32_t ticks, uint32_t* v_rec,
                  uint32_t* g_rec, uint32_t* ticks_done) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (!ticks_done) RET(TSW_EINVAL, "null argument");
  *ticks_done = 0;
  if (n == 0) return TSW_OK;
  if (!v || !g) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  // a failed round may leave queued pairs PENDING: reset them before returning the error
  return reset_pending_after(c, fleet_run_impl(c, v, g, n, radius, ticks, v_rec, g_rec, ticks_done));
}

// ---- K5c: a MAPD run on the lock-step tick (tsw_fleet_mapd.hip around the K5 / K5b pipeline) ----------

static int fleet_mapd_impl(tsw_ctx* c, const std::vector<uint32_t>& vcell, const std::vector<uint32_t>& pick,
                           const std::vector<uint32_t>& dlv, uint32_t radius, uint32_t max_t, tsw_rec* out,
                           uint32_t* goal_out, uint32_t* task_out, uint32_t* out_T, uint32_t* stalled) {
  const uint32_t n = (uint32_t)vcell.size(), m = (uint32_t)pick.size();
  // one ensure_tables for the whole run: task goals come from pick / dlv, swaps permute the goals and
  // rotations copy tick-start goals, so every goal of the run is a start, a pickup or a delivery
  {
    std::vector<uint32_t> goals;
    goals.reserve(n + 2 * (size_t)m);
    goals.insert(goals.end(), vcell.begin(), vcell.end());
    goals.insert(goals.end(), pick.begin(), pick.end());
    goals.insert(goals.end(), dlv.begin(), dlv.end());
    TRY(ensure_tables(c, goals, true));
  }
  FleetLists S;
  uint32_t* extra = nullptr;
  // behind the count pass: the apply state, and behind that the MAPD state
  const FleetApplyLayout L = fleet_apply_layout(n, nb_scan_blocks(n));
  const FleetMapdLayout ML = fleet_mapd_layout(n, m, MAPD_WORDS, nb_scan_blocks(n));
  TRY(fleet_lists_setup(c, n, radius, &S, L.total + ML.total, &extra));
  TRY(fleet_hgrow(c, 2 * (size_t)n + 2 * (size_t)m + 4));
  FleetApplyArgs A{};
  fleet_apply_state(&A, extra, L, n);
  A.v = S.v;
  A.g = S.g;
  uint32_t* const mapd = extra + L.total;
  FleetMapdArgs M{};
  M.n = n;
  M.m = m;
  M.W = c->G.W;
  M.v = S.v;
  M.g = S.g;
  M.st = mapd + ML.st;
  M.words = mapd + ML.words;
  M.tk = mapd + ML.tk;
  M.flag = mapd + ML.flag;
  M.bsum = mapd + ML.bsum;
  uint32_t* d_pick = mapd + ML.pick;
  M.pick = d_pick;
  M.dlv = mapd + ML.dlv;
  M.tick_changed = A.changed;
  const size_t stride = (size_t)max_t + 1;
  const FleetMapdRecLayout R = fleet_mapd_rec_layout((size_t)n * stride, goal_out != nullptr, task_out != nullptr);
  TRY(grow_synced(c, c->d_fleet[2], R.total));
  uint32_t* const dr = c->d_fleet[2];
  M.rec = reinterpret_cast<unsigned long long*>(dr + R.rec);
  M.g_rec = goal_out ? dr + R.g_rec : nullptr;
  M.t_rec = task_out ? dr + R.t_rec : nullptr;
  M.rec_stride = max_t + 1;
  // v | g (= v: an idle agent's goal is its own cell), and pick | dlv, through the staging buffer
  uint32_t* h = c->h_fleet;
  std::memcpy(h, vcell.data(), n * 4ull);
  std::memcpy(h + n, vcell.data(), n * 4ull);
  HIPCHK(hipMemcpyAsync(S.v, h, 2ull * n * 4, hipMemcpyHostToDevice, c->s));
  if (m) {
    std::memcpy(h + 2 * (size_t)n, pick.data(), m * 4ull);
    std::memcpy(h + 2 * (size_t)n + m, dlv.data(), m * 4ull);
    HIPCHK(hipMemcpyAsync(d_pick, h + 2 * (size_t)n, 2ull * m * 4, hipMemcpyHostToDevice, c->s));
  }
  HIPCHK(hipMemsetAsync(M.st, 0, ((size_t)n + MAPD_WORDS) * 4, c->s));  // IDLE, next = 0, no stamp yet
  HIPCHK(hipMemsetAsync(M.tk, 0xFF, n * 4ull, c->s));                   // MAPD_NO_TASK
  HIPCHK(hipMemsetAsync(A.changed, 0, 4, c->s));
  // Step s writes column s (every step before it was recorded, or the run had ended). Its three facts
  // reach the host as one status word inside step s + 1's count-pass read-back, so a step synchronises
  // exactly as often as a tsw_fleet_run tick does. The count pass reads positions only, which stage 1
  // does not touch: it runs ahead of stage 1, and when the status ends the run nothing of step s + 1
  // has changed the state. Behind step max_t there is no count pass: the word comes in a copy of its own.
  constexpr uint32_t NOT_READ = 0xFFFFFFFFu;
  uint32_t cols = 0;
  bool stall = false;
  int rc = TSW_OK;
  for (uint32_t s = 0;; ++s) {
    uint32_t status = NOT_READ;
    if (s <= max_t) {
      rc = fleet_lists_count(c, &S, M.words + MAPD_STATUS, &status);
    } else {
      if (hipMemcpyAsync(h, M.words + MAPD_STATUS, 4, hipMemcpyDeviceToHost, c->s) == hipSuccess &&
          hipStreamSynchronize(c->s) == hipSuccess) {
        status = h[0];
      } else {
        c->err = "reading the last step's status failed";
        rc = TSW_EHIP;
      }
    }
    // The ending decision of step s - 1. When the read-back itself failed (a HIP error: status stays
    // NOT_READ) step s - 1 cannot be judged and is not counted, although its column exists on the device;
    // TSW_EHIP copies nothing back anyway. Every other failure of step s arrives with the status read.
    if (s > 0 && status != NOT_READ) {
      if (status & MAPD_S_STUCK) {
        c->err = "internal: the goal-op rounds made no progress";
        rc = TSW_EHIP;
        break;
      }
      if (status & MAPD_S_DONE) {
        cols = s;
        rc = TSW_OK;
        break;
      }
      if (!(status & (MAPD_S_TASK | MAPD_S_TICK))) {  // a fixed point: step s - 1 is not recorded
        stall = true;
        rc = TSW_OK;
        break;
      }
      cols = s;
    }
    if (rc != TSW_OK || s > max_t) break;  // a failing step, or the horizon (tswap.rs:167)
    M.stamp = A.stamp = s + 1;
    M.rec_col = s;
    hipError_t e = launch_fleet_mapd_tasks(M, c->s);
    if (e != hipSuccess) {
      c->err = std::string("launch_fleet_mapd_tasks failed: ") + hipGetErrorString(e);
      rc = TSW_EHIP;
      break;
    }
    DecideDev D{};
    uint32_t *d_poff, *d_pout;
    if ((rc = fleet_decide_device(c, S, 0xFFFFFFFFu, &D, &d_poff, &d_pout)) != TSW_OK) break;
    A.act = D.act;
    A.cell = D.cell;
    A.partner = D.par;
    A.part_off = d_poff;
    A.part = d_pout;
    e = launch_fleet_apply(A, c->s);
    if (e == hipSuccess) e = launch_fleet_mapd_record(M, c->s);
    if (e != hipSuccess) {
      c->err = std::string("launch_fleet_apply / launch_fleet_mapd_record failed: ") + hipGetErrorString(e);
      rc = TSW_EHIP;
      break;
    }
  }
  // the records come down once: columns 0 .. cols - 1 of every agent's row, the later ones stay as the
  // caller left them
  auto copy_back = [&]() -> int {
    struct {
      void* host;
      const void* dev;
      size_t elem;
    } recs[3] = {{out, M.rec, 8}, {goal_out, M.g_rec, 4}, {task_out, M.t_rec, 4}};
    for (const auto& r : recs)
      if (r.host) TRY(download_columns(c, r.host, r.dev, n, cols, stride, r.elem));
    HIPCHK(hipStreamSynchronize(c->s));
    return TSW_OK;
  };
  if (rc == TSW_OK) {
    if (cols) rc = copy_back();
    if (rc == TSW_OK) {  // a copy back that fails delivered no complete column: *out_T stays 0
      *out_T = cols;
      if (stalled) *stalled = stall ? 1u : 0u;
    }
  } else if (rc != TSW_EHIP && cols > 0) {  // a failing step keeps its code, whatever the copy back does
    const std::string msg = c->err;
    if (copy_back() == TSW_OK) *out_T = cols;
    c->err = msg;
  }
  resolve_timing(c);
  return rc;
}

int tsw_fleet_mapd(tsw_ctx* c, const tsw_point* starts, uint32_t n, const tsw_task* tasks, uint32_t m, uint32_t radius,
                   uint32_t max_t, tsw_rec* out, uint32_t* goal_out, uint32_t* task_out, uint32_t* out_T,
                   uint32_t* stalled) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (!out_T || (n && (!starts || !out)) || (m && !tasks)) RET(TSW_EINVAL, "null argument");
  *out_T = 0;
  if (stalled) *stalled = 0;
  if (max_t > (1u << 20)) RET(TSW_EINVAL, "max_t too large");
  // every cell a kernel would index with, checked before anything is launched; all m tasks, dispatched
  // or not (the model is this library's own: there is no reference panic site to imitate)
  std::vector<uint32_t> vcell(n), pick(m), dlv(m);
  for (uint32_t i = 0; i < n; ++i)
    if (!cell_ok(c, starts[i].x, starts[i].y, &vcell[i])) RET(TSW_EINVAL, "start position off-grid or blocked");
  for (uint32_t k = 0; k < m; ++k)
    if (!cell_ok(c, tasks[k].pickup.x, tasks[k].pickup.y, &pick[k]) ||
        !cell_ok(c, tasks[k].delivery.x, tasks[k].delivery.y, &dlv[k]))
      RET(TSW_EINVAL, "task pickup or delivery off-grid or blocked");
  if (n == 0) return TSW_OK;
  TRY(set_device(c));
  // a failed round may leave queued pairs PENDING: reset them before returning the error
  return reset_pending_after(
      c, fleet_mapd_impl(c, vcell, pick, dlv, radius, max_t, out, goal_out, task_out, out_T, stalled));
}

}  // extern "C"
