// tsw_layout.h — where the arrays of the host runtime's scratch blocks lie. An entry point of tsw_fleet_host.hip,
// tsw_audit_host.hip, tsw_timeline_host.hip or tsw_st_astar_host.hip puts many arrays into one block of 32-bit
// words; the function here that lays the block out is the one place that says which arrays, in which order and of
// which size, and the block's size is what the same walk adds up to. A call site asks for its layout, grows the
// buffer to .total and points at base + L.part. Offsets, not pointers: there is no arithmetic on a buffer that is
// not there yet, and one layout serves a pinned host image and its device block alike.
// Plain C++17 and no HIP: the counts that kernel headers own (the scan's block counts, MAPD_WORDS, AUD_N*, TL_N*) come
// in as arguments, so a host compiler builds this header alone (tests/host/layout_main.cpp pins every total).
#pragma once

#include <cstddef>

namespace tsw {

// A walk over a block of 32-bit words. A part that is addressed as 64-bit words or as uint2 is taken with take64:
// it starts on an even word, so it is 8-byte aligned in an allocation that is.
struct Carve {
  size_t at = 0;
  size_t take(size_t words) {
    const size_t o = at;
    at += words;
    return o;
  }
  size_t take64(size_t qwords) {
    at += at & 1u;
    return take(2 * qwords);
  }
  size_t total() const { return at; }
};

// ---- tsw_fleet_host.hip -------------------------------------------------------------------------------------------

// The count pass (d_fleet[0]), sized by the fleet and the grid, with `extra` words of the caller's behind it.
// nbs: max(nb_scan_blocks(ncell), nb_scan_blocks(n)).
struct FleetListsLayout {
  size_t total64, maxlen, pad, cell_start, v, g, rank, sorted, off, bsum, extra, total;
};
inline FleetListsLayout fleet_lists_layout(size_t n, size_t ncell, size_t nbs, size_t extra) {
  Carve c;
  FleetListsLayout L{};
  // total64 | maxlen | pad come back in one 16-byte copy; launch_nearby_count clears total64 | maxlen | cell_start
  // with one memset
  L.total64 = c.take64(1);
  L.maxlen = c.take(1);
  L.pad = c.take(1);  // one word of the caller's rides along in the read-back (fleet_lists_count)
  L.cell_start = c.take(ncell + 1);
  L.v = c.take(n);  // v | g go up, and come back, in one copy
  L.g = c.take(n);
  L.rank = c.take(n);
  L.sorted = c.take(n);
  L.off = c.take(n + 1);
  L.bsum = c.take(nbs);
  L.extra = c.take(extra);
  L.total = c.total();
  return L;
}

// The apply state of n agents: behind the count pass (its `extra`) or behind tsw_fleet_apply's inputs.
// nbs_n: nb_scan_blocks(n).
struct FleetApplyLayout {
  size_t g0, owner, opflag, ops, bsum, changed, total;
};
inline FleetApplyLayout fleet_apply_layout(size_t n, size_t nbs_n) {
  Carve c;
  FleetApplyLayout L{};
  L.g0 = c.take(n);
  L.owner = c.take(n);
  L.opflag = c.take(n + 1);
  L.ops = c.take(2 * n);
  L.bsum = c.take(nbs_n);
  L.changed = c.take(1);
  L.total = c.total();
  return L;
}

// The MAPD state of n agents and m tasks, behind the apply state. mapd_words: MAPD_WORDS.
struct FleetMapdLayout {
  size_t st, words, tk, flag, bsum, pick, dlv, total;
};
inline FleetMapdLayout fleet_mapd_layout(size_t n, size_t m, size_t mapd_words, size_t nbs_n) {
  Carve c;
  FleetMapdLayout L{};
  L.st = c.take(n);  // st | words are cleared together
  L.words = c.take(mapd_words);
  L.tk = c.take(n);
  L.flag = c.take(n + 1);
  L.bsum = c.take(nbs_n);
  L.pick = c.take(m);  // pick | dlv go up in one copy
  L.dlv = c.take(m);
  L.total = c.total();
  return L;
}

// A tick's decisions (d_fleet[1]): the lists of `tot` entries with their cells and goals, k_decide's outputs and
// round lists, the participants as agent indices. v, g and the list offsets are the count pass's.
struct FleetDecideLayout {
  size_t idx, nv, ng, act, cell, par, poff, np, part, q0, q1, cnt, pout, total;
};
inline FleetDecideLayout fleet_decide_layout(size_t n, size_t tot) {
  const size_t nb = tot ? tot : 1;
  Carve c;
  FleetDecideLayout L{};
  L.idx = c.take(nb);
  L.nv = c.take(nb);
  L.ng = c.take(nb);
  L.act = c.take(n);  // act | cell | par | poff come back in one copy
  L.cell = c.take(n);
  L.par = c.take(n);
  L.poff = c.take(n + 1);
  L.np = c.take(n);
  L.part = c.take(tot + n);
  L.q0 = c.take(n);
  L.q1 = c.take(n);
  L.cnt = c.take(2);
  L.pout = c.take(tot + n);
  L.total = c.total();
  return L;
}

// tsw_decide's own block: what the caller uploads, k_decide's outputs and round lists.
struct DecideLayout {
  size_t v, g, off, nv, ng, act, cell, par, np, part, q0, q1, cnt, total;
};
inline DecideLayout decide_layout(size_t n, size_t tot) {
  const size_t nb = tot ? tot : 1;
  Carve c;
  DecideLayout L{};
  L.v = c.take(n);
  L.g = c.take(n);
  L.off = c.take(n + 1);
  L.nv = c.take(nb);
  L.ng = c.take(nb);
  L.act = c.take(n);
  L.cell = c.take(n);
  L.par = c.take(n);
  L.np = c.take(n);
  L.part = c.take(tot + n);
  L.q0 = c.take(n);
  L.q1 = c.take(n);
  L.cnt = c.take(2);
  L.total = c.total();
  return L;
}

// tsw_fleet_apply's inputs, once as the pinned image (h_fleet) and once on the device (d_fleet[1], the apply state
// behind them): the whole block goes up in one copy, v | g come back in one.
struct FleetApplyInLayout {
  size_t v, g, act, cell, partner, part_off, part, total;
};
inline FleetApplyInLayout fleet_apply_in_layout(size_t n, size_t ptot) {
  Carve c;
  FleetApplyInLayout L{};
  L.v = c.take(n);
  L.g = c.take(n);
  L.act = c.take(n);
  L.cell = c.take(n);
  L.partner = c.take(n);
  L.part_off = c.take(n + 1);
  L.part = c.take(ptot);
  L.total = c.total();
  return L;
}

// The records of a run (d_fleet[2]), `cells` = agents * columns each; a part the caller does not ask for is empty.
struct FleetRunRecLayout {
  size_t v_rec, g_rec, total;
};
inline FleetRunRecLayout fleet_run_rec_layout(size_t cells, bool want_v, bool want_g) {
  Carve c;
  FleetRunRecLayout L{};
  L.v_rec = c.take(want_v ? cells : 0);
  L.g_rec = c.take(want_g ? cells : 0);
  L.total = c.total();
  return L;
}
struct FleetMapdRecLayout {
  size_t rec, g_rec, t_rec, total;
};
inline FleetMapdRecLayout fleet_mapd_rec_layout(size_t cells, bool want_g, bool want_t) {
  Carve c;
  FleetMapdRecLayout L{};
  L.rec = c.take64(cells);  // tsw_rec (8 bytes) first
  L.g_rec = c.take(want_g ? cells : 0);
  L.t_rec = c.take(want_t ? cells : 0);
  L.total = c.total();
  return L;
}

// ---- tsw_audit_host.hip -------------------------------------------------------------------------------------------

// The audit's outputs (d_aud_out). nkind, ncol, nagent: AUD_NKIND, AUD_NCOL, AUD_NAGENT.
struct AuditOutLayout {
  size_t first, col, agent, total;
  size_t col_words, agent_words;
};
inline AuditOutLayout audit_out_layout(size_t n, size_t T, bool want_agent, size_t nkind, size_t ncol, size_t nagent) {
  Carve c;
  AuditOutLayout L{};
  L.col_words = T * ncol;
  L.agent_words = want_agent ? n * nagent : 0;
  L.first = c.take64(nkind);  // first | col come back in one copy
  L.col = c.take(L.col_words);
  L.agent = c.take(L.agent_words);
  L.total = c.total();
  return L;
}

// ---- tsw_timeline_host.hip ----------------------------------------------------------------------------------------

// Every word array of a timeline call (d_tl_w). q .. starts come from one host image of `live` words (the offset of
// pass B's own part is the image's size); vis, sorted, starts and live are read only under rule NEAREST, and only
// then do starts and live take room. nq, nw, ntask: TL_NQ, TL_NW, TL_NTASK.
struct TimelineLayout {
  size_t q, w, task, colflag, vis, release, sorted, starts, live, total;
};
inline TimelineLayout timeline_layout(size_t n, size_t m, size_t T, bool nearest, size_t nq, size_t nw, size_t ntask) {
  Carve c;
  TimelineLayout L{};
  L.q = c.take64(nq);  // q | w | task come back in one copy
  L.w = c.take(nw);
  L.task = c.take(m * ntask);
  L.colflag = c.take(T);
  L.vis = c.take(T);
  L.release = c.take(m);
  L.sorted = c.take64(m);  // uint2 each: behind an odd m one word is skipped
  L.starts = c.take64(nearest ? n : 0);
  L.live = c.take64(nearest ? m : 0);
  L.total = c.total();
  return L;
}

// ---- tsw_st_astar_host.hip ----------------------------------------------------------------------------------------

// One batch of kb space-time queries (d_st_w).
struct StBatchLayout {
  size_t start, goal, start_time, status, pops, len, path_off, total;
};
inline StBatchLayout st_batch_layout(size_t kb) {
  Carve c;
  StBatchLayout L{};
  L.start = c.take(kb);  // start | goal | start_time go up in one copy
  L.goal = c.take(kb);
  L.start_time = c.take(kb);
  L.status = c.take(kb);  // status | pops | len come back in one copy
  L.pops = c.take(kb);
  L.len = c.take(kb);
  L.path_off = c.take(kb);
  L.total = c.total();
  return L;
}

}  // namespace tsw
