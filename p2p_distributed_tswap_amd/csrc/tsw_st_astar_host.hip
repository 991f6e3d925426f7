// tsw_st_astar_host.hip — the space-time A* with reservations in the host runtime (tsw_ctx.h):
// tsw_astar_reserved around K9 (tsw_st_astar.hip) and the path packing. The host's share: the argument checks,
// the reservation set (built here, tsw_st_astar.h, and uploaded), the cut into batches that fit the free
// memory, and the prefix sum over the path lengths. The call reads the context's grid and nothing else of it:
// the table store, the queues and the stats stay as they were. Host code only.
#include "tsw_ctx.h"
#include "tsw_layout.h"
#include "tsw_place.h"
#include "tsw_st_astar.h"

// the scratch of a call stays below this and below half of the free memory
static constexpr size_t ST_SCRATCH_MAX = (size_t)16 << 30;
static constexpr size_t ST_SEG_WORDS_MAX = (size_t)256 << 20;  // path segments of one batch

extern "C" {

static int st_check(tsw_ctx* c, const uint32_t* start, const uint32_t* goal, const uint32_t* start_time, uint32_t k,
                    const tsw_node_res* node_res, uint32_t n_node, const tsw_edge_res* edge_res, uint32_t n_edge,
                    uint32_t max_time, uint32_t max_nodes, uint32_t* path_off, uint32_t* path, uint32_t path_cap,
                    uint32_t* status, uint32_t* total) {
  NOT_FROM_RESOLVER(c);
  if (max_time > ST_MAX_TIME) RET(TSW_EINVAL, "max_time above 2^20");
  if (max_nodes == 0) RET(TSW_EINVAL, "max_nodes is 0");
  if (k && (!start || !goal || !start_time || !status)) RET(TSW_EINVAL, "null start, goal, start_time or status");
  if (!path_off || !total) RET(TSW_EINVAL, "null path_off or total");
  if ((n_node && !node_res) || (n_edge && !edge_res)) RET(TSW_EINVAL, "null reservations with a count");
  if (path_cap && !path) RET(TSW_EINVAL, "null path with a capacity");
  for (uint32_t i = 0; i < k; ++i) {
    if (!cell_id_ok(c, start[i]) || !cell_id_ok(c, goal[i])) RET(TSW_EINVAL, "start or goal off the grid or blocked");
    if (start_time[i] > ST_MAX_TIME) RET(TSW_EINVAL, "start_time above 2^20");
  }
  return TSW_OK;
}

int tsw_astar_reserved(tsw_ctx* c, const uint32_t* start, const uint32_t* goal, const uint32_t* start_time, uint32_t k,
                       const tsw_node_res* node_res, uint32_t n_node, const tsw_edge_res* edge_res, uint32_t n_edge,
                       uint32_t max_time, uint32_t max_nodes, uint32_t* path_off, uint32_t* path, uint32_t path_cap,
                       uint32_t* status, uint32_t* pops, uint32_t* total) {
  if (!c) return TSW_EINVAL;
  TRY(st_check(c, start, goal, start_time, k, node_res, n_node, edge_res, n_edge, max_time, max_nodes, path_off, path,
               path_cap, status, total));
  std::fill(c->st_last, c->st_last + 5, 0.0);
  if (k == 0) {
    path_off[0] = 0;
    *total = 0;
    return TSW_OK;
  }
  TRY(set_device(c));
  static_assert(sizeof(tsw_node_res) == sizeof(StNode) && sizeof(tsw_edge_res) == sizeof(StEdge), "same layout");
  const uint32_t ncell = c->G.ncell;

  // the reservation set: built on the host, one upload
  const auto t_res = std::chrono::steady_clock::now();
  StResSet R;
  try {
    st_build_reservations(reinterpret_cast<const StNode*>(node_res), n_node, reinterpret_cast<const StEdge*>(edge_res),
                          n_edge, c->G.W, c->G.H, max_time, &R);
  } catch (const std::bad_alloc&) {
    RET(TSW_ENOMEM, "space-time A*: the reservation set does not fit host memory (or holds more than 2^30 keys)");
  }
  if (!R.set.empty()) {
    TRY(scratch_grow(c, c->d_st_res, R.set.size(), "space-time A*", "reservations"));
    HIPCHK(hipMemcpyAsync(c->d_st_res, R.set.data(), R.set.size() * 8, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  c->st_last[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_res).count();

  // the waves of a launch and their tables: as many as the device seats, fewer when the memory says so
  const StAstarCfg cfg = st_astar_config(c->G, c->max_lds, c->num_cu, c->tun.st_heap);
  const uint32_t eff = st_eff_nodes(ncell, max_time, max_nodes);
  const uint64_t vwords = st_vis_slots(eff);
  if (vwords > ST_SLOTS_MAX) RET(TSW_ENOMEM, "space-time A*: a visited table of more than 2^31 slots");
  const uint64_t per_wave = (vwords + eff) * 8u;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const size_t held = (c->d_st_vis.cap + c->d_st_heap.cap + c->d_st_seg.cap / 2u) * 8u;  // ours already: reused or replaced
  const size_t budget = std::min<size_t>((free_b + held) / 2u, ST_SCRATCH_MAX);
  if (per_wave > budget) RET(TSW_ENOMEM, "space-time A*: one query's visited table and heap do not fit the free memory");
  // the tables take three quarters of the budget at most (one wave's always), the path segments the rest
  const uint32_t waves = c->tun.st_waves ? std::min(cfg.waves, c->tun.st_waves) : cfg.waves;
  const uint32_t nslots = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(k, waves), std::max<uint64_t>(budget / 4u * 3u / per_wave, 1u));
  size_t seg_budget = std::min<size_t>((budget - (size_t)nslots * per_wave) / 4u, ST_SEG_WORDS_MAX);
  if (c->tun.st_seg_words) seg_budget = std::min<size_t>(seg_budget, c->tun.st_seg_words);
  TRY(scratch_grow(c, c->d_st_heap, (size_t)nslots * eff, "space-time A*", "overflow heaps"));
  const bool regrown = !c->d_st_vis.holds((size_t)nslots * vwords);
  TRY(scratch_grow(c, c->d_st_vis, (size_t)nslots * vwords, "space-time A*", "visited tables"));
  if (c->st_vis_words == 0) c->st_tag = std::max(c->tun.st_tag0, 1u);  // the context's first call
  if (regrown || c->st_vis_words != vwords) {
    c->st_vis_words = vwords;
    c->st_vis_wiped = 0;
  }

  PassTimer<4> pt(c);  // marks 0-1 around the search, 2-3 around the packing
  std::vector<uint32_t> h, all;  // all: the packed paths; they go to the caller once the total is known to fit
  std::vector<uint64_t> h_seg;
  uint64_t tot = 0;
  const bool want_paths = path_cap > 0;
  int rc = TSW_OK;
  auto run = [&]() -> int {
    for (uint32_t b0 = 0; b0 < k;) {
      // the batch: queries b0 .. b1 - 1, as many as the segments' room and the tags of one launch allow
      const uint64_t kb_max = (uint64_t)nslots * (ST_TAG_MAX - 1u);
      h_seg.assign(1, 0ull);
      uint32_t b1 = b0;
      while (b1 < k && b1 - b0 < kb_max) {
        const uint64_t room = st_path_room(start_time[b1], max_time, eff);
        if (h_seg.back() + room > seg_budget) break;
        h_seg.push_back(h_seg.back() + room);
        ++b1;
      }
      if (b1 == b0) RET(TSW_ENOMEM, "space-time A*: one query's path segment does not fit the free memory");
      const uint32_t kb = b1 - b0;
      const uint32_t iters = (kb + nslots - 1u) / nslots;
      // tags: a wave's j-th query of this launch carries st_tag + j; tags that would pass ST_TAG_MAX start over
      // at 1 after a wipe, and so do tables that were never wiped in this geometry (any tag does for them)
      const bool wrap = (uint64_t)c->st_tag + iters > (uint64_t)ST_TAG_MAX + 1u;
      if (c->st_vis_wiped < nslots || wrap) {
        HIPCHK(hipMemsetAsync(c->d_st_vis, 0, (size_t)nslots * vwords * 8u, c->s));
        c->st_vis_wiped = nslots;
        if (wrap) c->st_tag = 1;
      }
      const StBatchLayout L = st_batch_layout(kb);
      TRY(scratch_grow(c, c->d_st_w, L.total, "space-time A*", "queries and results"));
      TRY(scratch_grow(c, c->d_st_segoff, (size_t)kb + 1u, "space-time A*", "segment offsets"));
      TRY(scratch_grow(c, c->d_st_seg, (size_t)h_seg.back(), "space-time A*", "path segments"));
      uint32_t* const d = c->d_st_w.p;
      h.resize(L.status);  // start | goal | start_time go up together
      std::copy(start + b0, start + b1, h.begin() + L.start);
      std::copy(goal + b0, goal + b1, h.begin() + L.goal);
      std::copy(start_time + b0, start_time + b1, h.begin() + L.start_time);
      HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->s));
      HIPCHK(hipMemcpyAsync(c->d_st_segoff, h_seg.data(), h_seg.size() * 8, hipMemcpyHostToDevice, c->s));
      StAstarArgs A{};
      A.W = c->G.W;
      A.H = c->G.H;
      A.ncell = ncell;
      A.Ww = c->G.Ww;
      A.freebits = c->G.freebits;
      A.k = kb;
      A.start = d + L.start;
      A.goal = d + L.goal;
      A.start_time = d + L.start_time;
      A.res = R.set.empty() ? nullptr : c->d_st_res.p;
      A.res_mask = R.mask;
      A.max_time = max_time;
      A.max_nodes = eff;
      A.nslots = nslots;
      A.wpb = cfg.wpb;
      A.hl = cfg.hl;
      A.fb_lds = cfg.fb_lds;
      A.tag0 = c->st_tag;
      A.vis = c->d_st_vis;
      A.vis_mask = (uint32_t)(vwords - 1u);
      A.gheap = c->d_st_heap;
      A.seg_off = c->d_st_segoff;
      A.seg = c->d_st_seg;
      A.status = d + L.status;
      A.pops = d + L.pops;
      A.len = d + L.len;
      uint32_t* const d_boff = d + L.path_off;
      c->st_tag += iters;
      pt.mark(0);
      HIPCHK(launch_st_astar(A, cfg.lds, c->s));
      pt.mark(1);
      // status | pops | len come back together
      h.resize(L.path_off - L.status);
      HIPCHK(hipMemcpyAsync(h.data(), A.status, h.size() * 4, hipMemcpyDeviceToHost, c->s));
      HIPCHK(hipStreamSynchronize(c->s));
      const uint32_t* const hs = h.data();
      const uint32_t* const hp = hs + (L.pops - L.status);
      const uint32_t* const hl = hs + (L.len - L.status);
      std::vector<uint32_t> boff(kb);
      uint64_t btot = 0;
      for (uint32_t i = 0; i < kb; ++i) {
        if (hs[i] > TSW_SP_CAPACITY) RET(TSW_EHIP, "space-time A*: a came_from chain does not reach its start (internal)");
        status[b0 + i] = hs[i];
        if (pops) pops[b0 + i] = hp[i];
        path_off[b0 + i] = (uint32_t)tot;
        boff[i] = (uint32_t)btot;
        btot += hl[i];
        tot += hl[i];
        if (tot > 0xFFFFFFFFull) RET(TSW_EOVERFLOW, "the paths hold more than 2^32 - 1 entries");
      }
      c->st_last[1] += pt.elapsed(0);
      c->st_last[3] += 1.0;
      if (want_paths && tot <= path_cap && btot > 0) {
        TRY(scratch_grow(c, c->d_st_path, (size_t)btot, "space-time A*", "packed paths"));
        HIPCHK(hipMemcpyAsync(d_boff, boff.data(), (size_t)kb * 4, hipMemcpyHostToDevice, c->s));
        pt.mark(2);
        HIPCHK(launch_st_pack(kb, c->d_st_segoff, c->d_st_seg, d_boff, A.len, c->d_st_path, c->s));
        pt.mark(3);
        all.resize((size_t)tot);
        HIPCHK(hipMemcpyAsync(all.data() + (tot - btot), c->d_st_path, (size_t)btot * 4, hipMemcpyDeviceToHost, c->s));
        HIPCHK(hipStreamSynchronize(c->s));
        c->st_last[2] += pt.elapsed(2);
      }
      b0 = b1;
    }
    return TSW_OK;
  };
  try {
    rc = run();
  } catch (const std::bad_alloc&) {
    c->err = "space-time A*: host memory";
    rc = TSW_ENOMEM;
  }
  c->st_last[4] = nslots;
  if (rc != TSW_OK) return rc;
  path_off[k] = (uint32_t)tot;
  *total = (uint32_t)tot;
  if (tot > path_cap) RET(TSW_EOVERFLOW, "path is too small for the paths (*total entries)");
  if (tot) std::memcpy(path, all.data(), (size_t)tot * 4u);
  return TSW_OK;
}

int tsw_probe_st_astar(const tsw_ctx* c, double* out) {
  if (!c || !out) return TSW_EINVAL;
  std::copy(c->st_last, c->st_last + 5, out);
  return TSW_OK;
}

}  // extern "C"
