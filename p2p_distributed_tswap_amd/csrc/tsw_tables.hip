// tsw_tables.hip — K1 orchestration and the goal-table store of the host runtime (tsw_ctx.h): the K1
// launch orders and launches (run_bfs; the kernel choice is choose_bfs, tsw_place.h), the store's slots
// with their LRU eviction, the table builds (ensure_tables) and the table entry points of
// include/tswap.h. Host code only.
#include "tsw_ctx.h"

namespace tsw {

int ensure_tmp(tsw_ctx* c, size_t k) {
  if (c->d_tmp_a.holds(k) && c->d_tmp_b.holds(k) && c->d_tmp_c.holds(k)) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  HIPCHK(c->d_tmp_a.grow(k));
  HIPCHK(c->d_tmp_b.grow(k));
  HIPCHK(c->d_tmp_c.grow(k));
  return TSW_OK;
}

// K1 output buffer of a table-build batch: u16 tables of KTMP_BYTES at most (C5's 2 MiB tables: 1,024
// goals per batch), at least one table. Returns the batch size in tables.
constexpr size_t KTMP_BYTES = (size_t)2 << 30;
static int ensure_ktmp(tsw_ctx* c, size_t want, size_t* batch) {
  const size_t per = (size_t)c->tstride * 2u;
  const size_t b = std::max<size_t>(1, std::min(want, KTMP_BYTES / per));
  if (!c->d_ktmp.holds(b * c->tstride)) {
    HIPCHK(hipStreamSynchronize(c->s));
    HIPCHK(c->d_ktmp.alloc(b * c->tstride));
  }
  *batch = b;
  return TSW_OK;
}

// The K1 kernel of this context's grid and knobs (choose_bfs, tsw_place.h): bfs_lpt_order and run_bfs
// both ask here, so the launch order and the launch cannot disagree.
static BfsChoice bfs_choice(const tsw_ctx* c) {
  const BfsGeom g{c->G.W, c->G.H, c->G.ncell, c->nfree, c->npw, c->nbp};
  const BfsKnobs t{c->tun.bfs_mode, c->tun.blk_cap, c->tun.bfs_cap, c->tun.bfs_waves, c->tun.bfs_wls, c->tun.bfs_pair};
  return choose_bfs(g, t, c->max_lds, c->num_cu, bfs_mg_built());
}

static bool mg_selected(const tsw_ctx* c) {
  const BfsChoice ch = bfs_choice(c);
  return ch.kernel == BFS_MG && ch.fits;
}

// k_bfs_mg launch order: goals grouped by (cell parity, Morton order) into groups of <= 16 (one
// parity per group: the kernel advances all of a group's fronts on one checkerboard colour per
// level), groups ordered longest-first by the eccentricity bound of their first goal (LPT, as
// bfs_lpt_order). Fills c->h_mg_grp with the group offsets.
static void bfs_mg_order(tsw_ctx* c, std::vector<uint32_t>& goals, std::vector<uint32_t>& slots) {
  const uint32_t W = c->G.W, H = c->G.H;
  const size_t k = goals.size();
  std::vector<std::pair<uint64_t, uint32_t>> key(k);
  for (size_t i = 0; i < k; ++i) {
    const uint32_t y = goals[i] / W, x = goals[i] - y * W;
    key[i] = {((uint64_t)((x + y) & 1u) << 40) | morton2(x, y), (uint32_t)i};
  }
  std::sort(key.begin(), key.end());
  std::vector<std::pair<uint32_t, uint32_t>> grp;  // (start, end) in key order
  for (size_t i = 0; i < k;) {
    size_t j = i + 1;
    while (j < k && j - i < 16u && (key[j].first >> 40) == (key[i].first >> 40)) ++j;
    grp.push_back({(uint32_t)i, (uint32_t)j});
    i = j;
  }
  auto ecc = [&](uint32_t g) {
    const uint32_t y = g / W, x = g - y * W;
    return std::max(x, W - 1 - x) + std::max(y, H - 1 - y);
  };
  std::stable_sort(grp.begin(), grp.end(), [&](const auto& a, const auto& b) {
    return ecc(goals[key[a.first].second]) > ecc(goals[key[b.first].second]);
  });
  std::vector<uint32_t> g2, s2;
  g2.reserve(k);
  s2.reserve(k);
  c->h_mg_grp.assign(1, 0u);
  for (const auto& gr : grp) {
    for (uint32_t i = gr.first; i < gr.second; ++i) {
      g2.push_back(goals[key[i].second]);
      s2.push_back(slots[key[i].second]);
    }
    c->h_mg_grp.push_back((uint32_t)g2.size());
  }
  goals.swap(g2);
  slots.swap(s2);
}

// K1 launch order: longest BFS first. A goal's level count is its eccentricity; the distance
// to the farthest grid corner bounds it and ranks goals well enough that the work queue's last
// wave of goals is the short ones (LPT scheduling) instead of a few long ones running on an
// otherwise idle chip. Output positions are carried in `slots`. TSW_BFS_ORDER=0 keeps the
// caller's order (A/B). When k_bfs_mg serves the launch, its grouped order instead (bfs_mg_order).
static void bfs_lpt_order(tsw_ctx* c, std::vector<uint32_t>& goals, std::vector<uint32_t>& slots) {
  c->h_mg_grp.clear();
  if (mg_selected(c)) {
    bfs_mg_order(c, goals, slots);
    return;
  }
  if (!c->tun.bfs_order || goals.size() < 2) return;
  const uint32_t W = c->G.W, H = c->G.H, maxe = W + H;
  // counting sort by eccentricity bound, descending, stable: O(k + W + H) on the host
  std::vector<uint32_t> cnt(maxe + 1u, 0u), ecc(goals.size());
  for (size_t i = 0; i < goals.size(); ++i) {
    const uint32_t y = goals[i] / W, x = goals[i] - y * W;
    ecc[i] = maxe - (std::max(x, W - 1 - x) + std::max(y, H - 1 - y));
    ++cnt[ecc[i]];
  }
  uint32_t acc = 0;
  for (uint32_t e = 0; e <= maxe; ++e) {
    const uint32_t t = cnt[e];
    cnt[e] = acc;
    acc += t;
  }
  std::vector<uint32_t> g2(goals.size()), s2(goals.size());
  for (size_t i = 0; i < goals.size(); ++i) {
    const uint32_t j = cnt[ecc[i]]++;
    g2[j] = goals[i];
    s2[j] = slots[i];
  }
  goals.swap(g2);
  slots.swap(s2);
}

// per-wave scratch of the wave-per-goal kernels: `words` u16 anchors + `lwords` u16 list overflow
static int ensure_wave_scratch(tsw_ctx* c, uint64_t want, size_t words, size_t lwords) {
  if (want <= c->wave_scratch && words <= c->scratch_words && lwords <= c->scratch_lwords) return TSW_OK;
  want = std::max(want, c->wave_scratch);
  words = std::max(words, c->scratch_words);
  lwords = std::max(lwords, c->scratch_lwords);
  HIPCHK(hipStreamSynchronize(c->s));
  c->wave_scratch = 0;
  HIPCHK(c->d_anch.reset());  // both old blocks go before the first new one comes
  HIPCHK(c->d_lovf.reset());
  HIPCHK(c->d_anch.alloc((size_t)want * words));
  HIPCHK(c->d_lovf.alloc((size_t)want * lwords));
  c->wave_scratch = want;
  c->scratch_words = words;
  c->scratch_lwords = lwords;
  return TSW_OK;
}

// k_bfs_blk / k_bfs_big per-wave WL scratch (nbp words each) for as many waves as ensure_wave_scratch holds
static int ensure_wlg(tsw_ctx* c) {
  if (c->wlg_waves >= c->wave_scratch) return TSW_OK;
  HIPCHK(hipStreamSynchronize(c->s));
  c->wlg_waves = 0;
  HIPCHK(c->d_wlg.alloc((size_t)c->wave_scratch * c->nbp));
  c->wlg_waves = c->wave_scratch;
  return TSW_OK;
}

static unsigned long long* bfs_prof_buf(tsw_ctx* c) {
  if (!c->tun.bfs_prof) return nullptr;
  if (!c->d_bprof && c->d_bprof.alloc(8) != hipSuccess) return nullptr;
  if (hipMemsetAsync(c->d_bprof, 0, 8 * sizeof(unsigned long long), c->s) != hipSuccess) return nullptr;
  return c->d_bprof;
}

static int bfs_prof_print(tsw_ctx* c, const char* name, uint32_t k) {
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, c->d_bprof, sizeof h, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  fprintf(stderr, "[%s] goals %u  bfs %.0f cyc/goal  decode %.0f cyc/goal  levels %.1f/goal  chunks %.1f/goal"
          "  (mg: wave-cycles list+barrier %.0f, tasks %.0f per goal)\n",
          name, k, (double)h[0] / k, (double)h[1] / k, (double)h[2] / k, (double)h[3] / k, (double)h[4] / k,
          (double)h[5] / k);
  return TSW_OK;
}

// What every K1 rung is given, and fills into its kernel's argument struct the same way.
struct BfsJob {
  const uint32_t* goals;
  const uint32_t* slots;
  uint32_t k;
  uint16_t* dist;
  uint64_t dstride;
  uint8_t* nh;
  uint8_t* govf;
  uint32_t vec16;
  uint32_t* work;
  uint32_t* err;
  uint64_t* prof;  // set by bfs_begin
};

template <class Args>
static void bfs_fill(Args& A, const BfsJob& J) {  // what all four argument structs hold
  A.goals = J.goals;
  A.slots = J.slots;
  A.dist = J.dist;
  A.dstride = J.dstride;
  A.work = J.work;
  A.err = J.err;
}
template <class Args>
static void bfs_fill_goals(Args& A, const BfsJob& J) {  // ... and the goal-per-wave / -workgroup ones
  bfs_fill(A, J);
  A.k = J.k;
  A.govf = J.govf;
  A.vec16 = J.vec16;
}

// before a rung's launch: the profile buffer (the kernels that fill one) and the work counter zeroed
static int bfs_begin(tsw_ctx* c, BfsJob& J, bool prof) {
  J.prof = prof ? (uint64_t*)bfs_prof_buf(c) : nullptr;
  HIPCHK(hipMemsetAsync(J.work, 0, 4, c->s));
  return TSW_OK;
}

// after it: the profile print, and the next-hop codes from k_classify over the finished tables
static int bfs_finish(tsw_ctx* c, const BfsJob& J, const char* name) {
  if (J.prof) TRY(bfs_prof_print(c, name, J.k));
  if (J.nh) HIPCHK(launch_classify(c->G, J.goals, J.slots, J.k, J.dist, J.dstride, J.nh, c->s));
  return TSW_OK;
}

// goal-bit-parallel groups (the launch order came from bfs_mg_order)
static int run_bfs_mg(tsw_ctx* c, BfsJob& J) {
  const uint32_t ngroups = (uint32_t)c->h_mg_grp.size() - 1u;
  const uint32_t wlw = (c->G.ncell + 1u) / 2u;
  const uint32_t wgs = (uint32_t)std::max(c->num_cu, 1);
  if (c->mg_wgs < wgs || !c->d_mg_wl) {
    HIPCHK(hipStreamSynchronize(c->s));
    c->mg_wgs = 0;
    HIPCHK(c->d_mg_wl.reset());
    HIPCHK(c->d_mg_anch.reset());
    HIPCHK(c->d_mg_wl.alloc((size_t)wgs * wlw));
    HIPCHK(c->d_mg_anch.alloc((size_t)wgs * std::max<uint32_t>(c->nrs, 1u) * 16u));
    c->mg_wgs = wgs;
  }
  TRY(grow_synced(c, c->d_mg_grp, c->h_mg_grp.size()));
  HIPCHK(hipMemcpyAsync(c->d_mg_grp, c->h_mg_grp.data(), c->h_mg_grp.size() * 4u, hipMemcpyHostToDevice, c->s));
  TRY(bfs_begin(c, J, true));
  MgBfsArgs A{};
  bfs_fill(A, J);
  A.W = c->G.W;
  A.H = c->G.H;
  A.Bp = c->Bp;
  A.nbp = c->nbp;
  A.bp_magic = bp_magic(c->Bp);
  A.frb = c->d_frb;
  A.abase = c->d_abase;
  A.nrs = std::max<uint32_t>(c->nrs, 1u);
  A.grp = c->d_mg_grp;
  A.ngroups = ngroups;
  A.wl = c->d_mg_wl;
  A.wlw = wlw;
  A.anch = c->d_mg_anch;
  A.scratch_wgs = c->mg_wgs;
  A.prof = J.prof;
  HIPCHK(launch_bfs_mg(A, c->max_lds, c->num_cu, c->s));
  // the host copy of the group offsets must outlive the async upload
  HIPCHK(hipStreamSynchronize(c->s));
  return bfs_finish(c, J, "k_bfs_mg");
}

// one wave per goal over 8x8 blocks
static int run_bfs_blk(tsw_ctx* c, BfsJob& J, const BfsChoice& ch) {
  // scratch per goal slot: one per wave, two with TSW_BFS_PAIR
  TRY(ensure_wave_scratch(c, (uint64_t)c->num_cu * ch.waves_per_block * (ch.pair ? 2u : 1u), std::max<size_t>(c->nrs, 1),
                          (size_t)c->nbp * 2u));
  TRY(ensure_wlg(c));
  TRY(bfs_begin(c, J, true));
  BlkBfsArgs A{};
  bfs_fill_goals(A, J);
  A.W = c->G.W;
  A.H = c->G.H;
  A.BW = c->BW;
  A.BH = c->BH;
  A.Bp = c->Bp;
  A.nbp = c->nbp;
  A.cap = ch.cap;
  A.frb = c->d_frb;
  A.abase = c->d_abase;
  A.nrs = c->nrs;
  A.anch = c->d_anch;
  A.lovf = c->d_lovf;
  A.wlg = c->d_wlg;
  A.stage = (J.dstride % 8u == 0u && ((uintptr_t)J.dist & 15u) == 0u && !c->tun.bfs_nostage) ? 1u : 0u;
  A.dbg = c->tun.bfs_dbg;
  A.wls = c->tun.bfs_wls;
  A.pair = ch.pair ? 1u : 0u;
  A.max_waves = ch.waves_per_block;
  A.scratch_waves = std::min(c->wave_scratch, c->wlg_waves);
  A.prof = J.prof;
  HIPCHK(launch_bfs_blk(A, c->max_lds, c->num_cu, c->s));
  return bfs_finish(c, J, "k_bfs_blk");
}

// large grids (e.g. 1024x1024): one workgroup per goal, shared visited bitmap in LDS
static int run_bfs_big(tsw_ctx* c, BfsJob& J, const BfsChoice& ch) {
  const uint32_t nwg = bfs_big_workgroups(c->nbp, ch.cap, c->num_cu);
  TRY(ensure_wave_scratch(c, nwg, std::max<size_t>(c->nrs, 1), (size_t)c->nbp * 2u));
  TRY(ensure_wlg(c));
  TRY(bfs_begin(c, J, false));
  BigBfsArgs A{};
  bfs_fill_goals(A, J);
  A.W = c->G.W;
  A.H = c->G.H;
  A.BW = c->BW;
  A.BH = c->BH;
  A.Bp = c->Bp;
  A.nbp = c->nbp;
  A.cap = ch.cap;
  A.frb = c->d_frb;
  A.abase = c->d_abase;
  A.nrs = std::max<uint32_t>(c->nrs, 1u);
  A.anch = c->d_anch;
  A.lovf = c->d_lovf;
  A.wlg = reinterpret_cast<uint64_t*>(c->d_wlg.p);
  A.scratch_wgs = (uint32_t)std::min<uint64_t>(c->wave_scratch, c->wlg_waves);
  HIPCHK(launch_bfs_big(A, c->max_lds, c->num_cu, c->s));
  return bfs_finish(c, J, "k_bfs_big");
}

// one wave per goal over row words
static int run_bfs_wave(tsw_ctx* c, BfsJob& J, const BfsChoice& ch) {
  TRY(ensure_wave_scratch(c, (uint64_t)c->num_cu * ch.waves_per_block, (size_t)c->npw * 32u, (size_t)c->npw * 2u));
  TRY(bfs_begin(c, J, true));
  WaveBfsArgs A{};
  bfs_fill_goals(A, J);
  A.W = c->G.W;
  A.H = c->G.H;
  A.Ww = c->G.Ww;
  A.Wp = c->Wp;
  A.npw = c->npw;
  A.cap = ch.cap;
  A.frp = c->d_frp;
  A.anch = c->d_anch;
  A.lovf = c->d_lovf;
  A.max_waves = c->tun.bfs_waves;
  A.scratch_waves = c->wave_scratch;
  A.prof = J.prof;
  HIPCHK(launch_bfs_wave(A, c->max_lds, c->num_cu, c->s));
  return bfs_finish(c, J, "k_bfs_wave");
}

// What a forced kernel that does not fit the grid is refused with; nullptr for k_bfs, the last resort of the
// auto mode, whose own launcher reports a misfit.
static const char* bfs_misfit(BfsKernel k) {
  switch (k) {
    case BFS_MG: return "k_bfs_mg does not fit this grid (forced kernel mg)";
    case BFS_BLK: return "k_bfs_blk does not fit this grid (forced kernel blk)";
    case BFS_WAVE: return "k_bfs_wave does not fit this grid (forced kernel wave)";
    case BFS_BIG: return "k_bfs_big does not fit this grid (forced kernel big)";
    case BFS_BLOCK: break;
  }
  return nullptr;
}

// K1 over k goals (device arrays; slots may be null = goal index) with the kernel choose_bfs picks for this
// grid (tsw_place.h). Next-hop codes (nh != null) come fused from k_bfs, or from k_classify over the
// finished tables after the other kernels.
static int run_bfs(tsw_ctx* c, const uint32_t* goals, const uint32_t* slots, uint32_t k, uint16_t* dist, uint64_t dstride,
                   uint8_t* nh, uint8_t* govf = nullptr) {
  if (k == 0) return TSW_OK;
  BfsChoice ch = bfs_choice(c);
  // k_bfs_mg runs the groups of bfs_mg_order: a launch whose order did not come from there has none
  if (ch.kernel == BFS_MG && (c->h_mg_grp.empty() || c->h_mg_grp.back() != k)) ch.fits = false;
  if (!ch.fits && bfs_misfit(ch.kernel)) RET(TSW_EINVAL, bfs_misfit(ch.kernel));
  const bool vec16 = c->G.W % 8u == 0u && dstride % 8u == 0u && ((uintptr_t)dist & 15u) == 0u;
  BfsJob J{goals, slots, k, dist, dstride, nh, govf, vec16 ? 1u : 0u, &c->d_stat->work, &c->d_stat->err, nullptr};
  Timer t(c, CAT_BFS);
  switch (ch.kernel) {
    case BFS_MG: return run_bfs_mg(c, J);
    case BFS_BLK: return run_bfs_blk(c, J, ch);
    case BFS_WAVE: return run_bfs_wave(c, J, ch);
    case BFS_BIG: return run_bfs_big(c, J, ch);
    case BFS_BLOCK:
      HIPCHK(launch_bfs(c->G, goals, slots, k, dist, dstride, nh, dstride, &c->d_stat->err, c->max_lds, c->num_cu, c->s, govf));
  }
  return TSW_OK;
}

constexpr uint32_t NO_GOAL = 0xFFFFFFFFu;

// Grow the device store to at least `need` slots (never past the budget; callers check).
static int grow_store(tsw_ctx* c, size_t need) {
  if (need <= c->tab_cap) return TSW_OK;
  const uint64_t max_tabs = c->table_budget / (c->tstride * 2ull);
  size_t nc = std::max<size_t>(need, std::max<size_t>((size_t)c->tab_cap * 2, 64));
  nc = std::max<size_t>(need, std::min<size_t>(nc, (size_t)max_tabs));
  HIPCHK(hipStreamSynchronize(c->s));
  DevBuf<uint8_t> nd, nn;  // the live tables are copied over before the old blocks go
  HIPCHK(nd.alloc(nc * c->tstride));
  if (hipError_t e = nn.alloc(nc * c->tstride); e != hipSuccess)
    RET(TSW_ENOMEM, std::string("table store growth: ") + hipGetErrorString(e));
  if (c->tab_count) {
    HIPCHK(hipMemcpyAsync(nd, c->d_dt, (size_t)c->tab_count * c->tstride, hipMemcpyDeviceToDevice, c->s));
    HIPCHK(hipMemcpyAsync(nn, c->d_nh, (size_t)c->tab_count * c->tstride, hipMemcpyDeviceToDevice, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  c->d_dt = std::move(nd);
  c->d_nh = std::move(nn);
  c->tab_cap = (uint32_t)nc;
  c->h_tab_goal.resize(nc, NO_GOAL);
  c->h_tab_stamp.resize(nc, 0);
  c->h_tab_tableless.resize(nc, 0);
  return TSW_OK;
}

// Stamp the tables of `goals` as used by the current call and collect the goals that have none
// (deduplicated, marked -2 in h_goal_tab until committed or rolled back).
static void stamp_and_collect(tsw_ctx* c, const uint32_t* goals, size_t k, std::vector<uint32_t>& newg,
                       std::vector<uint32_t>* src = nullptr) {
  ++c->call_stamp;
  for (size_t i = 0; i < k; ++i) {
    const uint32_t g = goals[i];
    const int32_t t = c->h_goal_tab[g];
    if (t >= 0) {
      c->h_tab_stamp[t] = c->call_stamp;
    } else if (t == -1) {
      c->h_goal_tab[g] = -2;
      newg.push_back(g);
      if (src) src->push_back((uint32_t)i);
    }
  }
}

// Slots for k new tables: free slots first, then growth up to the budget, then the least-recently
// used live tables that the current call does not use (LRU eviction — a long-running per-tick
// manager streams goals through a bounded store instead of failing, SURVEY §7 hard part 4).
// Evicted goals lose their table (goal_tab -1); later calls rebuild them on demand.
static int reserve_slots(tsw_ctx* c, size_t k, std::vector<uint32_t>& slots) {
  slots.clear();
  const uint64_t max_tabs = c->table_budget / (c->tstride * 2ull);
  while (slots.size() < k && !c->tab_free.empty()) {
    slots.push_back(c->tab_free.back());
    c->tab_free.pop_back();
  }
  size_t want = k - slots.size();
  const size_t fresh = std::min<size_t>(want, max_tabs > c->tab_count ? (size_t)(max_tabs - c->tab_count) : 0u);
  if (fresh) {
    if (int r = grow_store(c, (size_t)c->tab_count + fresh); r != TSW_OK) {
      c->tab_free.insert(c->tab_free.end(), slots.begin(), slots.end());
      slots.clear();
      return r;
    }
    for (size_t j = 0; j < fresh; ++j) slots.push_back(c->tab_count++);
    want -= fresh;
  }
  if (want) {
    std::vector<uint32_t> cand;
    for (uint32_t s = 0; s < c->tab_count; ++s)
      if (c->h_tab_goal[s] != NO_GOAL && c->h_tab_stamp[s] < c->call_stamp) cand.push_back(s);
    if (cand.size() < want) {
      c->tab_free.insert(c->tab_free.end(), slots.begin(), slots.end());
      slots.clear();
      RET(TSW_ENOMEM, "goal-table budget exceeded by the goals of one call (raise tsw_opts.table_budget_bytes)");
    }
    std::partial_sort(cand.begin(), cand.begin() + want, cand.end(),
                      [&](uint32_t a, uint32_t b) { return c->h_tab_stamp[a] < c->h_tab_stamp[b]; });
    for (size_t j = 0; j < want; ++j) {
      const uint32_t s = cand[j];
      c->h_goal_tab[c->h_tab_goal[s]] = -1;
      c->h_tab_goal[s] = NO_GOAL;
      --c->tab_live;
      ++c->evictions;
      slots.push_back(s);
    }
  }
  return TSW_OK;
}

// Commit (rc == OK) or roll back the new goals and their reserved slots, then publish goal_tab.
static int finish_tables(tsw_ctx* c, int rc, const std::vector<uint32_t>& newg, const std::vector<uint32_t>& slots) {
  for (size_t j = 0; j < newg.size(); ++j) {
    if (rc == TSW_OK && j < slots.size()) {
      c->h_goal_tab[newg[j]] = (int32_t)slots[j];
      c->h_tab_goal[slots[j]] = newg[j];
      c->h_tab_stamp[slots[j]] = c->call_stamp;
    } else {
      c->h_goal_tab[newg[j]] = -1;
    }
  }
  if (rc == TSW_OK) c->tab_live += (uint32_t)newg.size();
  else c->tab_free.insert(c->tab_free.end(), slots.begin(), slots.end());
  c->st.tables = c->tab_live;
  const std::string keep = c->err;
  if (hipMemcpyAsync(c->d_goal_tab, c->h_goal_tab.data(), (size_t)c->G.ncell * 4, hipMemcpyHostToDevice, c->s) !=
          hipSuccess ||
      hipStreamSynchronize(c->s) != hipSuccess) {
    if (rc == TSW_OK) RET(TSW_EHIP, "goal_tab upload failed");
  }
  c->err = keep;
  return rc;
}

// tableless_ok: a goal whose distances overflow u16 is registered WITHOUT a table (next hops by K3)
// instead of failing the call — planning entry points; the table-returning ones pass false.
static int build_new_tables(tsw_ctx* c, const std::vector<uint32_t>& newg, const std::vector<uint32_t>& slots,
                     bool tableless_ok) {
  std::vector<uint32_t>& lg = c->h_lpt_goals;
  std::vector<uint32_t>& ls = c->h_lpt_slots;
  lg.resize(newg.size());
  ls.resize(newg.size());
  TRY(ensure_tmp(c, newg.size()));
  if (tableless_ok) {
    TRY(grow_synced(c, c->d_govf, newg.size()));
    HIPCHK(hipMemsetAsync(c->d_govf, 0, newg.size(), c->s));
  }
  // K1 in batches into the u16 buffer, each batch classified into the store (codes + detour bytes):
  // the u16 tables never live in the store (round 6: 3 -> 2 B per cell per goal; C5 79.5 -> ~57 GiB)
  // (launch order per batch: longest BFS first, bfs_lpt_order; lg / ls hold the ordered goals / store slots)
  size_t batch = 0;
  TRY(ensure_ktmp(c, newg.size(), &batch));
  for (size_t i0 = 0; i0 < newg.size(); i0 += batch) {
    const uint32_t nb = (uint32_t)std::min(batch, newg.size() - i0);
    std::vector<uint32_t> bg(newg.begin() + i0, newg.begin() + i0 + nb), bs(slots.begin() + i0, slots.begin() + i0 + nb);
    bfs_lpt_order(c, bg, bs);
    std::copy(bg.begin(), bg.end(), lg.begin() + i0);
    std::copy(bs.begin(), bs.end(), ls.begin() + i0);
    HIPCHK(hipMemcpyAsync(c->d_tmp_a + i0, lg.data() + i0, (size_t)nb * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_tmp_b + i0, ls.data() + i0, (size_t)nb * 4, hipMemcpyHostToDevice, c->s));
    TRY(run_bfs(c, c->d_tmp_a + i0, nullptr, nb, c->d_ktmp, c->tstride, nullptr,
                tableless_ok ? c->d_govf + i0 : nullptr));
    HIPCHK(launch_classify_dt(c->G, c->d_tmp_a + i0, nullptr, c->d_tmp_b + i0, nb, c->d_ktmp, c->tstride, c->d_nh,
                              c->d_dt, c->tstride, c->s));
    HIPCHK(hipStreamSynchronize(c->s));  // the host copies bg / bs and the mg group offsets are reused next batch
  }
  c->st.bfs_goals += newg.size();
  c->st.bfs_launches++;
  for (uint32_t s : slots) c->h_tab_tableless[s] = 0;
  HIPCHK(hipMemcpyAsync(&c->h_stat->err, &c->d_stat->err, 4, hipMemcpyDeviceToHost, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  if (tableless_ok && c->h_stat->err == ERR_DIST_OVERFLOW) {
    std::vector<uint8_t> f(newg.size());
    HIPCHK(hipMemcpy(f.data(), c->d_govf, f.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < f.size(); ++i) {
      if (!f[i]) continue;
      const uint32_t slot = ls[i];
      c->h_tab_tableless[slot] = 1;
      ++c->st.tableless_goals;
      // no distance (DAG prefetch reads DT_NONE: nothing to follow) and every code unresolved (K3)
      HIPCHK(hipMemsetAsync(c->d_dt + (size_t)slot * c->tstride, 0xFF, c->tstride, c->s));
      HIPCHK(hipMemsetAsync(c->d_nh + (size_t)slot * c->tstride, 0xFF, c->tstride, c->s));
    }
    HIPCHK(hipMemsetAsync(&c->d_stat->err, 0, 4, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
  }
  return check_err(c);
}

// K1 of `goals` (host array) into u16 tables for an API that returns them: batches through the K1
// buffer, each batch handed to `take(device tables, first goal index, count)` (the store holds detour
// bytes only, tsw_internal.h).
template <class Take>
static int build_u16(tsw_ctx* c, const uint32_t* goals, uint32_t k, Take&& take) {
  size_t batch = 0;
  TRY(ensure_ktmp(c, k, &batch));
  TRY(ensure_tmp(c, std::min<size_t>(k, batch)));
  for (uint32_t i0 = 0; i0 < k; i0 += (uint32_t)batch) {
    const uint32_t nb = (uint32_t)std::min<size_t>(batch, k - i0);
    // launch order longest-first (bfs_lpt_order); the slots carry each table's position in the batch
    std::vector<uint32_t> bg(goals + i0, goals + i0 + nb), bs(nb);
    for (uint32_t j = 0; j < nb; ++j) bs[j] = j;
    bfs_lpt_order(c, bg, bs);
    HIPCHK(hipMemcpyAsync(c->d_tmp_a, bg.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_tmp_b, bs.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->s));
    TRY(run_bfs(c, c->d_tmp_a, c->d_tmp_b, nb, c->d_ktmp, c->tstride, nullptr));
    TRY(take(c->d_ktmp, i0, nb));
    HIPCHK(hipStreamSynchronize(c->s));  // the next batch reuses the buffer and the goal upload
  }
  return check_err(c);
}

// Make sure every goal in `goals` (valid free cells) has a table. A failed K1 build (HIP error,
// distance overflow when !tableless_ok) leaves no goal registered against a partial table.
int ensure_tables(tsw_ctx* c, const std::vector<uint32_t>& goals_in, bool tableless_ok) {
  std::vector<uint32_t> newg, slots;
  newg.reserve(goals_in.size());
  stamp_and_collect(c, goals_in.data(), goals_in.size(), newg);
  if (newg.empty()) return TSW_OK;
  int rc = reserve_slots(c, newg.size(), slots);
  if (rc == TSW_OK) rc = build_new_tables(c, newg, slots, tableless_ok);
  TRY(finish_tables(c, rc, newg, slots));
  if (eager_policy(c, newg.size())) {
    // eager resolution over real tables only (a tableless goal stays lazy: one A* per cell would be
    // a whole-grid search per cell)
    std::vector<uint32_t> eg, es;
    for (size_t j = 0; j < newg.size(); ++j)
      if (!c->h_tab_tableless[slots[j]]) {
        eg.push_back(newg[j]);
        es.push_back(slots[j]);
      }
    TRY(resolve_all_unknown(c, eg, es));
  }
  return TSW_OK;
}

// TSW_EOVERFLOW if any of `goals` (with tables) is held without one (its distances overflow u16).
static int require_real_tables(tsw_ctx* c, const std::vector<uint32_t>& goals) {
  for (uint32_t g : goals) {
    const int32_t t = c->h_goal_tab[g];
    if (t >= 0 && c->h_tab_tableless[t])
      RET(TSW_EOVERFLOW, "goal farther than 65534 steps from some cell: no u16 distance table (plans use K3)");
  }
  return TSW_OK;
}

}  // namespace tsw

extern "C" {

int tsw_dist_tables(tsw_ctx* c, const uint32_t* goals, uint32_t k, uint16_t* out) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!goals || !out) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  std::vector<uint32_t> gv(goals, goals + k);
  for (uint32_t g : gv)
    if (!cell_id_ok(c, g)) RET(TSW_EINVAL, "goal cell off-grid or blocked");
  TRY(ensure_tables(c, gv));
  TRY(require_real_tables(c, gv));
  const size_t ncell = c->G.ncell;
  TRY(build_u16(c, gv.data(), k, [&](const uint16_t* d, uint32_t i0, uint32_t nb) -> int {
    for (uint32_t j = 0; j < nb; ++j)
      HIPCHK(hipMemcpyAsync(out + (size_t)(i0 + j) * ncell, d + (size_t)j * c->tstride, ncell * 2,
                            hipMemcpyDeviceToHost, c->s));
    return TSW_OK;
  }));
  resolve_timing(c);
  return TSW_OK;
}

int tsw_dist_tables_device(tsw_ctx* c, const uint32_t* goals, uint32_t k, uint16_t* dev_out) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!goals || !dev_out) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  for (uint32_t i = 0; i < k; ++i)
    if (!cell_id_ok(c, goals[i])) RET(TSW_EINVAL, "goal cell off-grid or blocked");
  // dev_out may have been allocated / zero-filled on another stream of the caller (e.g. torch's
  // current stream): order every outstanding device work before writing into it
  HIPCHK(hipDeviceSynchronize());
  TRY(ensure_tmp(c, k));
  // context-owned staging (like the caller's `goals`, read by the copy before it returns)
  std::vector<uint32_t>& lg = c->h_lpt_goals;
  std::vector<uint32_t>& ls = c->h_lpt_slots;
  lg.assign(goals, goals + k);
  ls.resize(k);
  for (uint32_t i = 0; i < k; ++i) ls[i] = i;
  bfs_lpt_order(c, lg, ls);
  HIPCHK(hipMemcpyAsync(c->d_tmp_a, lg.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipMemcpyAsync(c->d_tmp_b, ls.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->s));
  TRY(run_bfs(c, c->d_tmp_a, c->d_tmp_b, k, dev_out, c->G.ncell, nullptr));
  c->st.bfs_goals += k;
  c->st.bfs_launches++;
  TRY(check_err(c));
  resolve_timing(c);
  return TSW_OK;
}

int tsw_import_tables_device(tsw_ctx* c, const uint32_t* goals, uint32_t k, const uint16_t* dev_tables) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!goals || !dev_tables) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  for (uint32_t i = 0; i < k; ++i)
    if (!cell_id_ok(c, goals[i])) RET(TSW_EINVAL, "goal cell off-grid or blocked");
  // the tables were produced on the caller's streams (e.g. an RCCL all-gather): complete first
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint32_t> newg, src, slots;
  stamp_and_collect(c, goals, k, newg, &src);
  if (newg.empty()) return TSW_OK;
  auto ingest = [&]() -> int {
    TRY(reserve_slots(c, newg.size(), slots));
    for (uint32_t sl : slots) c->h_tab_tableless[sl] = 0;  // imported: real u16 tables
    TRY(ensure_tmp(c, newg.size()));
    HIPCHK(hipMemcpyAsync(c->d_tmp_a, newg.data(), newg.size() * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_tmp_b, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_tmp_c, src.data(), src.size() * 4, hipMemcpyHostToDevice, c->s));
    // codes and detour bytes straight from the caller's u16 tables (the store keeps no u16 copy)
    HIPCHK(launch_classify_dt(c->G, c->d_tmp_a, c->d_tmp_c, c->d_tmp_b, (uint32_t)newg.size(), dev_tables,
                              c->G.ncell, c->d_nh, c->d_dt, c->tstride, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    return TSW_OK;
  };
  TRY(finish_tables(c, ingest(), newg, slots));
  if (eager_policy(c, newg.size())) TRY(resolve_all_unknown(c, newg, slots));
  resolve_timing(c);
  return TSW_OK;
}

int tsw_next_hop_tables(tsw_ctx* c, const uint32_t* goals, uint32_t k, uint8_t* out) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!goals || !out) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  std::vector<uint32_t> gv(goals, goals + k);
  for (uint32_t g : gv)
    if (!cell_id_ok(c, g)) RET(TSW_EINVAL, "goal cell off-grid or blocked");
  TRY(ensure_tables(c, gv, true));
  const size_t ncell = c->G.ncell;
  for (uint32_t i = 0; i < k; ++i) {
    const int32_t slot = c->h_goal_tab[gv[i]];
    HIPCHK(hipMemcpyAsync(out + (size_t)i * ncell, c->d_nh + (size_t)slot * c->tstride, ncell,
                          hipMemcpyDeviceToHost, c->s));
  }
  HIPCHK(hipStreamSynchronize(c->s));
  resolve_timing(c);
  return TSW_OK;
}

int tsw_next_hop_tables_device(tsw_ctx* c, const uint32_t* goals, uint32_t k, uint8_t* dev_out, uint16_t* dev_dist) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!goals || !dev_out) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  std::vector<uint32_t> gv(goals, goals + k);
  for (uint32_t g : gv)
    if (!cell_id_ok(c, g)) RET(TSW_EINVAL, "goal cell off-grid or blocked");
  HIPCHK(hipDeviceSynchronize());  // dev_out may come from another stream of the caller
  TRY(ensure_tables(c, gv));
  TRY(require_real_tables(c, gv));
  // eager resolution of this shard's multi-candidate cells, whatever the context's policy
  std::vector<uint32_t> ug, us;
  std::vector<uint8_t> seen(c->tab_count, 0);
  for (uint32_t g : gv) {
    const int32_t slot = c->h_goal_tab[g];
    if (slot >= 0 && !seen[slot]) {
      seen[slot] = 1;
      ug.push_back(g);
      us.push_back((uint32_t)slot);
    }
  }
  TRY(resolve_all_unknown(c, ug, us));
  const size_t ncell = c->G.ncell;
  for (uint32_t i = 0; i < k; ++i) {
    const int32_t slot = c->h_goal_tab[gv[i]];
    HIPCHK(hipMemcpyAsync(dev_out + (size_t)i * ncell, c->d_nh + (size_t)slot * c->tstride, ncell,
                          hipMemcpyDeviceToDevice, c->s));
  }
  // the u16 K1 tables beside the codes (the store holds detour bytes only: K1 again, into the caller's buffer)
  if (dev_dist)
    TRY(build_u16(c, gv.data(), k, [&](const uint16_t* d, uint32_t i0, uint32_t nb) -> int {
      for (uint32_t j = 0; j < nb; ++j)
        HIPCHK(hipMemcpyAsync(dev_dist + (size_t)(i0 + j) * ncell, d + (size_t)j * c->tstride, ncell * 2,
                              hipMemcpyDeviceToDevice, c->s));
      return TSW_OK;
    }));
  HIPCHK(hipStreamSynchronize(c->s));
  resolve_timing(c);
  return TSW_OK;
}

int tsw_import_next_hops_device(tsw_ctx* c, const uint32_t* goals, uint32_t k, const uint16_t* dev_dist,
                                const uint8_t* dev_nh) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (k == 0) return TSW_OK;
  if (!goals || !dev_dist || !dev_nh) RET(TSW_EINVAL, "null argument");
  TRY(set_device(c));
  for (uint32_t i = 0; i < k; ++i)
    if (!cell_id_ok(c, goals[i])) RET(TSW_EINVAL, "goal cell off-grid or blocked");
  HIPCHK(hipDeviceSynchronize());  // produced on the caller's streams (e.g. an RCCL all-gather)
  std::vector<uint32_t> newg, src, slots;
  stamp_and_collect(c, goals, k, newg, &src);
  if (newg.empty()) return TSW_OK;
  auto ingest = [&]() -> int {
    TRY(reserve_slots(c, newg.size(), slots));
    for (uint32_t sl : slots) c->h_tab_tableless[sl] = 0;  // imported: real u16 tables
    const size_t ncell = c->G.ncell;
    for (size_t j = 0; j < newg.size(); ++j)
      HIPCHK(hipMemcpyAsync(c->d_nh + (size_t)slots[j] * c->tstride, dev_nh + (size_t)src[j] * ncell, ncell,
                            hipMemcpyDeviceToDevice, c->s));
    // detour bytes from the u16 tables (the imported codes stay: nh = null)
    TRY(ensure_tmp(c, newg.size()));
    HIPCHK(hipMemcpyAsync(c->d_tmp_a, newg.data(), newg.size() * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_tmp_b, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(hipMemcpyAsync(c->d_tmp_c, src.data(), src.size() * 4, hipMemcpyHostToDevice, c->s));
    HIPCHK(launch_classify_dt(c->G, c->d_tmp_a, c->d_tmp_c, c->d_tmp_b, (uint32_t)newg.size(), dev_dist, ncell,
                              nullptr, c->d_dt, c->tstride, c->s));
    // a pending marker from the producing context means "not resolved": unknown here — swept over
    // the imported slots only (a whole-store sweep grows with every table the context holds)
    for (size_t j = 0; j < newg.size(); ++j)
      HIPCHK(launch_reset_pending(c->d_nh + (size_t)slots[j] * c->tstride, c->tstride, c->s));
    HIPCHK(hipStreamSynchronize(c->s));
    return TSW_OK;
  };
  TRY(finish_tables(c, ingest(), newg, slots));
  resolve_timing(c);
  return TSW_OK;
}

int tsw_clear_tables(tsw_ctx* c) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  TRY(set_device(c));
  HIPCHK(hipStreamSynchronize(c->s));
  std::fill(c->h_goal_tab.begin(), c->h_goal_tab.end(), -1);
  HIPCHK(hipMemcpyAsync(c->d_goal_tab, c->h_goal_tab.data(), (size_t)c->G.ncell * 4, hipMemcpyHostToDevice, c->s));
  HIPCHK(hipStreamSynchronize(c->s));
  c->tab_count = 0;
  c->tab_live = 0;
  c->tab_free.clear();
  std::fill(c->h_tab_goal.begin(), c->h_tab_goal.end(), NO_GOAL);
  c->st.tables = 0;
  return TSW_OK;
}

}  // extern "C"
