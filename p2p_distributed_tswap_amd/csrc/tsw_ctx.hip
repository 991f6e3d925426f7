// tsw_ctx.hip — the context of the TSWAP planning core's host runtime behind the C ABI declared in
// include/tswap.h: create / destroy, the diagnostic tunables, the build id, stats and timing. The runtime
// owns device memory (tsw_ctx.h), the goal-table store (BFS distances + next-hop codes, tsw_tables.hip),
// the A* scratch slots (tsw_query.hip) and the per-step orchestration (tsw_plan_host.hip): K1 tables ->
// k_plan (persistent K4 assign + K2 step + record), relaunched after each batched K3 (A*) pass over the
// next hops it could not resolve; tsw_fleet_host.hip holds the decentralized tick's entry points.
// The only translation unit of the five that depends on the build flavour (-DTSW_DIAG, TSW_SRC_HASH).
//
// Reference call structure being replaced (RenKoya1/p2p_distributed_tswap):
//   tswap_mapd            src/algorithm/tswap.rs:39-172      -> tsw_plan_mapd
//   tswap_step            src/algorithm/tswap.rs:174-286     -> tsw_step
//   get_path              src/algorithm/tswap.rs:288-390     -> tsw_get_path_next
//   plan_all_paths' step  src/bin/centralized/manager.rs:101-144 -> tsw_step
#include "tsw_ctx.h"

namespace {

thread_local std::string g_create_err;

constexpr uint32_t HOST_RING_ENTRIES = 1u << 14;  // a t = 0 burst of every agent fits (C5: 10,000)

}  // namespace

// build provenance (tsw_build_id): first 16 hex digits of the sha1 of the sources, set by the build
#ifndef TSW_SRC_HASH
#define TSW_SRC_HASH 0ull
#endif

Tunables Tunables::from_env() {
  Tunables t;
#ifdef TSW_DIAG
  auto num = [](const char* k, long lo, long hi, long def) -> long {
    const char* v = getenv(k);
    if (!v) return def;
    return std::max(lo, std::min(hi, atol(v)));
  };
  if (const char* m = getenv("TSW_BFS_KERNEL"))
    t.bfs_mode = !strcmp(m, "wave") ? 1u : !strcmp(m, "block") ? 2u : !strcmp(m, "blk") ? 3u : !strcmp(m, "big") ? 4u : !strcmp(m, "mg") ? 5u : 0u;
  t.bfs_cap = (uint32_t)num("TSW_BFS_LISTCAP", 1, 32768, t.bfs_cap);
  t.blk_cap = (uint32_t)num("TSW_BFS_BLKCAP", 1, 32768, t.blk_cap);
  t.bfs_waves = (uint32_t)num("TSW_BFS_WAVES", 1, 16, t.bfs_waves);
  t.bfs_order = num("TSW_BFS_ORDER", 0, 1, 1) != 0;
  t.bfs_prof = getenv("TSW_BFS_PROF") != nullptr;
  t.bfs_nostage = getenv("TSW_BFS_NOSTAGE") != nullptr;
  t.bfs_dbg = (uint32_t)num("TSW_BFS_DBG", 0, 7, 0);
  t.bfs_wls = (uint32_t)num("TSW_BFS_WLS", 0, 1, t.bfs_wls);
  t.bfs_pair = (uint32_t)num("TSW_BFS_PAIR", 0, 1, t.bfs_pair);
  t.wave_hcap = (uint32_t)num("TSW_ASTAR_WAVE_HCAP", 4, 1 << 20, 0);
  t.astar_global_gs = (int)num("TSW_ASTAR_GLOBAL_GS", 0, 1, -1);
  t.astar_tier2 = getenv("TSW_ASTAR_NO_TIER2") == nullptr;
  t.astar_diag = (getenv("TSW_ASTAR_SERIAL") ? ASTAR_DIAG_SERIAL : 0u) | (getenv("TSW_ASTAR_PROF") ? ASTAR_DIAG_PROF : 0u);
  t.prefetch = getenv("TSW_NO_PREFETCH") == nullptr;
  t.wave_rules_max = (uint32_t)num("TSW_WAVE_RULES_MAX", 0, 0xFFFFFFFFl, t.wave_rules_max);
  t.walk_cap = (uint32_t)num("TSW_WALK_CAP", 0, 4096, t.walk_cap);
  t.wide_prefetch = (uint32_t)num("TSW_WIDE_PREFETCH", 0, 1 << 16, t.wide_prefetch);
  t.wide_hi = (uint32_t)num("TSW_WIDE_HI", 0, 1 << 16, t.wide_hi);
  t.wide_lo = (uint32_t)num("TSW_WIDE_LO", 1, 1 << 16, t.wide_lo);
  t.dag_prefetch = (uint32_t)num("TSW_DAG_PREFETCH", 0, 16, t.dag_prefetch);
  t.dag_width = (uint32_t)num("TSW_DAG_WIDTH", 1, 16, t.dag_width);
  t.urgent_hops = (uint32_t)num("TSW_URGENT_HOPS", 0, 16, t.urgent_hops);
  t.chain_hops = (uint32_t)num("TSW_CHAIN_HOPS", 0, 1000000, t.chain_hops);
  t.hot_chains = num("TSW_HOT_CHAINS", 0, 1, t.hot_chains ? 1 : 0) != 0;
  t.predict = (uint32_t)num("TSW_PREDICT", 0, 3, t.predict);
  t.walk_cache = num("TSW_WALK_CACHE", 0, 1, 1) != 0;
  t.walk_step = (uint32_t)num("TSW_WALK_STEP", 0, 1 << 16, t.walk_step);
  t.move_round0 = (uint32_t)num("TSW_MOVE_ROUND0", 0, 0x7FFFFFFF, 0);
  t.ab_flags = (uint32_t)num("TSW_AB_FLAGS", 0, 255, t.ab_flags);
  t.t0_delay_us = (uint32_t)num("TSW_T0_DELAY_US", 0, 10000000, t.t0_delay_us);
  t.prefetch_ext = (uint32_t)num("TSW_PREFETCH_EXT", 0, 7, t.prefetch_ext);
  t.flinks_lds = getenv("TSW_NO_FLINKS_LDS") == nullptr;
  t.part_lds = (uint32_t)num("TSW_PART_LDS", 0, 0x7F, t.part_lds);
  t.agents_lds = num("TSW_AGENTS_LDS", 0, 1, 1) != 0;
  t.occ_split = num("TSW_OCC_SPLIT", 0, 1, 1) != 0;
  t.plan_block = (uint32_t)num("TSW_PLAN_BLOCK", 0, PLAN_BLOCK_MAX, 0) / 64u * 64u;
  t.plan_debug = getenv("TSW_PLAN_DEBUG") != nullptr;
  t.coop = num("TSW_COOP", 0, 1, 1) != 0;
  t.task_chains = num("TSW_TASK_CHAINS", 0, 1, 1) != 0;
  t.chain_preempt = num("TSW_CHAIN_PREEMPT", 0, 1, 1) != 0;
  t.avoid_xcc = num("TSW_WORKER_AVOID_XCD", 0, 1, 1) != 0;
  t.worker_gs = (int)num("TSW_WORKER_GS", -1, 2, -1);
  t.worker_fb = (int)num("TSW_WORKER_FB", -1, 1, -1);
  t.dag_exit = num("TSW_DAG_EXIT", 0, 1, 1) != 0;
  t.dag_mask = (uint32_t)num("TSW_DAG_MASK", 0, 0x7FFFFFFF, t.dag_mask);
  t.stale_steps = (uint32_t)num("TSW_SPEC_STALE", 0, 1 << 20, t.stale_steps);
  t.reg_heap = (uint32_t)num("TSW_ASTAR_REGHEAP", 0, 63, t.reg_heap);
  t.wake_gate = (uint32_t)num("TSW_WAKE_GATE", 0, 8, t.wake_gate);
  t.chain_mask = (int)num("TSW_CHAIN_MASK", -1, 15, -1);
  t.slow_poll = (uint32_t)num("TSW_SLOW_POLL", 0, 8, t.slow_poll);
  t.slow_mult = (uint32_t)num("TSW_SLOW_MULT", 1, 1024, t.slow_mult);
  t.worker_idle_us = (uint64_t)num("TSW_WORKER_IDLE_US", 1, 5000000, (long)t.worker_idle_us);
  t.host_astar = (int)num("TSW_HOST_ASTAR", 0, 16, -1);
  t.host_delay_us = (uint32_t)num("TSW_HOST_ASTAR_DELAY_US", 0, 1000000, 0);
  t.host_ring = (uint32_t)num("TSW_HOST_ASTAR_RING", 8, 1 << 14, 0);
  t.host_early = (uint32_t)num("TSW_HOST_ASTAR_EARLY", 0, 2, t.host_early);
  t.st_heap = (uint32_t)num("TSW_ST_HEAP", 0, 512, 0);
  t.st_waves = (uint32_t)num("TSW_ST_WAVES", 0, 1 << 20, 0);
  t.st_seg_words = (uint32_t)num("TSW_ST_SEG_WORDS", 0, 1 << 28, 0);
  t.st_tag0 = (uint32_t)num("TSW_ST_TAG0", 1, (1 << 18) - 1, 1);
#endif
  return t;
}

namespace tsw {

hipEvent_t ev_get(tsw_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}

void resolve_timing(tsw_ctx* c) {
  if (c->pending.empty()) return;
  hipEventSynchronize(c->pending.back().b);
  for (auto& e : c->pending) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, e.a, e.b);
    switch (e.cat) {
      case CAT_BFS: c->st.bfs_ms += ms; break;
      case CAT_ASTAR: c->st.astar_ms += ms; break;
      case CAT_WALK: c->st.walker_ms += ms; break;
      case CAT_ASSIGN: c->st.assign_ms += ms; break;
    }
    c->pool.push_back(e.a);
    c->pool.push_back(e.b);
  }
  c->pending.clear();
}

int set_device(tsw_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  return TSW_OK;
}

bool cell_ok(const tsw_ctx* c, uint32_t x, uint32_t y, uint32_t* cell) {
  if (x >= c->G.W || y >= c->G.H) return false;
  const uint32_t cc = y * c->G.W + x;
  if (!(c->h_nbmask[cc] & NB_FREE)) return false;
  *cell = cc;
  return true;
}

bool cell_id_ok(const tsw_ctx* c, uint32_t cell) {
  return cell < c->G.ncell && (c->h_nbmask[cell] & NB_FREE);
}

}  // namespace tsw

tsw_ctx::~tsw_ctx() {
  if (!host_pool.th.empty()) {
    {
      std::lock_guard<std::mutex> lk(host_pool.mu);
      host_pool.quit = true;
    }
    host_pool.cv.notify_all();
    for (auto& t : host_pool.th) t.join();
    host_pool.th.clear();
  }
  hipSetDevice(device);
  if (s) hipStreamSynchronize(s);
  for (auto& e : pending) {
    hipEventDestroy(e.a);
    hipEventDestroy(e.b);
  }
  for (auto e : pool) hipEventDestroy(e);
  if (s) hipStreamDestroy(s);
}

extern "C" {

tsw_ctx* tsw_create(const uint8_t* cells, uint32_t w, uint32_t h, const tsw_opts* opts) {
  if (!cells || w == 0 || h == 0) {
    g_create_err = "tsw_create: empty grid";
    return nullptr;
  }
  if (w > MAX_WH || h > MAX_WH || (uint64_t)w * h > MAX_CELLS) {
    g_create_err = "tsw_create: grid exceeds 2048 per side or 2^20 cells";
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_err = "tsw_create: no HIP device visible (the HIP path has no CPU fallback)";
    return nullptr;
  }
  tsw_ctx* c = new tsw_ctx();
  c->tun = Tunables::from_env();  // diagnostic build only: the only place the environment is read
  c->device = opts ? opts->device : 0;
  c->flags = opts ? opts->flags : 0;
  if (c->flags & TSW_F_EXIT_MODE) c->tun.coop = false;
  if (opts && opts->watchdog_ms) c->watchdog_ms = opts->watchdog_ms;
  {
    // host A* service threads: the measured default is the calling thread alone
    const uint32_t ha = opts ? opts->host_astar : 0u;
    c->host_threads = ha == TSW_HOST_ASTAR_OFF ? 0u : ha == 0u ? 1u : std::min<uint32_t>(ha, 16u);
    if (c->tun.host_astar >= 0) c->host_threads = (uint32_t)c->tun.host_astar;
  }
  if (c->device < 0 || c->device >= ndev) {
    g_create_err = "tsw_create: bad device ordinal";
    delete c;
    return nullptr;
  }
  auto fail = [&](const char* what, hipError_t e) {
    g_create_err = std::string("tsw_create: ") + what + ": " + hipGetErrorString(e);
    tsw_destroy(c);
    return (tsw_ctx*)nullptr;
  };
  // a device copy of a host vector; false: the context is gone and g_create_err says which half failed
  auto upload = [&](auto& buf, const auto& host, const char* name) {
    const char* step = "malloc ";
    hipError_t ue = buf.alloc(host.size());
    if (ue == hipSuccess) {
      step = "copy ";
      ue = hipMemcpy(buf.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice);
    }
    if (ue != hipSuccess) fail((std::string(step) + name).c_str(), ue);
    return ue == hipSuccess;
  };
  hipError_t e;
  if ((e = hipSetDevice(c->device)) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking)) != hipSuccess) return fail("stream", e);
  hipDeviceGetAttribute(&c->max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device);
  hipDeviceGetAttribute(&c->num_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  if (c->max_lds <= 0) c->max_lds = 65536;
  if (c->num_cu <= 0) c->num_cu = 256;

  const uint32_t ncell = w * h, ncp = (ncell + 7u) & ~7u, Ww = (w + 31u) / 32u;
  c->G.W = w;
  c->G.H = h;
  c->G.ncell = ncell;
  c->G.Ww = Ww;
  c->tstride = ncp;
  // graph build (tswap.rs:44-77): '@' blocked, neighbours S,E,N,W
  c->h_nbmask.assign(ncp, 0);
  std::vector<uint32_t> fb((size_t)h * Ww, 0u);
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x)
      if (cells[(size_t)y * w + x] != '@') {
        c->h_nbmask[(size_t)y * w + x] = NB_FREE;
        fb[(size_t)y * Ww + (x >> 5)] |= 1u << (x & 31u);
      }
  auto is_free = [&](long x, long y) {
    return x >= 0 && y >= 0 && x < (long)w && y < (long)h && cells[(size_t)y * w + x] != '@';
  };
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      uint8_t& m = c->h_nbmask[(size_t)y * w + x];
      if (!(m & NB_FREE)) continue;
      if (is_free(x, (long)y + 1)) m |= 1;
      if (is_free((long)x + 1, y)) m |= 2;
      if (is_free(x, (long)y - 1)) m |= 4;
      if (is_free((long)x - 1, y)) m |= 8;
    }
  if (!upload(c->d_nbmask, c->h_nbmask, "nbmask") || !upload(c->d_freebits, fb, "freebits")) return nullptr;
  c->G.nbmask = c->d_nbmask;
  c->G.freebits = c->d_freebits;
  {
    // k_bfs_wave layout: word (r, cw) at (r + 1) * Wp + cw, zero guard column and rows
    c->Wp = Ww + 1u;
    c->npw = bfs_wave_npw(w, h);  // (h + 2) * Wp
    std::vector<uint32_t> frp(c->npw, 0u);
    for (uint32_t y = 0; y < h; ++y)
      for (uint32_t cw = 0; cw < Ww; ++cw) frp[(size_t)(y + 1u) * c->Wp + cw] = fb[(size_t)y * Ww + cw];
    if (!upload(c->d_frp, frp, "frp")) return nullptr;
    // k_bfs_blk layout: block (bx, by) at (by + 1) * Bp + bx, zero guard block column and rows
    c->BW = (w + 7u) / 8u;
    c->BH = (h + 7u) / 8u;
    c->Bp = c->BW + 1u;
    c->nbp = bfs_blk_nbp(w, h);  // (BH + 2) * Bp
    std::vector<uint64_t> frb(c->nbp, 0ull);
    for (uint32_t y = 0; y < h; ++y)
      for (uint32_t x = 0; x < w; ++x)
        if (c->h_nbmask[(size_t)y * w + x] & NB_FREE)
          frb[(size_t)((y >> 3) + 1u) * c->Bp + (x >> 3)] |= 1ull << (((y & 7u) << 3) | (x & 7u));
    // run starts (free cells whose west is blocked or x % 32 == 0) numbered in block order
    std::vector<uint32_t> abase(c->nbp, 0u);
    uint64_t nrs = 0;
    for (uint32_t p = 0; p < c->nbp; ++p) {
      const uint32_t bx = p % c->Bp;
      const uint64_t f = frb[p], fw = p ? frb[p - 1u] : 0ull;
      const uint64_t col0 = 0x0101010101010101ull;
      const uint64_t wf = ((f << 1) & ~col0) | ((bx & 3u) ? ((fw >> 7) & col0) : 0ull);
      abase[p] = (uint32_t)nrs;
      nrs += (uint64_t)__builtin_popcountll(f & ~wf);
    }
    c->nrs = (uint32_t)nrs;
    uint64_t nf = 0;
    for (uint32_t p = 0; p < c->nbp; ++p) nf += (uint64_t)__builtin_popcountll(frb[p]);
    c->nfree = (uint32_t)std::min<uint64_t>(nf, 0xFFFFFFFFull);
    if (!upload(c->d_abase, abase, "abase") || !upload(c->d_frb, frb, "frb")) return nullptr;
  }
  c->h_goal_tab.assign(ncell, -1);
  if (!upload(c->d_goal_tab, c->h_goal_tab, "goal_tab")) return nullptr;
  constexpr unsigned MAPPED = hipHostMallocCoherent | hipHostMallocMapped;
  if ((e = c->d_stat.alloc(1)) != hipSuccess) return fail("malloc status", e);
  if ((e = hipMemsetAsync(c->d_stat, 0, sizeof(DevStatus), c->s)) != hipSuccess) return fail("memset status", e);
  if ((e = c->h_stat.alloc(1)) != hipSuccess) return fail("pinned status", e);
  if ((e = c->d_ctl.alloc(1)) != hipSuccess) return fail("malloc ctl", e);
  if ((e = c->d_pargs.alloc(1)) != hipSuccess) return fail("malloc plan args", e);
  if ((e = c->d_ticks.alloc(TK_COUNT)) != hipSuccess) return fail("malloc ticks", e);
  if ((e = hipMemsetAsync(c->d_ticks, 0, TK_COUNT * sizeof(unsigned long long), c->s)) != hipSuccess)
    return fail("memset ticks", e);
  hipDeviceGetAttribute(&c->wall_khz, hipDeviceAttributeWallClockRate, c->device);
  if (c->wall_khz <= 0) c->wall_khz = 100000;
  if ((e = c->h_ctl.alloc(1)) != hipSuccess) return fail("pinned ctl", e);
  if ((e = c->h_flags.alloc(HF_WORDS, MAPPED)) != hipSuccess) return fail("pinned flags", e);
  if ((e = c->h_flags.map()) != hipSuccess) return fail("flags device pointer", e);
  if (c->host_threads) {
    uint32_t ring = HOST_RING_ENTRIES;
    if (c->tun.host_ring) {
      ring = 8u;
      while (ring * 2u <= c->tun.host_ring) ring *= 2u;
    }
    c->hring = ring;
    if ((e = c->h_hreq.alloc(ring, MAPPED)) != hipSuccess) return fail("pinned request ring", e);
    if ((e = c->h_hreq.map()) != hipSuccess) return fail("request ring device pointer", e);
    if ((e = c->h_hrep.alloc(ring, MAPPED)) != hipSuccess) return fail("pinned reply ring", e);
    if ((e = c->h_hrep.map()) != hipSuccess) return fail("reply ring device pointer", e);
    // the serving threads' scratch is sized here, so nothing allocates (or throws) while a dispatch runs
    try {
      c->host_scratch.resize(c->host_threads);
      for (HostAstar& S : c->host_scratch) {
        S.gs.assign(ncell, 0u);
        S.heap.resize(4u * (size_t)ncell + 8u);
      }
    } catch (const std::bad_alloc&) {
      return fail("host A* scratch", hipErrorOutOfMemory);
    }
  }
  memset(c->h_stat, 0, sizeof(DevStatus));
  size_t freeb = 0, totalb = 0;
  hipMemGetInfo(&freeb, &totalb);
  c->table_budget = (opts && opts->table_budget_bytes) ? opts->table_budget_bytes : (uint64_t)(freeb / 2);
  if ((e = hipStreamSynchronize(c->s)) != hipSuccess) return fail("stream sync", e);
  return c;
}

void tsw_destroy(tsw_ctx* c) { delete c; }

const char* tsw_last_error(const tsw_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int tsw_abi_version(void) { return TSW_ABI_VERSION; }

uint64_t tsw_build_id(void) { return (uint64_t)TSW_SRC_HASH; }

int tsw_get_stats(const tsw_ctx* c, tsw_stats* out) {
  if (!c || !out) return TSW_EINVAL;
  tsw_ctx* cc = const_cast<tsw_ctx*>(c);
  resolve_timing(cc);
  unsigned long long ticks[TK_SECTIONS] = {0};
  if (hipSetDevice(c->device) == hipSuccess && hipStreamSynchronize(c->s) == hipSuccess)
    (void)hipMemcpy(ticks, c->d_ticks, sizeof ticks, hipMemcpyDeviceToHost);
  *out = c->st;
  out->tables = c->tab_live;
  out->table_evictions = c->evictions;
  for (int k = 0; k < TK_SECTIONS; ++k) out->plan_section_ms[k] = (double)ticks[k] / (double)c->wall_khz;
  return TSW_OK;
}

int tsw_reset_stats(tsw_ctx* c) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  resolve_timing(c);
  const uint64_t tabs = c->st.tables;
  c->st = tsw_stats{};
  c->st.tables = tabs;
  if (c->d_ticks) (void)hipMemsetAsync(c->d_ticks, 0, TK_COUNT * sizeof(unsigned long long), c->s);
  return TSW_OK;
}

int tsw_set_timing(tsw_ctx* c, int enabled) {
  if (!c) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  resolve_timing(c);
  c->timing = enabled != 0;
  return TSW_OK;
}

int tsw_probe_round_floors(tsw_ctx* c, uint32_t block, double* out) {
  if (!c || !out) return TSW_EINVAL;
  NOT_FROM_RESOLVER(c);
  if (block == 0) block = c->st.plan_block ? c->st.plan_block : PLAN_BLOCK_MAX;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->s));
  HIPCHK(probe_round_floors(block, std::max<uint32_t>(c->acap ? (uint32_t)c->acap : 1024u, 64u), c->s, &out[0],
                            &out[1]));
  return TSW_OK;
}

}  // extern "C"
