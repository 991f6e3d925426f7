// Stand-alone driver for the placement and kernel-choice rules (csrc/tsw_place.h): which k_plan instantiation,
// worker layout and K1 kernel a grid, fleet, LDS size and CU count get. Built with the host compiler alone — no
// HIP, no device — under ASan + UBSan by tests/test_place.py. Three parts: (a) the planner placements that
// profiles/r16/gpu_tests.txt and profiles/r17/placement_parent.txt record from an MI355X, to the byte; (b) the
// worker layouts and K1 choices the repository records; (c) properties over a sweep of grids, fleets, LDS sizes
// and CU counts. Exits non-zero when a case fails.
#include <chrono>
#include <cstdint>
#include <cstdio>

#include "tsw_place.h"

using namespace tsw;

static int fails = 0;
static long checks = 0;

#define CHECK(cond, ...)             \
  do {                               \
    ++checks;                        \
    if (!(cond)) {                   \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);      \
      std::printf("\n");             \
      ++fails;                       \
    }                                \
  } while (0)

constexpr int MI355X_LDS = 163840;  // hipDeviceAttributeMaxSharedMemoryPerBlock there
constexpr int MI355X_CUS = 256;

static DevGrid grid(uint32_t W, uint32_t H) { return DevGrid{W, H, W * H, (W + 31u) / 32u, nullptr, nullptr}; }

static BfsGeom geom(uint32_t W, uint32_t H, uint32_t nfree) {
  return BfsGeom{W, H, W * H, nfree, bfs_wave_npw(W, H), bfs_blk_nbp(W, H)};
}

static BfsKnobs knobs(uint32_t mode = 0, uint32_t pair = 0, uint32_t wls = 0) {
  return BfsKnobs{mode, 576u, 512u, 16u, wls, pair};  // the Tunables defaults (tsw_ctx.h)
}

// ---- (a) measured planner placements ---------------------------------------------------------------------------
static void planner_pins() {
  struct Row {
    uint32_t n, W, H, mask;
    bool agents;
    uint32_t part;
    bool flinks, occ, mu;
    size_t bytes;
    int variant;
  };
  const Row rows[] = {
      // profiles/r16/gpu_tests.txt (the parity tests' placement lines)
      {400, 170, 84, 0x7F, true, 0, false, true, true, 131184, 0},
      {1000, 150, 150, 0x7F, true, 0, false, true, false, 126176, 1},
      {1000, 200, 200, 0x7F, true, 0, false, false, false, 36176, 2},
      {6000, 128, 128, 0x3F, false, 0x3F, true, false, false, 142128, 3},
      {6000, 100, 100, 0, false, 0, true, true, true, 132128, 4},
      {6000, 128, 128, 0, false, 0, true, true, false, 117664, 5},
      {6000, 128, 128, 0x3, false, 0x3, true, true, false, 147664, 5},
      {6000, 128, 128, 0x7F, false, 0x7F, false, false, false, 118096, 6},
      // profiles/r17/placement_parent.txt (C3, wh10k, C5). C3's 150,416 B are its placement's own bytes, plan_lds_bytes for
      // 1,000 agents on 170x84 (4,096 + 32,080 + 114,240); the coop dispatch's request (D->lds, setup_dispatch) is 161,792 B
      {1000, 170, 84, 0x7F, true, 0, false, true, true, 150416, 0},
      {10000, 510, 220, 0x7F, false, 0x3F, false, false, false, 154096, 3},
      {10000, 1024, 1024, 0x7F, false, 0x3F, false, false, false, 154096, 3},
  };
  for (const Row& r : rows) {
    const PlanPlacement p = choose_plan_placement(r.n, r.W * r.H, 0u, MI355X_LDS, r.mask, true, true);
    const size_t b = plan_lds_bytes(r.n, r.W * r.H, 0u, p);
    CHECK(p.agents == r.agents && p.part == r.part && p.flinks == r.flinks && p.occ == r.occ && p.mu == r.mu && !p.tasks,
          "n %u %ux%u mask 0x%x: agents %d part 0x%x flinks %d occ %d mu %d tasks %d", r.n, r.W, r.H, r.mask, p.agents,
          p.part, p.flinks, p.occ, p.mu, p.tasks);
    CHECK(b == r.bytes, "n %u %ux%u mask 0x%x: %zu B, recorded %zu", r.n, r.W, r.H, r.mask, b, r.bytes);
    CHECK(plan_variant(p) == r.variant, "n %u %ux%u mask 0x%x: variant %d, recorded %d", r.n, r.W, r.H, r.mask,
          plan_variant(p), r.variant);
  }
  // the last parameter (agents_on, Tunables::agents_lds) defaults to true: leaving it out and passing true give every
  // recorded placement above
  auto same = [](const PlanPlacement& a, const PlanPlacement& b) {
    return a.agents == b.agents && a.occ == b.occ && a.mu == b.mu && a.flinks == b.flinks && a.tasks == b.tasks && a.part == b.part;
  };
  for (const Row& r : rows) {
    const PlanPlacement d = choose_plan_placement(r.n, r.W * r.H, 0u, MI355X_LDS, r.mask, true, true);
    const PlanPlacement t = choose_plan_placement(r.n, r.W * r.H, 0u, MI355X_LDS, r.mask, true, true, true);
    CHECK(same(d, t) && plan_variant(t) == r.variant, "n %u %ux%u mask 0x%x: agents_on = true gives variant %d, the default %d",
          r.n, r.W, r.H, r.mask, plan_variant(t), plan_variant(d));
  }
  // the three placements of tests/test_gpu_rules.py, at the fleets and grids of tests/rules_cases.py:
  //   ag      no knob                                   -> k_plan<true, true, true, false>   (0)
  //   global  TSW_AGENTS_LDS=0 TSW_PART_LDS=0x7F        -> k_plan<false, true, true, false>  (4): the arrays admitted one by one
  //   pg      TSW_AGENTS_LDS=0 TSW_PART_LDS=0x3F, a case in the corner of a blocked 208x208 map: 43,264 cells x 4 B of OCC
  //           do not fit beside the parts                -> k_plan<false, false, false, true> (3)
  struct Small {
    uint32_t n, W, H;
  };
  // every (fleet, grid) of tests/rules_cases.py. tests/test_rules_cases.py::test_place_rows_cover_every_case reads this
  // initialiser and the `for (uint32_t n : {` list below from the source text: keep the two literals' form when editing
  const Small small[] = {{2, 64, 1},     {4, 2, 2},      {10, 4, 3},     {16, 16, 1},    {16, 40, 24},   {17, 17, 1},   {17, 19, 1},
                         {18, 18, 1},    {18, 20, 1},    {19, 21, 1},    {21, 40, 24},   {22, 64, 6},    {60, 14, 10},  {62, 17, 16},
                         {62, 64, 3},    {63, 14, 10},   {64, 17, 17},   {64, 64, 1},    {64, 64, 3},    {65, 65, 1},   {66, 18, 17},
                         {66, 64, 5},    {66, 66, 1},    {69, 14, 10},   {71, 80, 24},   {128, 33, 33},  {131, 131, 1}, {248, 34, 34},
                         {1024, 64, 63}, {1026, 64, 65}, {1088, 64, 22}, {1088, 64, 36}};
  for (const Small& c : small) {
    const PlanPlacement ag = choose_plan_placement(c.n, c.W * c.H, 0u, MI355X_LDS, 0x7Fu, true, true);
    CHECK(ag.agents && ag.part == 0u && plan_variant(ag) == 0, "ag, n %u %ux%u: variant %d", c.n, c.W, c.H, plan_variant(ag));
    const PlanPlacement gl = choose_plan_placement(c.n, c.W * c.H, 0u, MI355X_LDS, 0x7Fu, true, true, false);
    CHECK(!gl.agents && gl.part == 0x7Fu && gl.flinks && gl.occ && gl.mu && plan_variant(gl) == 4,
          "global, n %u %ux%u: part 0x%x occ %d mu %d variant %d", c.n, c.W, c.H, gl.part, gl.occ, gl.mu, plan_variant(gl));
  }
  for (uint32_t n : {4u, 10u, 22u, 62u, 64u, 66u, 128u, 1088u}) {
    const PlanPlacement pg = choose_plan_placement(n, 208u * 208u, 0u, MI355X_LDS, 0x3Fu, true, true, false);
    CHECK(!pg.agents && pg.part == PART_PG && pg.flinks && !pg.occ && !pg.mu && plan_variant(pg) == 3,
          "pg, n %u on 208x208: part 0x%x occ %d variant %d", n, pg.part, pg.occ, plan_variant(pg));
    // with the agent arrays allowed in LDS the same fleet is an AG placement: the knob alone reaches PG at this size
    CHECK(choose_plan_placement(n, 208u * 208u, 0u, MI355X_LDS, 0x3Fu, true, true).agents, "n %u on 208x208 without the knob", n);
  }
  CHECK(plan_lds_bytes(400, 170 * 84, 0, true, true, false) == 4096u + 12848u + 114240u, "the first row by hand");
  CHECK(MI355X_LDS - PLAN_LDS_RESERVE == 161792, "budget");
}

// ---- (b) recorded worker layouts and K1 choices ----------------------------------------------------------------
static void recorded_pins() {
  // the [k_plan] workers: lines of profiles/r17/placement_parent.txt; DESIGN.md's K3 worker table has the same counts
  struct Row {
    const char* name;
    uint32_t W, H, n, nworkers, wpb, gs, hcap, dag, lds_per_wave;
  };
  const Row rows[] = {
      {"C3", 170, 84, 1000, 1020, 4, 2, 1232, 1, 40448},
      {"wh10k", 510, 220, 10000, 1275, 5, 0, 2048, 2, 30464},
      {"C5", 1024, 1024, 10000, 2295, 9, 0, 2048, 2, 16384},
  };
  for (const Row& r : rows) {
    // a coop dispatch: the planner block asks for the whole budget, 1,024 threads at these fleet sizes
    const size_t lds = (size_t)(MI355X_LDS - PLAN_LDS_RESERVE);
    const WorkerCfg c = worker_config(grid(r.W, r.H), MI355X_CUS, r.n, 0u, -1, true, lds, -1);
    const WorkerLayout L = worker_layout(c.lds, lds, 1024u, MI355X_CUS);
    CHECK(L.nworkers(4096u) == r.nworkers && L.want == r.nworkers && L.wpb == r.wpb && c.gs_lds == r.gs && c.hcap == r.hcap && c.dag == r.dag &&
              L.lds_per_wave == r.lds_per_wave,
          "%s: %u waves (%u per workgroup), g-scores %u, heap %u, DAG exit %u, %u B each", r.name, L.want, L.wpb,
          c.gs_lds, c.hcap, c.dag, L.lds_per_wave);
    CHECK(L.wblocks(4096u) == MI355X_CUS - 1u, "%s: %u worker workgroups", r.name, L.wblocks(4096u));
  }
  // never more workers than scratch slots; nothing when a worker's carve does not fit the dispatch's LDS
  CHECK(worker_layout(16384, 161792, 1024, 256).nworkers(100) == 100u, "slots cap the workers");
  CHECK(worker_layout(16384, 161792, 1024, 256).wblocks(100) == 12u, "100 workers in groups of 9");
  CHECK(worker_layout(200000, 161792, 1024, 256).want == 0u, "no worker fits");
  CHECK(worker_layout(0, 161792, 1024, 256).wblocks(4096) == 0u, "no carve, no worker");
  CHECK(worker_layout(16384, 161792, 1024, 1).want == 0u, "one CU: the planner's");

  // 200x130: H * Ww = 910 words is no multiple of 4; the staged bitmap is padded to 16 bytes (3,640 -> 3,648),
  // so byte g-scores (26,000) + bitmap + detour bytes (26,000) leave every slice 16-byte aligned
  {
    const WorkerCfg c = worker_config(grid(200, 130), MI355X_CUS, 100u, 0u, -1, true, 161792, -1);
    CHECK(c.gs_lds == 2u && c.stage_fb == 1u && c.dag == 1u, "200x130: g-scores %u fb %u dag %u", c.gs_lds, c.stage_fb, c.dag);
    CHECK(c.lds - (size_t)c.hcap * 8u == 26000u + 3648u + 26000u, "200x130: rest %zu", c.lds - (size_t)c.hcap * 8u);
    CHECK((c.lds - (size_t)c.hcap * 8u) % 16u == 0u, "200x130: rest not a multiple of 16");
  }

  // K1: den520d (256x257, 28,178-odd free cells: the count plays no part outside mg) takes k_bfs_blk, 1024x1024 k_bfs_big
  for (int mg = 0; mg < 2; ++mg) {
    const BfsChoice d = choose_bfs(geom(256, 257, 28000), knobs(), MI355X_LDS, MI355X_CUS, mg != 0);
    CHECK(d.kernel == BFS_BLK && d.fits && d.waves_per_block >= 1u && !d.pair && d.cap == 576u, "den520d: kernel %u fits %d waves %u",
          d.kernel, d.fits, d.waves_per_block);
    const BfsChoice b = choose_bfs(geom(1024, 1024, 1u << 20), knobs(), MI355X_LDS, MI355X_CUS, mg != 0);
    CHECK(b.kernel == BFS_BIG && b.fits, "1024x1024: kernel %u fits %d", b.kernel, b.fits);
  }
  // the `wide` map of tests/test_gpu_limits.py (2048x33): mg's carve is 169,412 B against 163,840; the V term's
  // (W + 2) * (H + 2) * 2 = 143,500 B, rounded up to 16, are most of it
  CHECK(mg_vbytes(2048, 33) == 143504u, "wide: V term %u", mg_vbytes(2048, 33));
  CHECK(bfs_mg_lds_bytes(2048, 33, bfs_blk_nbp(2048, 33)) == 169412u, "wide: %zu B", bfs_mg_lds_bytes(2048, 33, bfs_blk_nbp(2048, 33)));
  {
    const BfsChoice w = choose_bfs(geom(2048, 33, 40000), knobs(5), MI355X_LDS, MI355X_CUS, true);
    CHECK(w.kernel == BFS_MG && !w.fits, "wide, forced mg: kernel %u fits %d", w.kernel, w.fits);
    // `over`: 65,536 free cells are one too many for u16 levels, whatever the carve
    const BfsChoice o = choose_bfs(geom(256, 257, 65536), knobs(5), 1 << 30, MI355X_CUS, true);
    CHECK(o.kernel == BFS_MG && !o.fits, "65,536 free cells, forced mg: fits %d", o.fits);
    const BfsChoice f = choose_bfs(geom(256, 257, 65535), knobs(5), MI355X_LDS, MI355X_CUS, true);
    CHECK(f.kernel == BFS_MG && f.fits, "den520d-sized, forced mg: fits %d", f.fits);
  }
  CHECK(bp_magic(33) == 130150525u && bp_magic(257) == 16711936u, "bp_magic: ceil(2^32 / Bp)");
  CHECK(CU_LDS_BYTES == 163840u, "CU LDS");
}

// ---- (c) properties over a sweep --------------------------------------------------------------------------------
struct WH {
  uint32_t W, H;
};
static const WH GRIDS[] = {{1, 1},     {7, 7},     {8, 8},       {9, 9},       {31, 31},    {32, 32},   {33, 33},  {64, 64},
                           {170, 84},  {256, 257}, {1000, 1000}, {1024, 1024}, {2048, 512}, {2048, 1},  {1, 2048}};
static const uint32_t AGENTS[] = {1, 64, 65, 400, 6000, 65534, 65535};
static const int LDS[] = {65536, 163840};
static const int CUS[] = {1, 256};

static void sweep_planner() {
  for (const WH& g : GRIDS)
    for (uint32_t n : AGENTS)
      for (int max_lds : LDS)
        for (uint32_t mask : {0x7Fu, 0x3Fu, 0x3u, 0u})
          for (int fl = 0; fl < 2; ++fl)
            for (int sp = 0; sp < 2; ++sp) {
              const uint32_t ncell = g.W * g.H;
              const PlanPlacement p = choose_plan_placement(n, ncell, 3u * n, max_lds, mask, fl != 0, sp != 0);
              // agents_on: true is the default; false never places the whole set and still fits
              const PlanPlacement pt = choose_plan_placement(n, ncell, 3u * n, max_lds, mask, fl != 0, sp != 0, true);
              const PlanPlacement pf = choose_plan_placement(n, ncell, 3u * n, max_lds, mask, fl != 0, sp != 0, false);
              CHECK(pt.agents == p.agents && pt.part == p.part && pt.occ == p.occ && pt.mu == p.mu && pt.flinks == p.flinks,
                    "n %u %ux%u: agents_on = true differs from the default", n, g.W, g.H);
              CHECK(!pf.agents && (pf.part & ~mask) == 0u && plan_lds_bytes(n, ncell, 3u * n, pf) <= (size_t)(max_lds - PLAN_LDS_RESERVE),
                    "n %u %ux%u mask 0x%x, agents_on = false: agents %d part 0x%x", n, g.W, g.H, mask, pf.agents, pf.part);
              const size_t budget = (size_t)(max_lds - PLAN_LDS_RESERVE);
              const int v = plan_variant(p);
              CHECK(plan_lds_bytes(n, ncell, 3u * n, p) <= budget, "n %u %ux%u lds %d mask 0x%x: %zu B over %zu", n, g.W, g.H,
                    max_lds, mask, plan_lds_bytes(n, ncell, 3u * n, p), budget);
              CHECK(!p.mu || p.occ, "mu without occ");
              CHECK(!p.mu || n < 65535u, "mu with %u agents", n);
              CHECK(v >= 0 && v <= 6, "variant %d", v);
              CHECK(!(p.part == PART_PG && !p.occ && !p.agents) || v == 3, "PART_PG alone is variant %d", v);
              CHECK((p.part & ~mask) == 0u && (!p.agents || p.part == 0u) && (!p.flinks || (fl && !p.agents)) && !p.tasks,
                    "part 0x%x mask 0x%x agents %d flinks %d", p.part, mask, p.agents, p.flinks);
            }
}

static void sweep_workers() {
  for (const WH& g : GRIDS)
    for (uint32_t n : AGENTS)
      for (int num_cu : CUS)
        for (size_t lds_cap : {(size_t)(65536 - PLAN_LDS_RESERVE), (size_t)(163840 - PLAN_LDS_RESERVE), (size_t)163840})
          for (int dag = 0; dag < 2; ++dag)
            for (int gs = -1; gs <= 2; ++gs)
              for (int fb = -1; fb <= 1; ++fb)
                for (uint32_t want : {0u, 64u, 5000u}) {
                  const DevGrid G = grid(g.W, g.H);
                  const WorkerCfg c = worker_config(G, num_cu, n, want, gs, dag != 0, lds_cap, fb);
                  // the carve as coop_worker lays it out: heap, g-scores, padded bitmap, detour bytes
                  const size_t pad16 = ((size_t)G.ncell + 15u) / 16u * 16u;
                  const size_t rest = (c.gs_lds == 1u ? (size_t)G.ncell * 4u : c.gs_lds == 2u ? pad16 : 0u) +
                                      (c.stage_fb ? ((size_t)G.H * G.Ww * 4u + 15u) / 16u * 16u : 0u) + (c.dag == 1u ? pad16 : 0u);
                  CHECK(c.gs_lds == 0u || c.stage_fb == 1u, "%ux%u: LDS g-scores without the staged bitmap", g.W, g.H);
                  CHECK(c.lds == (size_t)c.hcap * 8u + rest, "%ux%u n %u gs %d fb %d: lds %zu, heap %u + rest %zu", g.W, g.H, n, gs, fb,
                        c.lds, c.hcap, rest);
                  CHECK(c.waves <= (uint32_t)num_cu * 16u, "%u waves on %d CUs", c.waves, num_cu);
                  CHECK(c.lds * (c.waves / (uint32_t)num_cu) <= lds_cap, "%ux%u: %u waves of %zu B over %zu", g.W, g.H,
                        c.waves / (uint32_t)num_cu, c.lds, lds_cap);
                  CHECK(c.hcap >= 64u && c.hcap <= WAVE_HCAP, "%ux%u: heap %u", g.W, g.H, c.hcap);
                  CHECK(c.dag == (dag ? (c.gs_lds ? 1u : 2u) : 0u), "dag %u", c.dag);
                }
}

// LDS bytes of the launch a choice describes, from the carve sizes
static size_t choice_lds(const BfsGeom& g, const BfsKnobs& t, const BfsChoice& ch) {
  switch (ch.kernel) {
    case BFS_MG: return bfs_mg_lds_bytes(g.W, g.H, g.nbp);
    case BFS_BLK:
      return (size_t)blk_shared_u64(g.nbp) * 8u + (size_t)ch.waves_per_block * (ch.pair ? 2u : 1u) * 4u *
                                                      blk_bfs_words(g.nbp, 1u << bfs_blk_klog(g.nbp), ch.cap, t.wls != 0u);
    case BFS_WAVE:
      return (size_t)((g.npw + 3u) & ~3u) * 4u +
             (size_t)ch.waves_per_block * 4u * wave_bfs_words(g.npw, 1u << bfs_wave_klog(g.npw), ch.cap);
    case BFS_BIG: return big_bfs_lds(g.nbp, ch.cap);
    case BFS_BLOCK: return bfs_lds_bytes(g.H, (g.W + 31u) / 32u, g.ncell, false);
  }
  return ~(size_t)0;
}

static void sweep_bfs() {
  const BfsKernel forced[6] = {BFS_BLOCK, BFS_WAVE, BFS_BLOCK, BFS_BLK, BFS_BIG, BFS_MG};  // by TSW_BFS_KERNEL mode
  for (const WH& g : GRIDS)
    for (int max_lds : LDS)
      for (int num_cu : CUS)
        for (uint32_t mode = 0; mode <= 5; ++mode)
          for (uint32_t pair = 0; pair < 2; ++pair)
            for (uint32_t wls = 0; wls < 2; ++wls)
              for (int mg = 0; mg < 2; ++mg)
                for (int half = 0; half < 2; ++half) {
                  const BfsGeom G = geom(g.W, g.H, half ? (g.W * g.H + 1u) / 2u : g.W * g.H);
                  const BfsKnobs t = knobs(mode, pair, wls);
                  const BfsChoice ch = choose_bfs(G, t, max_lds, num_cu, mg != 0);
                  CHECK(ch.kernel <= BFS_BLOCK, "kernel %u", ch.kernel);
                  if (ch.fits) {
                    CHECK(choice_lds(G, t, ch) <= (size_t)max_lds, "%ux%u mode %u lds %d: kernel %u carves %zu B", g.W, g.H, mode,
                          max_lds, ch.kernel, choice_lds(G, t, ch));
                    if (ch.kernel == BFS_BLK || ch.kernel == BFS_WAVE)
                      CHECK(ch.waves_per_block >= 1u && ch.waves_per_block <= 16u, "%u waves per workgroup", ch.waves_per_block);
                    CHECK(ch.kernel != BFS_BLK || G.nbp <= 0x10000u, "blk with %u blocks", G.nbp);
                    CHECK(ch.kernel != BFS_WAVE || G.npw <= 0x8000u, "wave with %u words", G.npw);
                    CHECK(ch.kernel != BFS_BIG || G.nbp <= 0xFFFFu, "big with %u blocks", G.nbp);
                    CHECK(ch.kernel != BFS_MG || (G.nfree <= 0xFFFFu && G.nbp <= 0xFFFFu), "mg with %u free cells", G.nfree);
                    CHECK(!ch.pair || (ch.kernel == BFS_BLK && pair), "pair");
                  }
                  // a forced mode takes its kernel or reports it; the default mode falls through to k_bfs, never to mg
                  if (mode != 0u) CHECK(ch.kernel == forced[mode], "mode %u: kernel %u", mode, ch.kernel);
                  if (mode == 0u) CHECK(ch.kernel != BFS_MG && (ch.fits || ch.kernel == BFS_BLOCK), "default: kernel %u fits %d", ch.kernel, ch.fits);
                  CHECK(mg || !(ch.kernel == BFS_MG && ch.fits), "mg selected in a library without it");
                }
}

int main() {
  const auto t0 = std::chrono::steady_clock::now();
  planner_pins();
  recorded_pins();
  const long pinned = checks;
  sweep_planner();
  sweep_workers();
  sweep_bfs();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("%ld pins, %ld sweep checks, %.0f ms\n", pinned, checks - pinned, ms);
  // the rules are arithmetic on a handful of numbers: milliseconds here, sanitizers included; a second is generous
  CHECK(ms < 1000.0, "pins and sweep took %.0f ms", ms);
  if (fails) {
    std::printf("%d FAILED\n", fails);
    return 1;
  }
  std::printf("place ok\n");
  return 0;
}
