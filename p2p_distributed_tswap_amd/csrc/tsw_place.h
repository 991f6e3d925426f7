// tsw_place.h — what runs where: the LDS placement and kernel-choice rules of the host runtime as plain
// functions of numbers (grid, fleet, LDS size, CU count). Plain C++17, no HIP include: the host runtime,
// the kernels' launchers and a stand-alone CPU program (tests/host/place_main.cpp, tests/test_place.py)
// compile the same text. A function marked TSW_HD sizes an LDS carve: the kernel that carves and the
// host's fit test both call it, and the "must match the carve" comments stay at the carve.
//
//   planner   plan_lds_bytes, choose_plan_placement, plan_variant   (k_plan, tsw_plan_kernel.h)
//   workers   worker_config, worker_layout, the k_astar_wave sizes  (tsw_worker.h, tsw_astar.hip)
//   K1        the five kernels' carve sizes and fit tests, choose_bfs (tsw_bfs*.hip, run_bfs)
//   K8        the task timeline's tiles, workgroups and LDS share     (tsw_timeline.hip)
//   K9        the space-time A*'s waves, LDS heap and staged bitmap  (tsw_st_astar.hip)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "tsw_internal.h"

namespace tsw {

constexpr uint32_t CU_LDS_BYTES = 160u * 1024u;  // LDS of one gfx950 CU

// ---- planner: what of k_plan's state lives in LDS ---------------------------------------------------
// Agent arrays that go to LDS one by one when all of them do not fit (PlanArgs::part_lds), in the
// order the host admits them: the rules phase's successor chains and labels first (its relabel walks
// and firing scans are serial dependent loads), then cells and goals, then the code caches.
enum : uint32_t {
  PART_SUCC = 1u, PART_ONC = 2u, PART_V = 4u, PART_G = 8u, PART_NHC = 16u, PART_CANDC = 32u, PART_GT = 64u,
  PART_PG = 0x3Fu,  // the subset k_plan<false, *, *, true> carves unconditionally (LDS-typed accesses)
};

// the planner's dynamic LDS stays this far below the device's per-workgroup LDS: the placement's budget
// and the coop dispatch's whole-CU request (setup_dispatch) both subtract it
constexpr int PLAN_LDS_RESERVE = 2048;

inline size_t part_lds_bytes(uint32_t n, uint32_t part) {
  auto r16 = [](size_t b) { return (b + 15u) & ~(size_t)15u; };
  size_t b = 0;
  for (uint32_t bit : {PART_SUCC, PART_V, PART_G, PART_GT})
    if (part & bit) b += r16((size_t)n * 4);
  for (uint32_t bit : {PART_ONC, PART_NHC, PART_CANDC})
    if (part & bit) b += r16(n);
  return b;
}

// flinks: the pointer-doubling buffers F1/F2 alone in LDS (when the agent arrays are not)
inline size_t plan_lds_bytes(uint32_t n, uint32_t ncell, uint32_t m, bool agents, bool occ, bool tasks,
                             bool flinks = false, bool mu = true, uint32_t part = 0u) {
  auto r16 = [](size_t b) { return (b + 15u) & ~(size_t)15u; };
  size_t b = r16(1024 * 4);
  if (agents) b += 4 * r16((size_t)n * 4) + 3 * r16((size_t)(n + 1) * 4) + 4 * r16(n);
  else {
    b += part_lds_bytes(n, part);
    if (flinks) b += 2 * r16((size_t)(n + 1) * 4);
  }
  if (occ) b += r16((size_t)ncell * 4) + (mu ? r16((size_t)ncell * 4) : 0u);  // MU in LDS: u32 words (MU32)
  if (tasks) b += r16((size_t)((m + 3u) & ~3u) * 4);
  return b;
}

struct PlanPlacement {
  bool agents, occ, mu, flinks, tasks;
  uint32_t part;  // PART_* bits
};

inline size_t plan_lds_bytes(uint32_t n, uint32_t ncell, uint32_t m, const PlanPlacement& p) {
  return plan_lds_bytes(n, ncell, m, p.agents, p.occ, p.tasks, p.flinks, p.mu, p.part);
}

// What of the planner's state lives in LDS, in priority order: agents, occupancy grid, task table.
// part_mask / flinks_on / occ_split / agents_on: Tunables::part_lds / flinks_lds / occ_split / agents_lds
// (agents_on false: the whole set stays out of LDS however small the fleet — diagnostic builds only).
inline PlanPlacement choose_plan_placement(uint32_t n, uint32_t ncell, uint32_t m, int max_lds, uint32_t part_mask,
                                           bool flinks_on, bool occ_split, bool agents_on = true) {
  const size_t budget = (size_t)std::max(max_lds - PLAN_LDS_RESERVE, 0);
  bool ag = agents_on && plan_lds_bytes(n, ncell, m, true, false, false) <= budget;
  // without the whole set, single agent arrays in priority order (PART_*: the rules phase's serial
  // successor walks and firing scans read SUCC / ONC / V / G; wh10k rules 3.9 -> ? s), then the rules
  // relabel's pointer-doubling buffers
  uint32_t part = 0;
  if (!ag)
    for (uint32_t bit : {PART_SUCC, PART_ONC, PART_V, PART_G, PART_NHC, PART_CANDC, PART_GT})
      if ((part_mask & bit) && plan_lds_bytes(n, ncell, m, false, false, false, false, true, part | bit) <= budget)
        part |= bit;
  bool fl = !ag && flinks_on && plan_lds_bytes(n, ncell, m, false, false, false, true, true, part) <= budget;
  // the occupancy grid with the movement rounds' MU words, else OCC alone (every rules round reads
  // OCC: C3's 170x84 fits OCC but not MU beside the agent arrays)
  bool mu = n < 65535u && plan_lds_bytes(n, ncell, m, ag, true, false, fl, true, part) <= budget;  // MU32: 16-bit agent ids
  bool oc = mu || (occ_split && plan_lds_bytes(n, ncell, m, ag, true, false, fl, false, part) <= budget);
  const bool tk = false;  // K4 reads its spatial index from global memory (the chunks it needs only)
  return PlanPlacement{ag, oc, mu, fl, tk, part};
}

// The k_plan<AG, OC, MUL, PG> instantiation of a placement: k is the index of tsw_plan_v<k>.hip. The
// tests stand in this order.
inline int plan_variant(const PlanPlacement& p) {
  const bool mu = p.occ && p.mu;
  if (p.agents && mu) return 0;                    // <true, true, true, false>
  if (p.agents && p.occ) return 1;                 // <true, true, false, false>
  if (p.agents) return 2;                          // <true, false, false, false>
  if (p.part == PART_PG && !p.occ) return 3;       // <false, false, false, true>
  if (mu) return 4;                                // <false, true, true, false>
  if (p.occ) return 5;                             // <false, true, false, false>
  return 6;                                        // <false, false, false, false>
}

// ---- K3: k_astar_lds / k_astar_wave sizes and the coop workers' layout ------------------------------
inline bool astar_lds_ok(const DevGrid& G) { return G.ncell <= 1024u; }

constexpr uint32_t WAVE_HCAP = 4096;              // LDS heap entries (32 KiB)
constexpr uint32_t WAVE_GS_LDS_MAX = 24u * 1024u;   // cells whose u32 g_score words fit LDS beside it
constexpr uint32_t WAVE_GB_LDS_MAX = 120u * 1024u;  // cells whose byte g_scores fit LDS beside it

inline uint32_t wave_gs_mode(const DevGrid& G) {
  return G.ncell <= WAVE_GS_LDS_MAX ? 1u : G.ncell <= WAVE_GB_LDS_MAX ? 2u : 0u;
}

constexpr size_t WAVE_LDS_MAX = CU_LDS_BYTES;

// heap + LDS g_scores + free-cell bitmap (k_astar_wave's carve)
inline size_t wave_lds_bytes(const DevGrid& G, uint32_t hcap, uint32_t m) {
  return (size_t)hcap * 8u + (m == 1u ? (size_t)G.ncell * 4u : m == 2u ? ((size_t)G.ncell + 15u) / 16u * 16u : 0u) +
         (size_t)G.H * G.Ww * 4u;
}

// largest heap (<= want) whose carve fits the 160 KiB of LDS
inline uint32_t wave_fit_hcap(const DevGrid& G, uint32_t want, uint32_t m) {
  const size_t rest = wave_lds_bytes(G, 0, m);
  const size_t room = rest < WAVE_LDS_MAX ? (WAVE_LDS_MAX - rest) / 8u : 0u;
  return (uint32_t)std::min<size_t>(want, room);
}

inline bool astar_wave_lds_gs(const DevGrid& G) { return wave_gs_mode(G) != 0u; }  // k_astar_wave keeps this grid's g_scores in LDS

// waves of a host-launched k_astar_wave pass. global_gs: keep the g_scores in the global slots even when
// the grid's fit LDS (second tier for queries whose byte-encoded g_scores overflowed).
inline uint32_t astar_wave_slots(const DevGrid& G, int num_cu, bool global_gs = false) {
  const uint32_t m = global_gs ? 0u : wave_gs_mode(G);
  const size_t lds = wave_lds_bytes(G, wave_fit_hcap(G, WAVE_HCAP, m), m);
  const uint32_t per_cu = (uint32_t)std::max<size_t>(1, CU_LDS_BYTES / lds);
  return (uint32_t)num_cu * std::min<uint32_t>(per_cu, 16u);
}

// Worker placement: per-wave LDS (heap, g-scores, free bitmap) sets the waves per CU. g-scores stay
// in LDS (fastest per pop) unless that leaves < 3 waves per CU while many agents can need queries at
// once (n > 2000): then they move to the global slots and more waves run.
struct WorkerCfg {
  uint32_t gs_lds, stage_fb, hcap, waves;
  uint32_t dag;  // WorkerArgs::dag
  size_t lds;
};

inline WorkerCfg worker_config(const DevGrid& G, int num_cu, uint32_t n_agents, uint32_t hcap_want, int force_gs = -1,
                               bool dag_exit = true, size_t lds_cap = CU_LDS_BYTES, int force_fb = -1) {
  // the workers' LDS is the plan dispatch's per-workgroup request (the planner's, just under the
  // CU's 160 KiB): every carve below must fit THAT, not the CU (C5's bitmap + heap
  // came to 160 KiB, 2 KiB over the dispatch's request, and no worker fit — exit mode)
  const size_t WAVE_LDS_MAX = std::min<size_t>(lds_cap, ::tsw::WAVE_LDS_MAX);
  // the staged bitmap as coop_worker carves it: padded to 16 bytes, the detour bytes follow it. Unpadded
  // (H * Ww not a multiple of 4, e.g. 200x130) a slice with an odd heap size came out 8 bytes short, and
  // the last cells' detour bytes lay on the next worker's first heap entry
  const size_t fbb = ((size_t)G.H * G.Ww * 4u + 15u) / 16u * 16u;
  const uint32_t want = hcap_want ? std::min(hcap_want, WAVE_HCAP) : WAVE_HCAP;
  // m: g-score placement; fb: free bitmap in LDS. With LDS g-scores the DAG early exit stages the
  // goal's detour bytes in LDS too (its reads then cost what a g-score read costs) and the heap gives
  // up entries past 1,024 for more waves per CU, up to one per SIMD (C3 queries peak below 300
  // entries; an overflowing query is handed to the next tier); with global g-scores it reads the
  // u16 table beside them.
  auto make = [&](uint32_t m, bool fb) {
    WorkerCfg c{};
    c.gs_lds = m;
    c.stage_fb = fb ? 1u : 0u;
    c.dag = !dag_exit ? 0u : m != 0u ? 1u : 2u;
    const size_t gsb = m == 1u ? (size_t)G.ncell * 4u : m == 2u ? ((size_t)G.ncell + 15u) / 16u * 16u : 0u;
    const size_t dtb = c.dag == 1u ? ((size_t)G.ncell + 15u) / 16u * 16u : 0u;
    const size_t rest = gsb + (fb ? fbb : 0u) + dtb;
    c.hcap = rest < WAVE_LDS_MAX ? (uint32_t)std::min<size_t>(want, (WAVE_LDS_MAX - rest) / 8u) : 0u;
    if (c.dag == 1u && c.hcap > 1024u && hcap_want == 0u) {
      const size_t pc = std::min<size_t>(4u, WAVE_LDS_MAX / (rest + 1024u * 8u));
      if (pc >= 1u) c.hcap = (uint32_t)std::min<size_t>(c.hcap, (WAVE_LDS_MAX / pc - rest) / 8u);
    }
    c.lds = (size_t)c.hcap * 8u + rest;
    const uint32_t per_cu = c.lds ? (uint32_t)std::min<size_t>(16u, WAVE_LDS_MAX / c.lds) : 0u;
    c.waves = (uint32_t)num_cu * per_cu;
    return c;
  };
  const uint32_t m = wave_gs_mode(G);
  const bool fits = force_gs == 0 || (force_gs == 1 && G.ncell <= WAVE_GS_LDS_MAX) ||
                    (force_gs == 2 && G.ncell <= WAVE_GB_LDS_MAX);
  if (force_gs >= 0 && fits) {  // A/B: another g-score placement than the default
    // forced global g-scores take TSW_WORKER_FB=0 too (on grids whose default keeps them in LDS the
    // bitmap-less layout is reachable no other way)
    WorkerCfg f = make((uint32_t)force_gs, force_gs != 0 || force_fb != 0);
    if (f.hcap >= 64u) return f;
  }
  WorkerCfg c = make(m, true);
  // u32 LDS g-scores leave one wave per CU on a C3-sized grid; byte g-scores (tier-2 hand-off past a
  // 62-cell detour) run 3x the waves — A* latency is the same, the startup bursts drain faster
  // (C3 plan 585 -> 563 ms once idle workers stopped polling every queue word)
  if (m == 1u) {
    const WorkerCfg c2 = make(2u, true);
    if (c2.hcap >= 64u && c2.waves >= 2u * c.waves) c = c2;
  }
  // grids whose byte g-scores fit LDS (<= 120k cells): with many agents, trade the LDS g-scores for
  // 3x the waves (global u32 slots, L2-resident at this size)
  if (m != 0u && n_agents > 2000u && c.waves < 3u * (uint32_t)num_cu) c = make(0u, true);
  if (c.hcap < 64u) c = make(0u, false);
  // global g-score workers: the staged free bitmap saves one L2 read per relaxation but costs LDS; drop
  // it when that at least doubles the waves per CU (C5's 128 KiB bitmap left one wave per CU: plan
  // 8.6 s with 255 workers, 3.97 s with 910 without it, planner sections unchanged — round 4,
  // profiles/r4/c5_workers_ab.jsonl; round 3 measured the opposite in exit mode, before the coop
  // workers stopped with the planner). TSW_WORKER_FB=0 / 1 forces either.
  if (c.gs_lds == 0u && c.stage_fb != 0u && force_fb != 1) {
    const WorkerCfg nf = make(0u, false);
    if (nf.hcap >= 64u && (force_fb == 0 || nf.waves >= 2u * c.waves)) c = nf;
  }
  // heap-only workers (the bitmap-less global-g-score case, C5's 2^20 cells): a 2,048-entry LDS heap
  // doubles the waves per CU — C5 3.64-3.67 s with 1,020 workers -> 3.44-3.51 s with 2,295, no query
  // outgrowing it (profiles/r4/c5_slots_ab.txt); a larger heap would go to the global tier-3 heap
  if (c.gs_lds == 0u && c.stage_fb == 0u && hcap_want == 0u && c.hcap > 2048u) {
    const uint32_t h = 2048u;
    c.hcap = h;
    c.lds = (size_t)h * 8u;
    c.waves = (uint32_t)num_cu * (uint32_t)std::min<size_t>(16u, WAVE_LDS_MAX / c.lds);
  }
  // global g-score workers that keep the staged bitmap (wh10k's 112k cells: 14 KiB of bitmap): a 2,048-entry
  // heap too when that raises the waves per CU by half or more — round 5, busy wh10k: 765 -> 1,275 workers,
  // 11.07-11.13 -> 10.55 s, no query outgrowing the heap (profiles/r5/worker_cfg_ab.txt; round 4 measured
  // it neutral on the frozen instance)
  if (c.gs_lds == 0u && c.stage_fb != 0u && hcap_want == 0u && c.hcap > 2048u) {
    WorkerCfg h2 = c;
    const size_t rest = c.lds - (size_t)c.hcap * 8u;
    h2.hcap = 2048u;
    h2.lds = (size_t)h2.hcap * 8u + rest;
    h2.waves = (uint32_t)num_cu * (uint32_t)std::min<size_t>(16u, WAVE_LDS_MAX / h2.lds);
    if (2u * h2.waves >= 3u * c.waves) c = h2;
  }
  // invariant the workers rely on (tsw_worker.h): LDS g-scores always come with the staged bitmap
  if (c.gs_lds != 0u) c.stage_fb = 1u;
  return c;
}

// The worker waves of one plan dispatch: the planner (workgroup 0) and one worker workgroup on every
// other CU, each holding as many single-wave workers as its dynamic LDS (the planner's `lds`, whole-CU
// size) carves and its `block` threads seat. The host sizes its global g-score / heap slots by `want`
// and then runs no more waves than the `nslots` it has. wave_lds: WorkerCfg::lds.
struct WorkerLayout {
  uint32_t lds_per_wave, wpb;  // WorkerArgs::lds_per_wave / wpb
  uint32_t want;               // worker waves the dispatch seats
  uint32_t nworkers(uint32_t nslots) const { return std::min(want, nslots); }
  uint32_t wblocks(uint32_t nslots) const { return wpb ? (nworkers(nslots) + wpb - 1u) / wpb : 0u; }  // their workgroups
};
inline WorkerLayout worker_layout(size_t wave_lds, size_t lds, uint32_t block, int num_cu) {
  WorkerLayout L{};
  L.lds_per_wave = (uint32_t)((wave_lds + 15u) & ~(size_t)15u);
  L.wpb = L.lds_per_wave ? (uint32_t)std::min<size_t>(block / 64u, lds / L.lds_per_wave) : 0u;
  L.want = L.wpb * (uint32_t)std::max(num_cu - 1, 0);
  return L;
}

// ---- K1: carve sizes and fit tests of the five BFS kernels ------------------------------------------
// ceil(2^32 / Bp): exact p / Bp for p*Bp < 2^32 (the block kernels' __umulhi division)
inline uint32_t bp_magic(uint32_t Bp) { return (uint32_t)((0xFFFFFFFFull + Bp) / Bp); }

// the padded layouts' sizes (tsw_ctx.hip builds them): k_bfs_wave's row words, a zero guard word per
// row and a zero guard row above and below; the block kernels' 8x8 blocks, guarded the same way
inline uint32_t bfs_wave_npw(uint32_t W, uint32_t H) { return (H + 2u) * ((W + 31u) / 32u + 1u); }
inline uint32_t bfs_blk_nbp(uint32_t W, uint32_t H) { return ((H + 7u) / 8u + 2u) * ((W + 7u) / 8u + 1u); }

// k_bfs<LDS_TABLE> (tsw_bfs_block.hip): four bitmaps of H * Ww words and, with lds_table, the u16 table
inline size_t bfs_lds_bytes(uint32_t H, uint32_t Ww, uint32_t ncell, bool lds_table) {
  const size_t nwp = ((size_t)H * Ww + 3u) & ~(size_t)3u;
  size_t b = 4u * nwp * 4u;
  if (lds_table) b += (((size_t)ncell + 7u) & ~(size_t)7u) * 2u;
  return b;
}

// k_bfs_wave (tsw_bfs.hip). LDS words (u32 units) of one wave; must match the carve in k_bfs_wave. The
// list area holds at least 17 x 64 u16 (the decode's C table).
TSW_HD uint32_t wave_bfs_words(uint32_t npw, uint32_t nfk, uint32_t cap) {
  const uint32_t npw4 = (npw + 3u) & ~3u;
  const uint32_t ls = cap < 544u ? 544u : cap;
  return 2u * npw4 + 2u * nfk + ((ls + 3u) & ~3u);
}
// flag dwords per buffer: a power of two >= 64 with 32 * K >= npw
inline uint32_t bfs_wave_klog(uint32_t npw) {
  uint32_t kl = 6;
  while ((32u << kl) < npw) ++kl;
  return kl;
}
// waves per workgroup that fit max_lds (0: the kernel does not fit this grid)
inline uint32_t bfs_wave_waves_per_block(uint32_t npw, uint32_t cap, int max_lds) {
  const size_t per_wave = (size_t)wave_bfs_words(npw, 1u << bfs_wave_klog(npw), cap) * 4u;
  const size_t shared = (size_t)((npw + 3u) & ~3u) * 4u;
  if (max_lds <= 0 || shared + per_wave > (size_t)max_lds) return 0;
  return (uint32_t)std::min<size_t>(16u, ((size_t)max_lds - shared) / per_wave);
}

// k_bfs_blk (tsw_bfs_blk.hip)
constexpr uint32_t CT_U16 = 1152;  // decode run table: 18 rows x 64 lanes u16
// LDS dwords of one wave; must match the carve in k_bfs_blk: V (nbp rounded to even u64), flags,
// then the list / run-table / staging region LS, 16-B aligned (every part is a multiple of 4 dwords).
TSW_HD uint32_t blk_bfs_words(uint32_t nbp, uint32_t nfk, uint32_t cap, bool wls) {
  const uint32_t ls = 2u * cap < CT_U16 ? CT_U16 : 2u * cap;  // u16 entries: two lists, run table, staging
  return (wls ? 4u : 2u) * ((nbp + 1u) & ~1u) + 2u * nfk + ((ls + 7u) >> 3) * 4u;
}
// u64 words of the workgroup's shared part (FR u64 + AB u32), rounded to 16 B
TSW_HD uint32_t blk_shared_u64(uint32_t nbp) {
  return (nbp + (nbp + 1u) / 2u + 1u) & ~1u;
}
inline uint32_t bfs_blk_klog(uint32_t nbp) {
  uint32_t kl = 6;
  while ((32u << kl) < nbp) ++kl;
  return kl;
}
// waves per workgroup that fit LDS (pair: two goal slots per wave)
inline uint32_t bfs_blk_waves_per_block(uint32_t nbp, uint32_t cap, int max_lds, bool wls, bool pair) {
  const size_t per_wave = (size_t)blk_bfs_words(nbp, 1u << bfs_blk_klog(nbp), cap, wls) * 4u * (pair ? 2u : 1u);
  const size_t shared = (size_t)blk_shared_u64(nbp) * 8u;  // FR u64 + AB u32
  if (max_lds <= 0 || shared + per_wave > (size_t)max_lds) return 0;
  return (uint32_t)std::min<size_t>(16u, ((size_t)max_lds - shared) / per_wave);
}

// k_bfs_big (tsw_bfs_big.hip)
constexpr uint32_t BIG_THREADS = 512;
constexpr uint32_t BIG_RT_ROWS = 9;  // decode run table: 17 u16 rows = 9 dword rows per thread
TSW_HD uint32_t big_bfs_klog(uint32_t nbp) {
  uint32_t kl = 5;
  while ((32u << kl) < nbp) ++kl;
  return kl;
}
// LDS bytes of one workgroup (must match the carve in k_bfs_big)
TSW_HD size_t big_bfs_lds(uint32_t nbp, uint32_t cap) {
  const uint32_t nfk = 1u << big_bfs_klog(nbp);
  const size_t lists = (size_t)2u * cap * 2u;
  const size_t rt = (size_t)BIG_RT_ROWS * BIG_THREADS * 4u;  // reuses the flag + list area
  const size_t tail = (size_t)2u * nfk * 4u + lists;
  return (size_t)nbp * 8u + (tail > rt ? tail : rt);
}
inline bool bfs_big_fits(uint32_t nbp, int max_lds, uint32_t* cap_out) {
  if (nbp > 0xFFFFu || max_lds <= 0) return false;
  // largest list capacity (<= 8192) whose carve fits
  for (uint32_t cap = 8192; cap >= 256; cap >>= 1)
    if (big_bfs_lds(nbp, cap) <= (size_t)max_lds) {
      if (cap_out) *cap_out = cap;
      return true;
    }
  return false;
}
inline uint32_t bfs_big_workgroups(uint32_t nbp, uint32_t cap, int num_cu) {
  const size_t lds = big_bfs_lds(nbp, cap);
  return (uint32_t)num_cu * (uint32_t)std::max<size_t>(1u, CU_LDS_BYTES / lds);
}

// k_bfs_mg (tsw_bfs_mg.hip, diagnostic build only: bfs_mg_built()). LDS bytes of k_bfs_mg for a grid.
TSW_HD uint32_t mg_vbytes(uint32_t W, uint32_t H) {
  return (((W + 2u) * (H + 2u) * 2u) + 15u) & ~15u;
}
TSW_HD uint32_t mg_nwc(uint32_t nbp) { return ((nbp + 31u) / 32u + 3u) & ~3u; }
inline size_t bfs_mg_lds_bytes(uint32_t W, uint32_t H, uint32_t nbp) {
  return (size_t)mg_vbytes(W, H) + (size_t)nbp * 8u + (size_t)nbp * 4u + 3u * mg_nwc(nbp) * 4u +
         (((size_t)nbp * 2u + 15u) & ~(size_t)15u);
}

// ---- K1: which kernel builds a launch's tables ------------------------------------------------------
struct BfsGeom {
  uint32_t W, H, ncell, nfree;  // nfree: free cells (saturated at 2^32 - 1)
  uint32_t npw, nbp;            // bfs_wave_npw / bfs_blk_nbp
};
struct BfsKnobs {  // Tunables::bfs_mode / blk_cap / bfs_cap / bfs_waves / bfs_wls / bfs_pair
  uint32_t mode;   // TSW_BFS_KERNEL: 0 auto, 1 wave (row words), 2 block, 3 blk (8x8), 4 big, 5 mg
  uint32_t blk_cap, bfs_cap, waves, wls, pair;
};
enum BfsKernel : uint32_t { BFS_MG, BFS_BLK, BFS_WAVE, BFS_BIG, BFS_BLOCK };
struct BfsChoice {
  BfsKernel kernel;
  bool fits;                 // false: the forced kernel (or, in auto mode, the last resort k_bfs) does not fit this grid
  uint32_t waves_per_block;  // BLK (capped by the waves knob) / WAVE (its launcher applies the cap)
  bool pair;                 // BLK: two goals per wave
  uint32_t cap;              // LDS list entries: BLK / WAVE the knob, BIG the largest that fits
};

// Auto mode: the 8x8-block wave-per-goal kernel when its LDS fits, else the row-word wave-per-goal
// kernel, else the workgroup-per-goal kernel over blocks, else the workgroup-per-goal kernel k_bfs.
// k_bfs_mg serves a launch only when selected explicitly (TSW_BFS_KERNEL=mg, diagnostic build — measured
// 5.5 ms vs k_bfs_blk's 2.7 ms on den520d's 10k goals), its LDS layout fits and the
// levels fit u16 (<= 65535 free cells). mg_built: the library holds k_bfs_mg.
inline BfsChoice choose_bfs(const BfsGeom& g, const BfsKnobs& t, int max_lds, int num_cu, bool mg_built) {
  (void)num_cu;  // no rule reads it today: every kernel sizes its grid from it after the choice
  const uint32_t mode = t.mode;
  if (mode == 5) {
    const bool fits = mg_built && g.nfree <= 0xFFFFu && g.nbp <= 0xFFFFu && max_lds > 0 &&
                      bfs_mg_lds_bytes(g.W, g.H, g.nbp) <= (size_t)max_lds;
    return BfsChoice{BFS_MG, fits, 16u, false, 0u};
  }
  uint32_t nbw = 0;
  // two goals per wave only where two goal slots per wave fit LDS, else one
  bool pair = t.pair != 0u;
  if ((mode == 0 || mode == 3) && g.nbp <= 0x10000u) {
    nbw = std::min(t.waves, bfs_blk_waves_per_block(g.nbp, t.blk_cap, max_lds, t.wls != 0u, pair));
    if (nbw == 0 && pair) {
      pair = false;
      nbw = std::min(t.waves, bfs_blk_waves_per_block(g.nbp, t.blk_cap, max_lds, t.wls != 0u, false));
    }
  }
  if (nbw > 0 || mode == 3) return BfsChoice{BFS_BLK, nbw > 0, nbw, pair, t.blk_cap};
  uint32_t nwv = 0;
  if ((mode == 0 || mode == 1) && g.npw <= 0x8000u) nwv = bfs_wave_waves_per_block(g.npw, t.bfs_cap, max_lds);
  if (nwv == 0 && mode == 1) return BfsChoice{BFS_WAVE, false, 0u, false, t.bfs_cap};
  uint32_t big_cap = 0;
  // large grids (e.g. 1024x1024): one workgroup per goal, shared visited bitmap in LDS
  if (nwv == 0 && (mode == 0 || mode == 4) && bfs_big_fits(g.nbp, max_lds, &big_cap))
    return BfsChoice{BFS_BIG, true, BIG_THREADS / 64u, false, big_cap};
  if (mode == 4) return BfsChoice{BFS_BIG, false, 0u, false, 0u};
  if (nwv > 0) return BfsChoice{BFS_WAVE, true, nwv, false, t.bfs_cap};
  return BfsChoice{BFS_BLOCK, bfs_lds_bytes(g.H, (g.W + 31u) / 32u, g.ncell, false) <= (size_t)std::max(max_lds, 0),
                   0u, false, 0u};
}

// ---- K8: the task timeline's three passes (tsw_timeline.hip) ----------------------------------------
// Pass A works on tiles of TL_TILE_AGENTS agents x TL_TILE_COLS columns, one TL_A_BLOCK-thread workgroup
// each. Pass B is one workgroup of TL_B_BLOCK threads, whatever the instance: the replay is sequential in
// (t, agent), and a take's arg-min wants every lane of one CU. Its candidates (8 B a task) go to dynamic LDS
// as far as the workgroup's limit allows beside the static tl_replay_lds_bytes, in whole strides of the
// block (tl_lds_candidates: 18,432 of them with 160 KiB); the others stay in global memory. Pass C is one
// thread per task.
constexpr uint32_t TL_TILE_AGENTS = 64u, TL_TILE_COLS = 64u, TL_A_BLOCK = 256u;
constexpr uint32_t TL_B_BLOCK = 1024u, TL_C_BLOCK = 256u;
// pass B's LDS: release counts and flags of TL_B_BLOCK columns, the takers' positions of TL_B_BLOCK agents,
// and per wave the take mask, the stay mask and the arg-min slot
constexpr size_t tl_replay_lds_bytes() { return (size_t)TL_B_BLOCK * 4u * 3u + (size_t)(TL_B_BLOCK / 64u) * 8u * 3u; }
inline uint32_t tl_tiles(uint32_t count, uint32_t tile) { return (count + tile - 1u) / tile; }
// candidates of pass B that live in LDS: a multiple of TL_B_BLOCK, no more than m rounded up to one
inline uint32_t tl_lds_candidates(uint32_t m, int max_lds) {
  const size_t fixed = tl_replay_lds_bytes() + 1024u;  // the static part and some room for the compiler's own
  if (max_lds <= 0 || (size_t)max_lds <= fixed) return 0u;
  const size_t fit = ((size_t)max_lds - fixed) / 8u / TL_B_BLOCK, want = ((size_t)m + TL_B_BLOCK - 1u) / TL_B_BLOCK;
  return (uint32_t)(std::min(fit, want) * TL_B_BLOCK);
}
inline uint32_t tl_attach_workgroups(uint32_t m) { return std::max<uint32_t>(tl_tiles(m, TL_C_BLOCK), 1u); }

// ---- K9: the space-time A* with reservations (tsw_st_astar.hip) -------------------------------------
// One wave per query, ST_WPB waves per workgroup. A wave's pop is a chain of dependent global loads (the
// reservation set and its visited table), so the rule is "as many waves per CU as the hardware seats" (32, or
// what the workgroups' LDS leaves: 20 with a staged bitmap near its 16 KiB limit):
// the LDS heap is 512 entries a wave — searches with reservations peak at a few hundred, a larger heap moves
// to the wave's global overflow heap — and the free-cell bitmap is staged once per workgroup while it is
// small. Carve: ST_WPB heaps, then the bitmap.
constexpr uint32_t ST_WPB = 4u, ST_HEAP_LDS = 512u, ST_HEAP_LDS_MIN = 64u, ST_FB_LDS_MAX = 16u * 1024u;
constexpr uint32_t ST_WAVES_PER_CU = 32u;
struct StAstarCfg {
  uint32_t wpb, hl, fb_lds;  // waves per workgroup, LDS heap entries per wave, bitmap staged in LDS
  uint32_t waves;            // waves the device seats at once
  size_t lds;                // dynamic LDS of one workgroup
};
// hl_want: Tunables::st_heap (0: ST_HEAP_LDS)
inline StAstarCfg st_astar_config(const DevGrid& G, int max_lds, int num_cu, uint32_t hl_want = 0u) {
  const size_t room = (size_t)std::max(max_lds, 0);
  const size_t fbb = ((size_t)G.H * G.Ww * 4u + 15u) / 16u * 16u;
  StAstarCfg c{};
  c.wpb = ST_WPB;
  c.hl = hl_want ? std::min(std::max(hl_want, 4u), ST_HEAP_LDS) : ST_HEAP_LDS;
  while (c.hl > ST_HEAP_LDS_MIN && (size_t)c.wpb * c.hl * 8u > room) c.hl >>= 1;
  const size_t heaps = (size_t)c.wpb * c.hl * 8u;
  c.fb_lds = fbb <= ST_FB_LDS_MAX && heaps + fbb <= room ? 1u : 0u;
  c.lds = heaps + (c.fb_lds ? fbb : 0u);
  const uint32_t wg_per_cu = (uint32_t)std::min<size_t>(ST_WAVES_PER_CU / c.wpb, std::max<size_t>(1u, CU_LDS_BYTES / c.lds));
  c.waves = (uint32_t)std::max(num_cu, 1) * wg_per_cu * c.wpb;
  return c;
}

}  // namespace tsw
