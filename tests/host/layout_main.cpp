// Stand-alone check of the host runtime's scratch layouts (csrc/tsw_layout.h). Built with the host compiler alone —
// no HIP, no device — under ASan + UBSan by tests/test_layout.py. For every block and every combination of the
// swept sizes: (1) the layout's total is the closed-form sum the call site carried before there were layouts, written
// out here literally with the name of the function that held it; (2) the parts come in the documented order, do not
// overlap and end within the total; (3) every part addressed as 64-bit words or uint2 starts on an even word;
// (4) the parts that one memset or one copy covers are adjacent; (5) a malloc of exactly `total` words takes a write
// to the first and last word of every part (ASan reports a layout that runs past its own total).
// The counts that kernel headers own are this program's own numbers: the library's (scan tile 2048, MAPD_WORDS 8,
// AUD_NKIND / NCOL / NAGENT 5 / 11 / 4, TL_NQ / NW / NTASK 5 / 10 / 4) and others. Exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tsw_layout.h"

using namespace tsw;

static int fails = 0;
static long checks = 0;

#define CHECK(cond, ...)               \
  do {                                 \
    ++checks;                          \
    if (!(cond)) {                     \
      if (fails < 50) {                \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
      ++fails;                         \
    }                                  \
  } while (0)

struct Part {
  const char* name;
  size_t off, words;
  bool wide;  // addressed as 64-bit words or uint2
};

// (2), (3) and (5) for one block, its parts in the documented order
static void check_block(const char* block, const std::vector<Part>& parts, size_t total) {
  size_t end = 0;
  for (const Part& p : parts) {
    CHECK(p.off >= end, "%s.%s starts at %zu, the part before it ends at %zu", block, p.name, p.off, end);
    CHECK(p.off + p.words <= total, "%s.%s ends at %zu of %zu", block, p.name, p.off + p.words, total);
    if (p.wide) CHECK(p.off % 2 == 0, "%s.%s starts on odd word %zu", block, p.name, p.off);
    end = std::max(end, p.off + p.words);
  }
  CHECK(end == total, "%s: the parts end at %zu, total %zu", block, end, total);
  uint32_t* w = static_cast<uint32_t*>(std::malloc(total * sizeof(uint32_t)));
  if (total) CHECK(w != nullptr, "%s: malloc of %zu words", block, total);
  if (!w) return;
  for (const Part& p : parts)
    if (p.words) {
      w[p.off] = 1u;
      w[p.off + p.words - 1] = 2u;
    }
  std::free(w);
}

// (4): b lies right behind a
static void adjacent(const char* block, const Part& a, const Part& b) {
  CHECK(a.off + a.words == b.off, "%s: %s ends at %zu, %s starts at %zu", block, a.name, a.off + a.words, b.name, b.off);
}

static size_t scan_blocks(size_t m, size_t tile) { return (m + tile - 1) / tile; }  // nb_scan_blocks of tsw_nearby.h

static const size_t N[] = {1, 2, 63, 64, 65, 1023, 1024, 1025};
static const size_t M[] = {0, 1, 2, 3, 1024, 1025};
static const size_t TT[] = {1, 2, 3, 1024};
static const size_t NCELL[] = {1, 64, 65, 40000};
static const size_t KB[] = {1, 2, 4097};
static const size_t EXTRA[] = {0, 1};
static const size_t TILE[] = {2048, 64};
static const size_t MAPD_W[] = {8, 5};
static const bool ONOFF[] = {false, true};

static void fleet_blocks() {
  for (size_t n : N)
    for (size_t tile : TILE) {
      const size_t nbs_n = scan_blocks(n, tile);
      for (size_t ncell : NCELL)
        for (size_t extra : EXTRA) {
          const size_t nbs = std::max(scan_blocks(ncell, tile), nbs_n);
          const FleetListsLayout L = fleet_lists_layout(n, ncell, nbs, extra);
          // fleet_lists_setup
          CHECK(L.total == 4 + 2 * n + (ncell + 1) + 2 * n + (n + 1) + nbs + extra, "count pass n %zu ncell %zu", n, ncell);
          const std::vector<Part> p = {{"total64", L.total64, 2, true}, {"maxlen", L.maxlen, 1, false}, {"pad", L.pad, 1, false},
                                       {"cell_start", L.cell_start, ncell + 1, false}, {"v", L.v, n, false}, {"g", L.g, n, false},
                                       {"rank", L.rank, n, false}, {"sorted", L.sorted, n, false}, {"off", L.off, n + 1, false},
                                       {"bsum", L.bsum, nbs, false}, {"extra", L.extra, extra, false}};
          check_block("count pass", p, L.total);
          CHECK(L.total64 == 0, "total64 at word %zu", L.total64);
          adjacent("count pass", p[0], p[1]);  // total64 | maxlen | pad: one read-back
          adjacent("count pass", p[1], p[2]);
          adjacent("count pass", p[2], p[3]);  // total64 | maxlen (+ pad) | cell_start: one memset
          adjacent("count pass", p[4], p[5]);  // v | g: one copy
        }
      {
        const FleetApplyLayout L = fleet_apply_layout(n, nbs_n);
        CHECK(L.total == 5 * n + 1 + nbs_n + 1, "apply state n %zu", n);  // fleet_apply_words
        check_block("apply state", {{"g0", L.g0, n, false}, {"owner", L.owner, n, false}, {"opflag", L.opflag, n + 1, false},
                                    {"ops", L.ops, 2 * n, false}, {"bsum", L.bsum, nbs_n, false}, {"changed", L.changed, 1, false}},
                    L.total);
      }
      for (size_t m : M)
        for (size_t words : MAPD_W) {
          const FleetMapdLayout L = fleet_mapd_layout(n, m, words, nbs_n);
          CHECK(L.total == 3 * n + words + 1 + nbs_n + 2 * m, "MAPD state n %zu m %zu", n, m);  // fleet_mapd_words
          const std::vector<Part> p = {{"st", L.st, n, false}, {"words", L.words, words, false}, {"tk", L.tk, n, false},
                                       {"flag", L.flag, n + 1, false}, {"bsum", L.bsum, nbs_n, false}, {"pick", L.pick, m, false},
                                       {"dlv", L.dlv, m, false}};
          check_block("MAPD state", p, L.total);
          adjacent("MAPD state", p[0], p[1]);  // st | words: one memset
          adjacent("MAPD state", p[5], p[6]);  // pick | dlv: one copy
        }
    }
  for (size_t n : N) {
    const size_t TOT[] = {0, 1, n, 7 * n + 3};
    for (size_t tot : TOT) {
      const size_t nb = std::max<size_t>(tot, 1);
      {
        const FleetDecideLayout L = fleet_decide_layout(n, tot);
        // fleet_decide_device
        CHECK(L.total == 3 * nb + 4 * n + 2 * (tot + n) + 2 * n + 2 + (n + 1), "tick decisions n %zu tot %zu", n, tot);
        const std::vector<Part> p = {{"idx", L.idx, nb, false}, {"nv", L.nv, nb, false}, {"ng", L.ng, nb, false},
                                     {"act", L.act, n, false}, {"cell", L.cell, n, false}, {"par", L.par, n, false},
                                     {"poff", L.poff, n + 1, false}, {"np", L.np, n, false}, {"part", L.part, tot + n, false},
                                     {"q0", L.q0, n, false}, {"q1", L.q1, n, false}, {"cnt", L.cnt, 2, false},
                                     {"pout", L.pout, tot + n, false}};
        check_block("tick decisions", p, L.total);
        CHECK(L.idx == 0, "idx at word %zu", L.idx);
        adjacent("tick decisions", p[3], p[4]);  // act | cell | par | poff: one copy back
        adjacent("tick decisions", p[4], p[5]);
        adjacent("tick decisions", p[5], p[6]);
      }
      {
        const DecideLayout L = decide_layout(n, tot);
        // decide_impl
        CHECK(L.total == 2 * n + (n + 1) + 2 * nb + 4 * n + (tot + n) + 2 * n + 2, "tsw_decide n %zu tot %zu", n, tot);
        check_block("tsw_decide", {{"v", L.v, n, false}, {"g", L.g, n, false}, {"off", L.off, n + 1, false}, {"nv", L.nv, nb, false},
                                   {"ng", L.ng, nb, false}, {"act", L.act, n, false}, {"cell", L.cell, n, false},
                                   {"par", L.par, n, false}, {"np", L.np, n, false}, {"part", L.part, tot + n, false},
                                   {"q0", L.q0, n, false}, {"q1", L.q1, n, false}, {"cnt", L.cnt, 2, false}},
                    L.total);
      }
      {
        const size_t ptot = tot;  // the rotations' participants
        const FleetApplyInLayout L = fleet_apply_in_layout(n, ptot);
        CHECK(L.total == 6 * n + 1 + ptot, "apply inputs n %zu ptot %zu", n, ptot);  // tsw_fleet_apply: in_words
        const std::vector<Part> p = {{"v", L.v, n, false}, {"g", L.g, n, false}, {"act", L.act, n, false},
                                     {"cell", L.cell, n, false}, {"partner", L.partner, n, false},
                                     {"part_off", L.part_off, n + 1, false}, {"part", L.part, ptot, false}};
        check_block("apply inputs", p, L.total);
        CHECK(L.v == 0, "v at word %zu", L.v);
        adjacent("apply inputs", p[0], p[1]);  // v | g: one copy back, the changed word behind them
        adjacent("apply inputs", p[1], p[2]);
      }
    }
    for (size_t T : TT) {
      const size_t cells = n * T;  // T columns: ticks + 1, max_t + 1
      for (bool a : ONOFF)
        for (bool b : ONOFF) {
          {
            const FleetRunRecLayout L = fleet_run_rec_layout(cells, a, b);
            CHECK(L.total == ((a ? 1 : 0) + (b ? 1 : 0)) * cells, "run records n %zu T %zu", n, T);  // fleet_run_impl
            check_block("run records", {{"v_rec", L.v_rec, a ? cells : 0, false}, {"g_rec", L.g_rec, b ? cells : 0, false}}, L.total);
            CHECK(L.v_rec == 0 && L.g_rec == (a ? cells : 0), "run records: g_rec at %zu", L.g_rec);
          }
          {
            const FleetMapdRecLayout L = fleet_mapd_rec_layout(cells, a, b);
            CHECK(L.total == (2 + (a ? 1 : 0) + (b ? 1 : 0)) * cells, "MAPD records n %zu T %zu", n, T);  // fleet_mapd_impl
            check_block("MAPD records", {{"rec", L.rec, 2 * cells, true}, {"g_rec", L.g_rec, a ? cells : 0, false},
                                         {"t_rec", L.t_rec, b ? cells : 0, false}},
                        L.total);
            CHECK(L.rec == 0, "rec at word %zu", L.rec);
            CHECK(L.g_rec == 2 * cells && L.t_rec == (a ? 3 : 2) * cells, "MAPD records: g_rec %zu t_rec %zu", L.g_rec, L.t_rec);
          }
        }
    }
  }
}

static void audit_block() {
  const size_t K[][3] = {{5, 11, 4}, {3, 7, 2}};  // AUD_NKIND, AUD_NCOL, AUD_NAGENT
  for (const auto& k : K)
    for (size_t n : N)
      for (size_t T : TT)
        for (bool agent : ONOFF) {
          const size_t nkind = k[0], ncol = k[1], nagent = k[2];
          const AuditOutLayout L = audit_out_layout(n, T, agent, nkind, ncol, nagent);
          const size_t col_words = T * ncol, agent_words = agent ? n * nagent : 0;
          CHECK(L.total == 2 * nkind + col_words + agent_words, "audit outputs n %zu T %zu", n, T);  // audit_device
          CHECK(L.col_words == col_words && L.agent_words == agent_words, "audit outputs: sizes");
          const std::vector<Part> p = {{"first", L.first, 2 * nkind, true}, {"col", L.col, col_words, false},
                                       {"agent", L.agent, agent_words, false}};
          check_block("audit outputs", p, L.total);
          CHECK(L.first == 0, "first at word %zu", L.first);
          adjacent("audit outputs", p[0], p[1]);  // first | col: one copy back
        }
}

static void timeline_block() {
  // TL_NQ, TL_NW, TL_NTASK. The closed form below holds while 2 * NQ + NW and NTASK are even (tsw_timeline.h's are, and
  // the parent asserted the first): then its round-up of m to an even count is exactly what puts `sorted` on an
  // even word. With other counts the layout still aligns its 64-bit parts; the last row checks that alone.
  const size_t K[][3] = {{5, 10, 4}, {3, 6, 2}, {4, 7, 3}};
  for (const auto& k : K)
    for (size_t n : N)
      for (size_t m : M)
        for (size_t T : TT)
          for (bool nearest : ONOFF) {
            const size_t nq = k[0], nw = k[1], ntask = k[2];
            const TimelineLayout L = timeline_layout(n, m, T, nearest, nq, nw, ntask);
            if ((2 * nq + nw) % 2 == 0 && ntask % 2 == 0) {
              // timeline_device
              const size_t mp = (m + 1u) & ~(size_t)1u;
              const size_t o_q = 0, o_w = o_q + 2 * nq, o_task = o_w + nw, o_flag = o_task + m * ntask, o_vis = o_flag + T,
                           o_rel = o_vis + T, o_sorted = o_rel + mp, o_starts = o_sorted + 2 * m,
                           o_live = o_starts + (nearest ? 2 * n : 0), total = o_live + (nearest ? 2 * m : 0);
              CHECK(L.total == total, "timeline n %zu m %zu T %zu", n, m, T);
              CHECK(L.q == o_q && L.w == o_w && L.task == o_task && L.colflag == o_flag && L.vis == o_vis && L.release == o_rel &&
                        L.sorted == o_sorted && L.starts == o_starts && L.live == o_live,
                    "timeline offsets n %zu m %zu T %zu", n, m, T);
            }
            const std::vector<Part> p = {{"q", L.q, 2 * nq, true}, {"w", L.w, nw, false}, {"task", L.task, m * ntask, false},
                                         {"colflag", L.colflag, T, false}, {"vis", L.vis, T, false}, {"release", L.release, m, false},
                                         {"sorted", L.sorted, 2 * m, true}, {"starts", L.starts, nearest ? 2 * n : 0, true},
                                         {"live", L.live, nearest ? 2 * m : 0, true}};
            // one pad word at most, between release and sorted; every other part starts where the one before it ends
            CHECK(L.sorted - (L.release + m) <= 1, "timeline: %zu pad words before sorted", L.sorted - (L.release + m));
            for (size_t i = 0; i + 1 < p.size(); ++i)
              if (i != 5) adjacent("timeline", p[i], p[i + 1]);  // q | w | task among them: one copy back
            check_block("timeline", p, L.total);
            CHECK(L.q == 0, "q at word %zu", L.q);
          }
}

static void st_block() {
  for (size_t kb : KB) {
    const StBatchLayout L = st_batch_layout(kb);
    CHECK(L.total == 7u * kb, "space-time batch kb %zu", kb);  // tsw_astar_reserved
    const std::vector<Part> p = {{"start", L.start, kb, false}, {"goal", L.goal, kb, false}, {"start_time", L.start_time, kb, false},
                                 {"status", L.status, kb, false}, {"pops", L.pops, kb, false}, {"len", L.len, kb, false},
                                 {"path_off", L.path_off, kb, false}};
    check_block("space-time batch", p, L.total);
    CHECK(L.start == 0, "start at word %zu", L.start);
    for (int i = 0; i < 6; ++i) adjacent("space-time batch", p[i], p[i + 1]);  // start .. start_time up, status .. len down
  }
}

int main() {
  {  // the walk itself
    Carve c;
    CHECK(c.take(3) == 0 && c.total() == 3, "take");
    CHECK(c.take64(2) == 4 && c.total() == 8, "take64 skips to an even word");
    CHECK(c.take64(0) == 8 && c.total() == 8, "an empty take64 on an even word moves nothing");
    CHECK(c.take(0) == 8 && c.take(1) == 8 && c.total() == 9, "an empty take moves nothing");
  }
  fleet_blocks();
  audit_block();
  timeline_block();
  st_block();
  std::printf("%ld checks, %d failed\n", checks, fails);
  if (fails) return 1;
  std::printf("layout ok\n");
  return 0;
}
