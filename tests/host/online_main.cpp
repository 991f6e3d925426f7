// Stand-alone driver for the release schedule of tsw_plan_mapd_online (csrc/tsw_online.h): the tasks in release
// order, the epochs, the segment limits and what follows a stopped segment (hold range, next column, end of the
// run). Built with the host compiler alone — no HIP, no device — under ASan + UBSan by
// tests/test_online_schedule.py. Pinned cases first, then a seeded sweep that walks the host's segment loop with a
// stand-in for k_plan and checks that the columns of a run are covered once, in order, and that every task with
// release <= max_t is released once, at its time. Exits non-zero when a case fails.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tsw_online.h"

using namespace tsw;

static int fails = 0;
static long checks = 0;

#define CHECK(cond, ...)               \
  do {                                 \
    ++checks;                          \
    if (!(cond)) {                     \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);        \
      std::printf("\n");               \
      ++fails;                         \
    }                                  \
  } while (0)

static bool same(const std::vector<uint32_t>& a, std::initializer_list<uint32_t> b) { return a == std::vector<uint32_t>(b); }

static void pins() {
  {  // unsorted and duplicate release times: ties keep task index order
    const uint32_t rel[] = {5, 0, 3, 5, 3, 0, 9};
    const OnlineSchedule S = online_schedule(rel, 7, 10);
    CHECK(same(S.rel_order, {1, 5, 2, 4, 0, 3, 6}), "order");
    CHECK(S.at_zero == 2 && S.never == 0 && S.epochs.size() == 3 && S.segments() == 4, "counts");
    CHECK(S.epochs[0].t == 3 && S.epochs[0].lo == 2 && S.epochs[0].hi == 4, "epoch 0");
    CHECK(S.epochs[1].t == 5 && S.epochs[1].lo == 4 && S.epochs[1].hi == 6, "epoch 1");
    CHECK(S.epochs[2].t == 9 && S.epochs[2].lo == 6 && S.epochs[2].hi == 7, "epoch 2");
    CHECK(S.segment_limit(0) == 2 && S.segment_limit(1) == 4 && S.segment_limit(2) == 8 && S.segment_limit(3) == 10, "limits");
    CHECK(S.released_lo(0) == 0 && S.released_hi(0) == 2 && S.released_lo(2) == 4 && S.released_hi(2) == 6, "released");
    OnlineNext nx = online_next(S, 0, 3);  // stopped at the limit: no hold, on to column 3
    CHECK(nx.hold_from == nx.hold_to && nx.next_t == 3 && !nx.done, "limit stop");
    nx = online_next(S, 1, 4);  // stopped early after column 3: column 4 repeats it
    CHECK(nx.hold_from == 4 && nx.hold_to == 5 && nx.next_t == 5 && !nx.done, "early stop");
    nx = online_next(S, 3, 10);  // last segment, every task used: over where it stopped
    CHECK(nx.hold_from == nx.hold_to && nx.next_t == 10 && nx.done, "end");
    nx = online_next(S, 3, 11);
    CHECK(nx.hold_from == nx.hold_to && nx.next_t == 11 && nx.done, "end at max_t");
  }
  {  // releases at 0, at max_t and at max_t + 1
    const uint32_t rel[] = {0, 10, 11};
    const OnlineSchedule S = online_schedule(rel, 3, 10);
    CHECK(S.at_zero == 1 && S.never == 1 && S.epochs.size() == 1 && S.epochs[0].t == 10, "counts");
    CHECK(S.epochs[0].lo == 1 && S.epochs[0].hi == 2, "epoch");
    CHECK(S.segment_limit(0) == 9 && S.segment_limit(1) == 10, "limits");
    OnlineNext nx = online_next(S, 0, 4);
    CHECK(nx.hold_from == 4 && nx.hold_to == 10 && nx.next_t == 10 && !nx.done, "hold to the last column");
    nx = online_next(S, 1, 11);
    CHECK(nx.hold_from == nx.hold_to && nx.next_t == 11 && nx.done, "max_t reached");
  }
  {  // m = 0, and release == nullptr
    const OnlineSchedule S = online_schedule(nullptr, 0, 7);
    CHECK(S.rel_order.empty() && S.epochs.empty() && S.segments() == 1 && S.segment_limit(0) == 7 && S.never == 0, "m = 0");
    const OnlineNext nx = online_next(S, 0, 1);
    CHECK(nx.done && nx.next_t == 1 && nx.hold_from == nx.hold_to, "m = 0 ends at once");
    const OnlineSchedule N = online_schedule(nullptr, 5, 7);
    CHECK(same(N.rel_order, {0, 1, 2, 3, 4}) && N.at_zero == 5 && N.epochs.empty() && N.never == 0, "null release");
  }
  {  // all tasks never released: one segment, held to max_t
    const uint32_t rel[] = {50, 60};
    const OnlineSchedule S = online_schedule(rel, 2, 40);
    CHECK(S.at_zero == 0 && S.never == 2 && S.epochs.empty() && S.segment_limit(0) == 40, "counts");
    OnlineNext nx = online_next(S, 0, 1);
    CHECK(nx.hold_from == 1 && nx.hold_to == 41 && nx.next_t == 41 && nx.done, "hold capped at max_t");
    nx = online_next(S, 0, 41);
    CHECK(nx.hold_from == nx.hold_to && nx.next_t == 41 && nx.done, "already there");
  }
  {  // hold ranges that hit max_t: a gap past it, and a release exactly at it
    const uint32_t past[] = {0, 100};
    OnlineSchedule S = online_schedule(past, 2, 20);
    OnlineNext nx = online_next(S, 0, 7);
    CHECK(nx.hold_from == 7 && nx.hold_to == 21 && nx.next_t == 21 && nx.done, "gap past max_t");
    const uint32_t at[] = {0, 20};
    S = online_schedule(at, 2, 20);
    nx = online_next(S, 0, 7);
    CHECK(nx.hold_from == 7 && nx.hold_to == 20 && nx.next_t == 20 && !nx.done, "gap to max_t");
    CHECK(S.segment_limit(1) == 20, "last segment");
    nx = online_next(S, 1, 21);
    CHECK(nx.hold_from == nx.hold_to && nx.next_t == 21 && nx.done, "done");
  }
  {  // max_t = 0: one column, whatever is released later is never seen
    const uint32_t rel[] = {0, 1, 0xFFFFFFFFu};
    const OnlineSchedule S = online_schedule(rel, 3, 0);
    CHECK(S.at_zero == 1 && S.never == 2 && S.epochs.empty() && S.segment_limit(0) == 0, "max_t 0");
    const OnlineNext nx = online_next(S, 0, 1);
    CHECK(nx.done && nx.next_t == 1 && nx.hold_from == nx.hold_to, "max_t 0 ends");
  }
}

static uint64_t rng_state = 0x0123456789ABCDEFull;
static uint32_t rnd(uint32_t below) {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) % below);
}

// The host's segment loop with a stand-in for k_plan: a segment started at column t records at least one column
// and stops anywhere up to its limit + 1.
static void sweep() {
  for (int it = 0; it < 4000; ++it) {
    const uint32_t m = rnd(40), max_t = rnd(60), span = 1u + rnd(90);
    std::vector<uint32_t> rel(m);
    for (auto& r : rel) r = rnd(3) == 0 ? 0u : rnd(span);
    const OnlineSchedule S = online_schedule(m ? rel.data() : nullptr, m, max_t);
    std::vector<int> seen(m, 0);
    std::vector<int> col((size_t)max_t + 2, 0);
    for (uint32_t j = 0; j + 1 < m; ++j) {
      const uint32_t a = S.rel_order[j], b = S.rel_order[j + 1];
      CHECK(rel[a] < rel[b] || (rel[a] == rel[b] && a < b), "order %u %u", a, b);
    }
    for (uint32_t j = S.released_lo(0); j < S.released_hi(0); ++j) {
      CHECK(rel[S.rel_order[j]] == 0, "segment 0 task");
      ++seen[S.rel_order[j]];
    }
    uint32_t t = 0, T = 0;
    for (uint32_t e = 0;; ++e) {
      const uint32_t lim = S.segment_limit(e);
      CHECK(lim >= t && lim <= max_t, "limit %u start %u", lim, t);
      const uint32_t stop = t + 1u + rnd(lim - t + 1u);  // PlanCtl::t when k_plan stops: t + 1 .. lim + 1
      for (uint32_t c = t; c < stop; ++c) ++col[c];
      const OnlineNext nx = online_next(S, e, stop);
      CHECK(nx.hold_from == stop && nx.hold_to >= nx.hold_from && nx.hold_to <= max_t + 1u, "hold %u %u", nx.hold_from, nx.hold_to);
      for (uint32_t c = nx.hold_from; c < nx.hold_to; ++c) ++col[c];
      CHECK(nx.next_t == nx.hold_to, "next column follows the hold");
      if (nx.done) {
        T = nx.next_t;
        CHECK(e + 1u == S.segments(), "done in the last segment");
        break;
      }
      CHECK(e < S.epochs.size() && nx.next_t == S.epochs[e].t, "next is the release time");
      for (uint32_t j = S.released_lo(e + 1u); j < S.released_hi(e + 1u); ++j) {
        CHECK(rel[S.rel_order[j]] == nx.next_t, "released at its time");
        ++seen[S.rel_order[j]];
      }
      t = nx.next_t;
    }
    CHECK(T >= 1 && T <= max_t + 1u, "T %u", T);
    if (S.never) CHECK(T == max_t + 1u, "unreleased tasks keep the run alive");
    for (uint32_t c = 0; c <= max_t; ++c) CHECK(col[c] == (c < T ? 1 : 0), "column %u written %d times (T %u)", c, col[c], T);
    uint32_t never = 0;
    for (uint32_t k = 0; k < m; ++k) {
      CHECK(seen[k] == (rel[k] <= max_t ? 1 : 0), "task %u released %d times", k, seen[k]);
      never += rel[k] > max_t;
    }
    CHECK(never == S.never, "never %u %u", never, S.never);
  }
}

int main() {
  pins();
  sweep();
  std::printf("%ld checks, %d failed\n", checks, fails);
  if (fails == 0) std::printf("online schedule ok\n");
  return fails ? 1 : 0;
}
