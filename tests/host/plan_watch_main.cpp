// Stand-alone driver for what the plan dispatch loop shares with the planner by convention (csrc/tsw_plan.h):
// the watchdog rule (PlanWatchdog), the error table (PLAN_ERR_TABLE / plan_err_row) and the slot enums of
// PlanArgs::hflags and PlanArgs::sec_ticks. Built with the host compiler alone — no HIP, no device — under
// ASan + UBSan by tests/test_plan_watch.py. The clock is fake: time points built by hand, nothing sleeps.
// Exits non-zero when a case fails.
#include <chrono>
#include <cstdint>
#include <cstdio>

#include "tsw_plan.h"

using namespace tsw;
using Clock = PlanWatchdog::Clock;
using std::chrono::milliseconds;
using std::chrono::nanoseconds;

static int fails = 0;

static void expect(const char* name, bool got, bool want) {
  if (got != want) {
    std::printf("FAIL %s: got %d want %d\n", name, (int)got, (int)want);
    ++fails;
  } else {
    std::printf("ok   %s\n", name);
  }
}

static void watchdog_cases() {
  const Clock::time_point t0{};  // the fake clock's origin
  const uint32_t ms = 250u;

  // a heartbeat that advances at every check never fires, however long the dispatch runs
  {
    PlanWatchdog w(ms, 0u, t0);
    bool any = false;
    for (uint32_t k = 1; k <= 100u; ++k) any |= w.check(k, 0u, t0 + milliseconds(1000) * k);
    expect("advancing heartbeat never fires", any, false);
    expect("advancing heartbeat: latch clear", w.fired, false);
  }

  // a still heartbeat: not at exactly watchdog_ms, at the next instant yes; then never again
  {
    PlanWatchdog w(ms, 7u, t0);
    expect("still: well before the limit", w.check(7u, 0u, t0 + milliseconds(ms / 2)), false);
    expect("still: at exactly watchdog_ms", w.check(7u, 0u, t0 + milliseconds(ms)), false);
    expect("still: one tick past watchdog_ms", w.check(7u, 0u, t0 + milliseconds(ms) + Clock::duration(1)), true);
    bool again = false;
    // the caller raises the abort word after a firing; the latch holds whether or not the word reads back yet
    for (uint32_t k = 2; k <= 50u; ++k) again |= w.check(7u, k & 1u, t0 + milliseconds(ms) * k);
    expect("still: fires once only", again, false);
    // a heartbeat that moves after the firing re-arms the timer, not the latch
    expect("moves after the firing", w.check(8u, 1u, t0 + milliseconds(ms) * 60), false);
    expect("moved: timer re-armed", w.seen == t0 + milliseconds(ms) * 60 && w.last == 8u, true);
    expect("still again after the firing, abort word set", w.check(8u, 1u, t0 + milliseconds(ms) * 70), false);
    expect("still again after the firing, abort word clear", w.check(8u, 0u, t0 + milliseconds(ms) * 80), false);
  }

  // the timer counts from the last change, not from the start
  {
    PlanWatchdog w(ms, 0u, t0);
    expect("re-arm: change at 200 ms", w.check(1u, 0u, t0 + milliseconds(200)), false);
    expect("re-arm: 251 ms after the start, 51 after the change", w.check(1u, 0u, t0 + milliseconds(251)), false);
    expect("re-arm: exactly watchdog_ms after the change", w.check(1u, 0u, t0 + milliseconds(200 + ms)), false);
    expect("re-arm: past watchdog_ms after the change", w.check(1u, 0u, t0 + milliseconds(201 + ms)), true);
  }

  // an abort word that is already set (a firing carried from the caller) never fires
  {
    PlanWatchdog w(ms, 3u, t0);
    bool any = false;
    for (uint32_t k = 1; k <= 20u; ++k) any |= w.check(3u, 1u, t0 + milliseconds(ms) * k);
    expect("abort word already set never fires", any, false);
    expect("abort word already set: latch clear", w.fired, false);
  }

  // the limits of watchdog_ms: 1 ms, and 0xFFFFFFFF ms (49.7 days) without overflow
  {
    PlanWatchdog w(1u, 0u, t0);
    expect("1 ms: at 1 ms", w.check(0u, 0u, t0 + milliseconds(1)), false);
    expect("1 ms: one tick later", w.check(0u, 0u, t0 + milliseconds(1) + Clock::duration(1)), true);
    expect("1 ms: once", w.check(0u, 0u, t0 + milliseconds(5)), false);
  }
  {
    const uint32_t big = 0xFFFFFFFFu;
    PlanWatchdog w(big, 0u, t0);
    expect("0xFFFFFFFF ms: limit kept whole", w.limit == milliseconds(4294967295ll), true);
    expect("0xFFFFFFFF ms: after a day", w.check(0u, 0u, t0 + std::chrono::hours(24)), false);
    expect("0xFFFFFFFF ms: at the limit", w.check(0u, 0u, t0 + milliseconds(4294967295ll)), false);
    expect("0xFFFFFFFF ms: one tick past it", w.check(0u, 0u, t0 + milliseconds(4294967295ll) + Clock::duration(1)), true);
    expect("0xFFFFFFFF ms: once", w.check(0u, 0u, t0 + milliseconds(4294967295ll) * 2), false);
  }

  // a fresh object for the next dispatch is armed again, from its own start
  {
    const Clock::time_point t1 = t0 + milliseconds(100000);
    PlanWatchdog a(ms, 5u, t0);
    expect("first dispatch fires", a.check(5u, 0u, t0 + milliseconds(ms + 1)), true);
    PlanWatchdog b(ms, 5u, t1);
    expect("next dispatch: armed, not yet", b.check(5u, 0u, t1 + milliseconds(ms)), false);
    expect("next dispatch: fires", b.check(5u, 0u, t1 + milliseconds(ms + 1)), true);
  }
}

static int code_of(uint32_t err) {
  const PlanErrRow* r = plan_err_row(err);
  return r ? r->code : TSW_OK;
}
static uint32_t row_of(uint32_t err) {
  const PlanErrRow* r = plan_err_row(err);
  return r ? r->bits : 0u;
}

static void error_table_cases() {
  expect("no error: no row", plan_err_row(0u) == nullptr, true);
  // each bit alone
  expect("ERR_ABORT alone", row_of(ERR_ABORT) == ERR_ABORT && code_of(ERR_ABORT) == TSW_EINVAL, true);
  expect("ERR_ABORT: message composed by the host", plan_err_row(ERR_ABORT)->msg == nullptr, true);
  expect("ERR_BAD_PICKUP alone", row_of(ERR_BAD_PICKUP) == ERR_BAD_PICKUP && code_of(ERR_BAD_PICKUP) == TSW_EINVAL, true);
  expect("ERR_BAD_PICKUP: fixed message", plan_err_row(ERR_BAD_PICKUP)->msg != nullptr, true);
  expect("ERR_BAD_DELIVERY alone", row_of(ERR_BAD_DELIVERY) == ERR_BAD_DELIVERY && code_of(ERR_BAD_DELIVERY) == TSW_EINVAL, true);
  expect("ERR_BAD_DELIVERY: fixed message", plan_err_row(ERR_BAD_DELIVERY)->msg != nullptr, true);
  expect("pickup and delivery messages differ", plan_err_row(ERR_BAD_PICKUP)->msg != plan_err_row(ERR_BAD_DELIVERY)->msg, true);
  expect("ERR_NO_TABLE alone", row_of(ERR_NO_TABLE) == ERR_NO_TABLE && code_of(ERR_NO_TABLE) == TSW_EINVAL, true);
  const uint32_t named = ERR_ABORT | ERR_BAD_PICKUP | ERR_BAD_DELIVERY | ERR_NO_TABLE;
  for (uint32_t b = 0; b < 32u; ++b) {
    const uint32_t bit = 1u << b;
    if (bit & named) continue;
    char name[64];
    std::snprintf(name, sizeof name, "bit %u alone -> TSW_EOVERFLOW", b);
    expect(name, code_of(bit) == TSW_EOVERFLOW && plan_err_row(bit)->msg == nullptr, true);
  }
  // the order of the loop: ABORT, BAD_PICKUP, BAD_DELIVERY, NO_TABLE, the rest
  expect("ABORT wins over everything", row_of(0xFFFFFFFFu) == ERR_ABORT, true);
  expect("ABORT over BAD_PICKUP", row_of(ERR_ABORT | ERR_BAD_PICKUP) == ERR_ABORT, true);
  expect("ABORT over an overflow bit", row_of(ERR_ABORT | ERR_HEAP_OVERFLOW) == ERR_ABORT && code_of(ERR_ABORT | ERR_HEAP_OVERFLOW) == TSW_EINVAL, true);
  expect("BAD_PICKUP next", row_of(0xFFFFFFFFu & ~ERR_ABORT) == ERR_BAD_PICKUP, true);
  expect("BAD_PICKUP over BAD_DELIVERY", row_of(ERR_BAD_PICKUP | ERR_BAD_DELIVERY) == ERR_BAD_PICKUP, true);
  expect("BAD_DELIVERY next", row_of(0xFFFFFFFFu & ~(ERR_ABORT | ERR_BAD_PICKUP)) == ERR_BAD_DELIVERY, true);
  expect("BAD_DELIVERY over NO_TABLE and overflow bits", row_of(ERR_BAD_DELIVERY | ERR_NO_TABLE | ERR_G_OVERFLOW) == ERR_BAD_DELIVERY, true);
  expect("NO_TABLE next", row_of(0xFFFFFFFFu & ~(ERR_ABORT | ERR_BAD_PICKUP | ERR_BAD_DELIVERY)) == ERR_NO_TABLE, true);
  expect("NO_TABLE with an overflow bit -> TSW_EINVAL", code_of(ERR_NO_TABLE | ERR_HEAP_OVERFLOW) == TSW_EINVAL, true);
  expect("the rest -> TSW_EOVERFLOW", code_of(0xFFFFFFFFu & ~named) == TSW_EOVERFLOW, true);
  expect("overflow bits together", code_of(ERR_HEAP_OVERFLOW | ERR_WALK_OVERFLOW) == TSW_EOVERFLOW, true);
}

static void slot_cases() {
  // PlanArgs::hflags: the single words, and the two per-wave runs of PLAN_WAVES_MAX words
  const int single[] = {HF_RESIDENT, HF_ABORT, HF_HEARTBEAT, HF_HOST_TAIL, HF_BAR_MISMATCH};
  bool used[HF_WORDS] = {false};
  bool clash = false, inside = true;
  auto take = [&](int w) {
    if (w < 0 || w >= HF_WORDS) {
      inside = false;
      return;
    }
    clash |= used[w];
    used[w] = true;
  };
  for (int w : single) take(w);
  for (int w = 0; w < PLAN_WAVES_MAX; ++w) take(HF_BAR_LINE + w);
  for (int w = 0; w < PLAN_WAVES_MAX; ++w) take(HF_BAR_COUNT + w);
  expect("hflags: no two names share a word", clash, false);
  expect("hflags: every word below HF_WORDS", inside, true);
  expect("hflags: room for 16 waves", PLAN_WAVES_MAX == 16 && HF_BAR_COUNT - HF_BAR_LINE >= 16 && HF_WORDS - HF_BAR_COUNT >= 16, true);

  // PlanArgs::sec_ticks
  expect("sec_ticks: counts", TK_SECTIONS == 8 && TK_STICK_COUNT == 48 && TK_COUNT == 64, true);
  const int lds[] = {TK_MOVE_PASS1, TK_R3_WALK_HOPS, TK_MOVE_PASS2, TK_R4_ROTATIONS, TK_MOVE_PASS3, TK_RULES_SCAN, TK_RULES_FIRE,
                     TK_RULES_RELABEL, TK_WR_LOAD, TK_WR_STALE, TK_WR_FAST, TK_WR_UPDATE, TK_WR_SLOW, TK_WR_ROT, TK_WR_LOADS,
                     TK_WR_FAST_FIRINGS, TK_PRE1_PUBLISH, TK_PRE1_PUBLISHES, TK_RULES_INIT, TK_RULES_PREFETCH, TK_RULES_PUBLISH,
                     TK_RULES_PUBLISHES, TK_SETTLE_SUCC, TK_SETTLE_WALK, TK_ASG_TRANSITIONS, TK_ASG_COMPACT, TK_ASG_SCAN,
                     TK_ASG_ACCEPT, TK_ASG_UPDATE, TK_ASG_BATCHES, TK_ASG_ACCEPTED, TK_ASG_SECTIONS, TK_WB_MARKS, TK_WB_WALKS,
                     TK_WB_APPLY, TK_WB_BATCHES, TK_WB_HOPS, TK_WALK_IN_PRE1, TK_WALK_LEFT, TK_WALK_WAVE0_FIRST};
  const int direct[] = {TK_SCAN_INDEX, TK_SCAN_BOUND, TK_SCAN_ENTRIES, TK_SCAN_REDUCE, TK_SCAN_PAIRS, TK_SCAN_CHUNKS, TK_SCAN_WAVES,
                        TK_SCAN_B_ONE, TK_SCAN_B_LE4, TK_SCAN_B_LE8, TK_SCAN_B_MORE, TK_SCAN_ROUNDS, TK_WALKERS, TK_WALK_IN_RULES};
  bool tused[TK_COUNT] = {false};
  bool tclash = false, below48 = true, from48 = true;
  for (int s = TK_SECTION; s < TK_SECTIONS; ++s) tused[s] = true;
  for (int s : lds) {
    below48 &= s >= TK_SECTIONS && s < TK_STICK_COUNT;
    if (s >= 0 && s < TK_COUNT) {
      tclash |= tused[s];
      tused[s] = true;
    }
  }
  for (int s : direct) {
    from48 &= s >= TK_STICK_COUNT && s < TK_COUNT;
    if (s >= 0 && s < TK_COUNT) {
      tclash |= tused[s];
      tused[s] = true;
    }
  }
  expect("sec_ticks: the s_tick names lie in [8, 48)", below48, true);
  expect("sec_ticks: the names added in place lie in [48, 64)", from48, true);
  expect("sec_ticks: no two names share a slot", tclash, false);
  bool all48 = true;
  for (int s = 0; s < TK_STICK_COUNT; ++s) all48 &= tused[s];
  expect("sec_ticks: every slot below 48 is named", all48, true);
}

int main() {
  watchdog_cases();
  error_table_cases();
  slot_cases();
  if (fails) {
    std::printf("%d case(s) failed\n", fails);
    return 1;
  }
  std::printf("plan watch ok\n");
  return 0;
}
