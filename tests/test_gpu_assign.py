"""GPU: k_plan's K4 assignment scan (round 12: chunk list in LDS read with one lane per entry, batches of up
to 16 idle agents, lane-per-agent accept) at the smallest shapes where it can go wrong.

Every run compares plan_mapd_arrays' records and goals with OracleGraph.mapd. Each case runs on the product
library and on the diagnostic library with TSW_AB_FLAGS 0 (its counters say which path ran), 4 (one agent per
batch) and 32 (a scan list of 4 entries, so that small instances overflow it too).

tests/test_assign_scan_model.py restates the scan on the CPU and holds the mutants.
"""
import re

import numpy as np
import pytest

from oracle import OracleGraph
from p2p_distributed_tswap_amd import TSW_EINVAL, Planner, TswapError, maps

pytestmark = pytest.mark.gpu

# tsw_plan_assign.h: the scan's LDS list of (chunk, agent mask) entries lies in what the step's idle agents leave
# free of the 1,024-word `list` (two words an entry), or in SCAN_CAP entries of their own when that is less
LIST_CAP = 1024
SCAN_CAP = 64
SMALL_CAP = 4  # ... with TSW_AB_FLAGS bit 32 (diagnostic library)
KCH = 32       # tasks per chunk of the Morton index
ABATCH = 16    # widest batch

# product, then the diagnostic library with TSW_AB_FLAGS = 0 / 4 / 32
VARIANTS = [("product", None), ("diag", 0), ("diag-one", 4), ("diag-cap4", 32)]

# the two stderr lines of plan_debug_report (tsw_plan_host.hip) under TSW_PLAN_DEBUG that _diag() reads:
#   "[k_plan] assign us: ... | sections %llu batches %llu accepted %llu"
#   "[k_plan] assign scan us: ... | chunk-agent pairs %llu chunks %llu scanning waves %llu list rounds %llu | batch widths
#    1: %llu 2-4: %llu 5-8: %llu 9-16: %llu"
_RE_ASSIGN = re.compile(r"\[k_plan\] assign us: .*\| sections (\d+) batches (\d+) accepted (\d+)")
_RE_SCAN = re.compile(r"\[k_plan\] assign scan us: .*\| chunk-agent pairs (\d+) chunks (\d+) scanning waves (\d+) "
                      r"list rounds (\d+) \| batch widths 1: (\d+) 2-4: (\d+) 5-8: (\d+) 9-16: (\d+)")


def _diag(err: str) -> dict:
    """Counters of the call's LAST plan (the ticks accumulate over a context's calls; every test here makes one)."""
    a, s = _RE_ASSIGN.findall(err), _RE_SCAN.findall(err)
    assert a and s, "no assign lines in the diagnostic output"
    sec, bat, acc = (int(x) for x in a[-1])
    pairs, chunks, waves, rounds, w1, w4, w8, w16 = (int(x) for x in s[-1])
    return dict(sections=sec, batches=bat, accepted=acc, pairs=pairs, chunks=chunks, waves=waves, rounds=rounds,
                widths=(w1, w4, w8, w16))


def _run(rows, starts, tasks, max_t, variant, monkeypatch, capfd):
    """The plan on `variant`, checked against the oracle; the diagnostic counters (None on the product)."""
    name, flags = variant
    starts = np.asarray(starts, dtype=np.uint32).reshape(-1, 2)
    tasks = np.asarray(tasks, dtype=np.uint32).reshape(-1, 4)
    ref, rgoal = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, max_t, trace_goals=True)
    if flags is not None:
        monkeypatch.setenv("TSW_PLAN_DEBUG", "1")
        monkeypatch.setenv("TSW_AB_FLAGS", str(flags))
        capfd.readouterr()
    with Planner(rows, diag=flags is not None) as p:
        rec, goal = p.plan_mapd_arrays(starts, tasks, max_t, trace_goals=True)
        fires = p.stats().get("watchdog_fires", 0)
    assert rec.shape == ref.shape
    bad = np.argwhere(rec != ref)
    assert bad.size == 0, f"{name}: records differ first at agent {bad[0][0]} t {bad[0][1]}"
    assert np.array_equal(goal, rgoal), f"{name}: goals differ"
    assert fires == 0
    if flags is None:
        return None
    d = _diag(capfd.readouterr().err)
    if flags == 4:
        assert d["widths"][1:] == (0, 0, 0), d  # one agent per batch
        assert d["batches"] >= d["accepted"]
    return d


def _far_tasks(rows, m, seed):
    """m valid tasks (make_instance's stream)."""
    return maps.make_instance(rows, 1, m, seed)[1]


def _assigned_at_t0(rows, starts, tasks):
    """The oracle's t = 0 goals -> per agent the pickup cell id it was sent to."""
    _, g = OracleGraph(maps.rows_to_array(rows)).mapd(np.asarray(starts, np.uint32), np.asarray(tasks, np.uint32), 1,
                                                      trace_goals=True)
    return g[:, 0]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("m", [0, 1, 32, 33, 65])
def test_task_count_edges(m, variant, monkeypatch, capfd):
    """Tail-chunk padding (m = 1, 33, 65), exactly one chunk (32), no task at all; 12 agents, so with
    m < 12 the tasks run out inside the first batch."""
    rows = maps.random_map(24, 24, 0.15, 11)
    starts, tasks = maps.make_instance(rows, 12, max(m, 1), 11)
    d = _run(rows, starts, tasks[:m], 30, variant, monkeypatch, capfd)
    if d is not None and m >= 12 and variant[1] == 0:
        assert d["accepted"] >= 12 and d["widths"][3] >= 1, d  # the t = 0 burst ran as a batch wider than 8


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_fewer_tasks_than_idle_agents(variant, monkeypatch, capfd):
    """40 agents, 21 tasks: `unused` reaches 0 inside the second batch of t = 0, and stays 0 afterwards."""
    rows = maps.open_map(32, 32)
    starts, tasks = maps.make_instance(rows, 40, 21, 5)
    d = _run(rows, starts, tasks, 25, variant, monkeypatch, capfd)
    if d is not None:
        assert d["accepted"] == 21, d


def _tie_instance(piles):
    """Agent 0 at (0, 0); pickups (20, 0) and (0, 20) are both 20 away, Morton codes 272 and 544; `fill` far cells
    of (24..31, 8..12) lie between them in the Morton order, so the two sit in different chunks. Task 0 is at the
    Morton-LATER cell: the lower task index must win although its chunk is read later (or by another wave).
    piles > 1: that many chunks' worth of tasks at each of the two cells."""
    rows = maps.open_map(40, 40)
    fill = [(24 + k % 8, 8 + (k // 8) % 5) for k in range(40)]
    late, early = [(0, 20)] * (1 if piles == 1 else piles * KCH), [(20, 0)] * (1 if piles == 1 else piles * KCH)
    picks = late + fill + early
    tasks = [(x, y, 35, 35 - (k % 30)) for k, (x, y) in enumerate(picks)]
    starts = [(0, 0), (39, 39), (1, 0)]
    return rows, starts, tasks


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("piles", [1, 3])
def test_tie_across_chunks_lower_task_index_wins(piles, variant, monkeypatch, capfd):
    rows, starts, tasks = _tie_instance(piles)
    g0 = _assigned_at_t0(rows, starts, tasks)
    assert g0[0] == 20 * 40 + 0, "premise: the oracle sends agent 0 to task 0's cell (0, 20)"
    d = _run(rows, starts, tasks, 30, variant, monkeypatch, capfd)
    if d is not None and piles == 3 and variant[1] == 32:
        assert d["rounds"] > d["batches"], d  # 6 tied chunks against a list of 4


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_conflict_ring_width_drops_and_regrows(variant, monkeypatch, capfd):
    """48 idle agents (three batch widths) in rings around three pickup cells with six tasks each, far tasks for the
    rest: neighbours in agent order want the same task, so batches are cut at conflicts."""
    rows = maps.open_map(48, 48)
    ring = [(20 + dx, 20 + dy) for dx in range(-5, 6) for dy in range(-5, 6) if abs(dx) + abs(dy) in (3, 4, 5)]
    starts = ring[:48]
    assert len(starts) == 48 and len(set(starts)) == 48
    near = [(20, 20), (21, 20), (20, 21)] * 6
    tasks = [(x, y, 40, 2 + k) for k, (x, y) in enumerate(near)] + [tuple(t) for t in _far_tasks(rows, 60, 3)]
    d = _run(rows, starts, tasks, 20, variant, monkeypatch, capfd)
    if d is not None and variant[1] == 0:
        # conflicts: more batches at t = 0 than 48 / 16, and narrower ones among them
        assert d["batches"] > 3 and sum(d["widths"][:3]) > 0 and d["widths"][3] > 0, d


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[1]], ids=["product", "diag"])
@pytest.mark.parametrize("w,n,m", [(48, 200, 300), (64, 1100, 1500)], ids=["48x48-200", "64x64-1100"])
def test_t0_burst_wider_than_a_batch(w, n, m, variant, monkeypatch, capfd):
    """Every agent idle at t = 0; with 1,100 agents the outer loop over blocks of agents runs twice, and its first
    pass fills `list` with idle agents, so the scan's list is the SCAN_CAP entries of its own."""
    rows = maps.random_map(w, w, 0.1, 21)
    starts, tasks = maps.make_instance(rows, n, m, 21)
    d = _run(rows, starts, tasks, 3, variant, monkeypatch, capfd)
    if d is not None:
        assert d["accepted"] >= n and d["widths"][3] > 0, d


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[1], VARIANTS[2]], ids=["product", "diag", "diag-one"])
@pytest.mark.parametrize("lone", [False, True], ids=["all-agents", "one-agent"])
def test_list_overflow(lone, variant, monkeypatch, capfd):
    """(LIST_CAP / 2 + 6) chunks' worth of tasks at one pickup cell: more chunks tie than the list holds beside
    the idle agents (at most LIST_CAP / 2 entries), so the scan takes a second round over the list. `lone`: only agent 3 is near the pile; the others stand
    on pickups of their own, so their bounds keep the pile's chunks out of their masks."""
    rows = maps.open_map(40, 40)
    npile = (LIST_CAP // 2 + 6) * KCH
    if lone:
        # the pile at (3, 3), agent 3 beside it; the other agents stand at (32.., 0) on pickups of their own, which
        # follow the whole pile in the Morton order (x >= 32) and so fill a chunk of their own, 7 cells wide: the
        # pile is at least 32 away from them, beyond their bound
        tasks = [(3, 3, 2 + k % 30, 6 + (k // 30) % 30) for k in range(npile)]
        starts = [(32 + i, 0) for i in range(8)]
        starts[3] = (3, 4)
        tasks += [(x, y, x, y + 3) for i, (x, y) in enumerate(starts) if i != 3]
    else:
        tasks = [(30, 30, 2 + k % 30, 2 + (k // 30) % 30) for k in range(npile)]
        starts = [(28 + i % 5, 26 + i // 5) for i in range(20) if (28 + i % 5, 26 + i // 5) != (30, 30)]
    # lone: 3 steps, in which nobody is idle a second time (the deliveries are 3 cells away): one batch at t = 0
    d = _run(rows, starts, tasks, 3 if lone else 12, variant, monkeypatch, capfd)
    if d is not None and variant[1] == 0:
        assert d["rounds"] > d["batches"], d  # the overflow rounds ran
        if lone:
            # agent 3's mask alone holds the pile's chunks: pairs ~ chunks, far fewer than chunks * agents
            assert d["pairs"] < 2 * d["chunks"] + 8 * len(starts), d


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[1]], ids=["product", "diag"])
def test_strided_chunks(variant, monkeypatch, capfd):
    """70,000 tasks = 2,188 chunks: more than two per thread of the block, so the third comes from the strided
    path (re-read from the index for every use). A 32x32 grid has at most 1,024 pickup cells: long runs of chunks
    tie at every agent's nearest cell, and the list overflows as well."""
    rows = maps.open_map(32, 32)
    starts, tasks = maps.make_instance(rows, 6, 70000, 17)
    d = _run(rows, starts, tasks, 12, variant, monkeypatch, capfd)
    if d is not None:
        assert d["accepted"] >= 6 and d["chunks"] >= d["batches"], d


def _bad_cell_instance(kind):
    """16 agents in a column, all idle at t = 0 (one batch of 16). Agent i stands on the pickup of task i, whose
    delivery is the cell to its right, so it is idle again at t = 2. Agent 8's task is 2 cells away instead:
    `pickup`: that pickup cell is blocked -> the reference panics when agent 8 is assigned it at t = 0, in the middle
    of the batch (tswap.rs:136). `delivery`: its delivery is off the grid -> the reference panics when agent 8 reaches
    the pickup at t = 2 (tswap.rs:112), in the step in which the other 15 agents are idle again."""
    w = 40
    grid = [["."] * w for _ in range(40)]
    starts = [(4, 2 * i + 2) for i in range(16)]
    tasks = []
    for i, (x, y) in enumerate(starts):
        if i != 8:
            tasks.append((x, y, x + 1, y))
        elif kind == "pickup":
            grid[y][x + 2] = "@"
            tasks.append((x + 2, y, x + 9, y))
        else:
            tasks.append((x + 2, y, 1000, 1000))
    rows = ["".join(r) for r in grid]
    tasks += [(20 + k % 16, 3 + k // 16, 30, 3 + k) for k in range(32)]  # what the idle agents of t = 2 take
    return rows, starts, tasks


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("kind", ["pickup", "delivery"])
def test_bad_cell_in_the_middle_of_a_wide_batch(kind, variant, monkeypatch, capfd):
    rows, starts, tasks = _bad_cell_instance(kind)
    starts, tasks = np.asarray(starts, np.uint32), np.asarray(tasks, np.uint32)
    og = OracleGraph(maps.rows_to_array(rows))
    with pytest.raises(ValueError):
        og.mapd(starts, tasks, 10)
    # premise: without agent 8's task nothing fails, and up to the failing step the plan is the oracle's
    ok_until = 0 if kind == "pickup" else 1
    if variant[1] is not None:
        monkeypatch.setenv("TSW_PLAN_DEBUG", "1")
        monkeypatch.setenv("TSW_AB_FLAGS", str(variant[1]))
    with Planner(rows, diag=variant[1] is not None) as p:
        with pytest.raises(TswapError) as ei:
            p.plan_mapd_arrays(starts, tasks, 10)
        # the message names the reference's panic site: pickup lookup :136, delivery lookup :112
        assert ei.value.code == TSW_EINVAL and ("tswap.rs:136" if kind == "pickup" else "tswap.rs:112") in str(ei.value)
        if ok_until:  # the steps before the panic are planned as the reference plans them
            ref, rgoal = og.mapd(starts, tasks, ok_until, trace_goals=True)
            rec, goal = p.plan_mapd_arrays(starts, tasks, ok_until, trace_goals=True)
            assert np.array_equal(rec, ref) and np.array_equal(goal, rgoal)
        # the context stays usable, and the same step without the bad task is exact
        good = np.delete(tasks, 8, axis=0)
        ref, rgoal = og.mapd(starts, good, 10, trace_goals=True)
        rec, goal = p.plan_mapd_arrays(starts, good, 10, trace_goals=True)
        assert np.array_equal(rec, ref) and np.array_equal(goal, rgoal)
