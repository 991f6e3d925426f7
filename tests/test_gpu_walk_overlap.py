"""GPU: k_plan's step-start walk-ahead on the waves that idle through the wave-0 rules rounds (round 14).

A small warehouse of one-wide aisles, packed with agents, fires rule-3 swaps and 2-cycle rotations at every step: they
rewrite goals under the walkers. Every plan must equal the oracle's (records and goals), whatever runs the walk: the
waves beside wave 0 (default block of 256: three walker waves; 128: one; 1,024: fifteen) or PRE1 as before (a
one-wave block, TSW_AB_FLAGS bit 64, exit mode). TSW_AB_FLAGS 128 is planned as well: the bit chose between two sets of
walker waves while both were measured; only one is kept (all of waves 1..), so it now selects nothing and must
behave as 0. On the diagnostic library the counters of the "[k_plan] PRE1 publish" line say where the walks ran:
steps PRE1 walked, steps it left to the rules phase, and walks the waves beside wave 0 finished and published
there, counted by the wave that publishes.

The last case guards the walkers' (goal, table slot) pairing: a code stored under another goal's table would show
in next_hop_codes even if the plan never read it.
"""
import functools
import re

import numpy as np
import pytest

from oracle import OracleGraph
from p2p_distributed_tswap_amd import TSW_F_EXIT_MODE, TSW_F_LAZY_NEXTHOP, Planner, maps

W, H, N_AGENTS, N_TASKS, MAX_T = 24, 14, 70, 2000, 300
SEED = 6
STEPS = MAX_T + 1  # PRE1 sections of the plan: one per record, the last one's step ends at the horizon

# plan_debug_report (tsw_plan_host.hip) under TSW_PLAN_DEBUG:
#   "[k_plan] PRE1 publish us ... | walk-ahead steps in PRE1 %llu left to RULES %llu done in RULES %llu
#    walkers us %.0f wave 0 first %llu"
_RE_WALK = re.compile(r"\[k_plan\] PRE1 publish us .*\| walk-ahead steps in PRE1 (\d+) left to RULES (\d+) "
                      r"done in RULES (\d+) walkers us (\d+) wave 0 first (\d+)")


def aisle_map():
    """24 x 14: one-wide horizontal aisles on the even rows 0..10 between shelf rows, crossed by one-wide aisles at
    x = 0, 6, 12, 18 and 23; rows 12 and 13 are an open corridor."""
    rows = []
    for y in range(H):
        shelf = y % 2 == 1 and y < 12
        rows.append("".join("@" if shelf and x % 6 != 0 and x != W - 1 else "." for x in range(W)))
    return rows


@functools.lru_cache(maxsize=None)
def instance():
    """(rows, starts, tasks, oracle records, oracle goals): computed once, shared, never written to."""
    rows = aisle_map()
    starts, tasks = maps.make_instance(rows, N_AGENTS, N_TASKS, SEED)
    ref, rgoal = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, MAX_T, trace_goals=True)
    for a in (starts, tasks, ref, rgoal):
        a.setflags(write=False)
    return rows, starts, tasks, ref, rgoal


def rule_steps(ref, rgoal):
    """Per step (record t -> t + 1): some agent's goal changed while its state did not. The state machine changes a goal only
    together with the state (pickup reached, task assigned), so such a change is a rule-3 swap or a rule-4 rotation."""
    state = ref >> np.uint64(32)
    return np.any((rgoal[:, 1:] != rgoal[:, :-1]) & (state[:, 1:] == state[:, :-1]), axis=0)


def first_move_fires(rows, starts, tasks, ref, rgoal):
    """The records hide the rules of the first iteration in which anything moves (record 0 -> 1), so it is replayed
    through the oracle's tswap_step. Iteration 0 of the reference gives every idle agent, in index order, the nearest
    unused pickup (Manhattan, first of equals: tswap.rs:120-139); make_instance starts every agent on a pickup, so
    each gets the one under it, nothing moves and no rule can fire (every agent is at its goal, tswap.rs:181):
    that is record 0. In the next iteration every agent has reached its pickup and turns to its delivery cell, all
    states change (rule_steps sees nothing), and tswap_step runs on those goals: its rules fired iff the goals it
    leaves differ from the delivery cells. Record 1 checks the restatement."""
    px, py = tasks[:, 0].astype(np.int64), tasks[:, 1].astype(np.int64)
    used = np.zeros(len(tasks), dtype=bool)
    v0 = starts[:, 1].astype(np.uint32) * W + starts[:, 0].astype(np.uint32)
    gp = np.empty(len(starts), dtype=np.uint32)
    gd = np.empty(len(starts), dtype=np.uint32)
    for k, (x, y) in enumerate(starts.astype(np.int64)):
        d = np.where(used, np.iinfo(np.int64).max, np.abs(px - x) + np.abs(py - y))
        j = int(np.argmin(d))  # first of equals
        used[j] = True
        gp[k] = py[j] * W + px[j]
        gd[k] = int(tasks[j, 3]) * W + int(tasks[j, 2])
    assert np.array_equal(gp, v0) and np.array_equal(rgoal[:, 0], v0), "agents do not start on their pickups"
    v1, g1 = OracleGraph(maps.rows_to_array(rows)).step(v0, gd)
    x1, y1 = ref[:, 1] & np.uint64(0xFFFF), (ref[:, 1] >> np.uint64(16)) & np.uint64(0xFFFF)
    assert np.array_equal(g1, rgoal[:, 1]) and np.array_equal(v1, y1 * np.uint64(W) + x1), "iteration 1 restated wrongly"
    return bool(np.any(g1 != gd))


def test_instance_fires_rules_at_every_early_step():
    """CPU, oracle alone: the premise of the GPU cases. The task stream outlasts the horizon, the map is what the
    docstring says, and rules fire at every one of the first 100 steps in which agents move: step s takes record s
    to record s + 1, s = 0..99. (Before record 0 lies the reference's first iteration, in which every agent is given
    the pickup it stands on: nobody moves and no rule can fire, whatever the density.) Step 0 changes every state,
    which hides its firings from rule_steps, so it is replayed through the oracle's tswap_step (first_move_fires);
    steps 1.. come from the records — in fact every step of the horizon shows a firing."""
    rows, starts, tasks, ref, rgoal = instance()
    assert len(rows) == H and all(len(r) == W for r in rows)
    assert len(maps.largest_component(rows)) == sum(r.count(".") for r in rows)  # connected
    assert ref.shape == (N_AGENTS, MAX_T + 1)  # not finished at the horizon
    state = ref >> np.uint64(32)
    assert np.count_nonzero(state[:, -1] == state[0, 0]) < N_AGENTS // 2  # still busy: most agents hold a task
    assert first_move_fires(rows, starts, tasks, ref, rgoal), "no rule fired at step 0"
    fired = rule_steps(ref, rgoal)  # fired[s]: record s -> s + 1
    assert fired[1:101].all(), f"no rule fired at steps {np.flatnonzero(~fired[:101])[1:11]}"
    assert fired.sum() >= MAX_T - 5


def _plan(monkeypatch, capfd, diag=False, env=None, flags=0, keep=None):
    """One plan against the oracle; the walk counters (PRE1 steps, RULES steps, wave 0 first) on the diagnostic
    library. keep: called with the open planner after the plan."""
    rows, starts, tasks, ref, rgoal = instance()
    if diag:
        monkeypatch.setenv("TSW_PLAN_DEBUG", "1")
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, str(v))
        capfd.readouterr()
    with Planner(rows, flags=TSW_F_LAZY_NEXTHOP | flags, diag=diag) as p:
        rec, goal = p.plan_mapd_arrays(starts, tasks, MAX_T, trace_goals=True)
        st = p.stats()
        out = keep(p) if keep else None
    assert rec.shape == ref.shape
    bad = np.argwhere(rec != ref)
    assert bad.size == 0, f"records differ first at agent {bad[0][0]} t {bad[0][1]}"
    assert np.array_equal(goal, rgoal), "goals differ"
    assert st.get("watchdog_fires", 0) == 0
    if not diag:
        return None, out
    m = _RE_WALK.findall(capfd.readouterr().err)
    assert m, "no walk-ahead counters in the diagnostic output"
    pre1, left, done, us, first = (int(x) for x in m[-1])
    return dict(pre1=pre1, left=left, done=done, walkers_us=us, wave0_first=first), out


def _check_counters(d, overlapped):
    """pre1: steps whose walk PRE1 ran; left: steps PRE1 left to the rules phase (counted in PRE1); done: walks the
    walker waves finished there (counted by the wave that completes the walkers' count and publishes). Every step's
    PRE1 does one or the other, so pre1 + left == STEPS by construction; done == left is what shows that every walk
    left to the rules phase was armed, run by all walkers and published once — none lost, none doubled."""
    print(d)
    assert d["pre1"] + d["left"] == STEPS, d
    assert d["done"] == d["left"], d
    assert d["pre1"] + d["done"] == STEPS, d
    if overlapped:
        assert d["done"] > 0, d  # the overlapped path ran
        assert d["walkers_us"] > 0, d
        assert d["wave0_first"] <= d["done"], d
    else:
        assert d["left"] == 0 and d["done"] == 0 and d["walkers_us"] == 0 and d["wave0_first"] == 0, d


@pytest.mark.gpu
def test_product_default_block(monkeypatch, capfd):
    _plan(monkeypatch, capfd)


@pytest.mark.gpu
def test_product_exit_mode(monkeypatch, capfd):
    """TSW_F_EXIT_MODE: no concurrent workers, the walk stays in PRE1; the plan is the same."""
    _plan(monkeypatch, capfd, flags=TSW_F_EXIT_MODE)


@pytest.mark.gpu
@pytest.mark.parametrize("ab", [0, 64, 128], ids=["overlap", "in-pre1", "bit-128-unused"])
def test_diag_ab_flags(ab, monkeypatch, capfd):
    """Default block (256): three walker waves. Bit 64 keeps the parent's schedule; bit 128 selects nothing."""
    d, _ = _plan(monkeypatch, capfd, diag=True, env={"TSW_AB_FLAGS": ab})
    _check_counters(d, overlapped=ab != 64)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [64, 128, 1024])
def test_diag_block_sizes(block, monkeypatch, capfd):
    """128: one walker wave covers every agent; 1,024: fifteen walkers, most of them without an agent; 64: no walker,
    so the walk must stay in PRE1."""
    d, _ = _plan(monkeypatch, capfd, diag=True, env={"TSW_AB_FLAGS": 0, "TSW_PLAN_BLOCK": block})
    _check_counters(d, overlapped=block != 64)


@pytest.mark.gpu
def test_codes_stored_during_the_plan_are_their_goals(monkeypatch, capfd):
    """After the plan: every (free cell, goal) pair over the goals the plan used, from the context's store, against
    the oracle's first hops."""
    rows, _, _, _, rgoal = instance()
    og = OracleGraph(maps.rows_to_array(rows))
    cells = np.array([y * W + x for x, y in maps.largest_component(rows)], dtype=np.uint32)
    goals = np.unique(rgoal)

    def codes(p):
        st = np.tile(cells, goals.size)
        gl = np.repeat(goals.astype(np.uint32), cells.size)
        return p.next_hop_codes(st, gl).reshape(goals.size, cells.size)

    _, got = _plan(monkeypatch, capfd, keep=codes)
    for i, g in enumerate(goals):
        want = og.next_codes(int(g))[cells]
        bad = np.flatnonzero(got[i] != want)
        assert bad.size == 0, f"goal {g}: cell {cells[bad[0]]} holds code {got[i][bad[0]]}, oracle {want[bad[0]]}"
