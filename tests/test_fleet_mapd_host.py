"""CPU: the decentralized MAPD run (tsw_fleet_mapd) is declared in every mirror of the C ABI without an ABI
bump, the scan form of its dispatch (what the kernels compute) equals the sequential loop of the header,
and the plain-Python model of the run (fleet_mapd_model.py) ends the hand-made cases the way the header
says and the table cases the way the GPU comparison relies on."""
import ctypes
import os
import re

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg

import fleet_mapd_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fleet_mapd_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tswap.h")).read()
    rs = open(os.path.join(ROOT, "rust", "tswap-amd-sys", "src", "lib.rs")).read()
    assert "tsw_fleet_mapd" in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint tsw_fleet_mapd\(tsw_ctx \*ctx, const tsw_point \*starts", hdr)
    assert re.search(r"pub fn tsw_fleet_mapd\(ctx: \*mut TswCtx", rs)
    assert hasattr(pkg.Planner, "fleet_mapd")
    assert re.search(r"#define TSW_ABI_VERSION 8\b", hdr)  # a function was added, nothing else changed
    assert "agent.rs:859-888" in hdr  # the header says where the model departs from the reference
    if os.path.exists(pkg.LIB_PATH):
        for path in (pkg.LIB_PATH, pkg.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), "tsw_fleet_mapd"), path


# ---- the dispatch: scan form == sequential loop -------------------------------------------------------

def _random_state(rng, n, m, nxt, p_arrived):
    """A reachable-looking stage-1 input: busy agents hold distinct tasks below `nxt`, some have arrived."""
    ncell = 4096
    pick = rng.randint(0, ncell, m).astype(np.uint32)
    dlv = rng.randint(0, ncell, m).astype(np.uint32)
    st = rng.randint(0, 3, n).astype(np.uint32) if nxt else np.zeros(n, dtype=np.uint32)
    busy = np.flatnonzero(st != mm.IDLE)
    if busy.size > nxt:  # more busy agents than tasks handed out: the surplus is idle
        st[busy[nxt:]] = mm.IDLE
        busy = busy[:nxt]
    tk = np.full(n, mm.NONE, dtype=np.uint32)
    tk[busy] = rng.permutation(nxt)[:busy.size]
    v = rng.randint(0, ncell, n).astype(np.uint32)
    g = v.copy()  # an idle agent's goal is its own cell
    g[busy] = np.where(st[busy] == mm.TO_PICKUP, pick[tk[busy]], dlv[tk[busy]])
    arrived = busy[rng.rand(busy.size) < p_arrived]
    v[arrived] = g[arrived]
    return v, g, st, tk, pick, dlv


def _both_forms(v, g, st, tk, nxt, pick, dlv):
    a = [x.copy() for x in (g, st, tk)]
    b = [x.copy() for x in (g, st, tk)]
    na, ca, _ = mm.task_phase(v, *a, nxt, pick, dlv)
    nb, cb = mm.task_phase_scan(v, *b, nxt, pick, dlv)
    return (na, ca, a), (nb, cb, b)


@pytest.mark.parametrize("seed", range(12))
def test_scan_dispatch_equals_sequential_loop(seed):
    rng = np.random.RandomState(seed)
    n = int(rng.choice([1, 5, 64, 257, 700]))
    m = int(rng.choice([0, 1, n // 2, n, 3 * n]))
    nxt = int(rng.randint(0, m + 1))
    v, g, st, tk, pick, dlv = _random_state(rng, n, m, nxt, 0.5)
    (na, ca, a), (nb, cb, b) = _both_forms(v, g, st, tk, nxt, pick, dlv)
    assert (na, ca) == (nb, cb)
    for x, y, name in zip(a, b, ("g", "st", "tk")):
        assert np.array_equal(x, y), name


def test_scan_dispatch_with_next_reaching_m_inside_the_fleet():
    """300 agents, 40 of them carrying and arrived, 100 tasks of which 60 are out: the 40 that go idle and
    the idle rest compete for the 40 open tasks, which end inside the fleet."""
    rng = np.random.RandomState(100)
    n, m, nxt = 300, 100, 60
    v, g, st, tk, pick, dlv = _random_state(rng, n, m, nxt, 1.0)
    (na, ca, a), (nb, cb, b) = _both_forms(v, g, st, tk, nxt, pick, dlv)
    assert na == nb == m and ca and cb
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    g1, st1, tk1 = a
    taken = np.sort(tk1[(st1 == mm.TO_PICKUP) & (tk1 >= nxt)])
    assert taken.tolist() == list(range(nxt, m))  # each open task once, in ascending agent index
    assert (st1 == mm.IDLE).sum() > 0 and np.all(tk1[st1 == mm.IDLE] == mm.NONE)
    holders = np.flatnonzero((st1 == mm.TO_PICKUP) & (tk1 >= nxt))
    assert np.all(np.diff(tk1[holders]) == 1) and holders.max() < np.flatnonzero(st1 == mm.IDLE).min()
    # an agent that delivered (TO_DELIVERY, arrived) went idle and took a task in the same step
    again = np.flatnonzero((st == mm.TO_DELIVERY) & (st1 == mm.TO_PICKUP))
    assert again.size > 0 and np.all(tk1[again] != tk[again]) and np.all(g1[again] == pick[tk1[again]])


def test_an_agent_just_given_a_task_is_not_checked_again():
    """Pickup on the agent's own cell: the step that hands the task out leaves it TO_PICKUP."""
    v = np.array([7], dtype=np.uint32)
    g, st, tk = v.copy(), np.zeros(1, dtype=np.uint32), np.full(1, mm.NONE, dtype=np.uint32)
    pick, dlv = np.array([7], dtype=np.uint32), np.array([9], dtype=np.uint32)
    for form in (mm.task_phase, mm.task_phase_scan):
        a = [g.copy(), st.copy(), tk.copy()]
        assert form(v, *a, 0, pick, dlv)[:2] == (1, True)
        assert a[0][0] == 7 and a[1][0] == mm.TO_PICKUP and a[2][0] == 0


# ---- the ending rules on hand-made inputs -------------------------------------------------------------

def _states(run):
    return (run.rec >> np.uint64(32)).astype(np.int64)


def _xy(run):
    return (run.rec & np.uint64(0xFFFF)).astype(np.int64), ((run.rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)


def test_no_tasks_gives_one_column():
    run = mm.run_case("no-tasks")
    assert (run.T, run.stalled, run.next) == (1, False, 0)
    assert np.all(_states(run) == mm.REC_IDLE) and np.all(run.tasks == mm.NONE)
    x, y = _xy(run)
    assert x[:, 0].tolist() == [0, 3] and y[:, 0].tolist() == [0, 2]
    assert run.goals[:, 0].tolist() == [0, 2 * 6 + 3]  # g = v


def test_max_t_zero_gives_one_column():
    run = mm.run_case("max_t-0")
    assert (run.T, run.stalled, run.next) == (1, False, 2)
    assert np.all(_states(run) == mm.PICKING) and run.tasks[:, 0].tolist() == [0, 1]
    x, y = _xy(run)  # column 0 is the state after the first tick: one cell towards the pickup
    assert (np.abs(x[:, 0] - [0, 3]) + np.abs(y[:, 0] - [0, 2])).tolist() == [1, 1]


def test_pickup_equal_to_delivery():
    run = mm.run_case("pickup-is-delivery")
    s = _states(run)[0]
    assert not run.stalled and run.delivered == 2 and s[-1] == mm.REC_IDLE
    # three steps to (2, 1); the step after the arrival turns to TO_DELIVERY at its goal: DELIVERED,
    # never CARRYING; the step after that takes task 1
    assert s[:5].tolist() == [mm.PICKING] * 3 + [mm.DELIVERED, mm.PICKING]
    assert run.tasks[0, :5].tolist() == [0, 0, 0, 0, 1]


def test_pickup_on_the_start_cell():
    run = mm.run_case("pickup-on-start")
    s = _states(run)
    x, y = _xy(run)
    # agent 0 is handed task 0 on its own cell: PICKING there in column 0, CARRYING one cell on in column 1
    assert s[0, :2].tolist() == [mm.PICKING, mm.CARRYING] and (x[0, 0], y[0, 0]) == (1, 1)
    assert abs(x[0, 1] - 1) + abs(y[0, 1] - 1) == 1
    assert not run.stalled and run.delivered == 2 and np.all(s[:, -1] == mm.REC_IDLE)


def test_fewer_tasks_than_agents_leaves_the_surplus_idle():
    run = mm.run_case("fewer-tasks")
    s = _states(run)
    assert not run.stalled and run.next == 2 and run.delivered == 2
    assert np.all(s[2:] == mm.REC_IDLE) and np.all(run.tasks[2:] == mm.NONE)
    assert np.all(run.goals[2] == 5 * 6) and np.all(run.goals[3] == 5 * 6 + 5)  # g = v all along
    x, y = _xy(run)
    assert np.all(x[2] == 0) and np.all(y[2] == 5) and np.all(x[3] == 5) and np.all(y[3] == 5)


# ---- the table cases end the way their row names ------------------------------------------------------

@pytest.mark.parametrize("name", list(mm.CASES) + list(mm.HAND_CASES))
def test_model_ends_each_case_as_named(name):
    rows, starts, tasks, r, max_t, ending = mm.instance(name)
    run = mm.run_case(name)
    assert mm.ending(run, max_t) == ending
    assert run.rec.shape == run.goals.shape == run.tasks.shape == (starts.shape[0], run.T)
    assert 1 <= run.T <= max_t + 1
    if ending == "normal":
        assert run.next == run.delivered == tasks.shape[0]
    elif ending == "stalled":
        assert run.next < tasks.shape[0] or run.delivered < run.next
    else:
        assert run.T == max_t + 1
    # goals stay inside starts + pickups + deliveries: one table build covers the run
    W = len(rows[0])
    cells = set(mm.cells_of(starts, W).tolist()) | set(mm.cells_of(tasks[:, :2], W).tolist()) | set(
        mm.cells_of(tasks[:, 2:], W).tolist())
    assert set(np.unique(run.goals).tolist()) <= cells


def test_table_cases_cover_what_they_are_for():
    assert {e for _, _, e in mm.CASES.values()} == {"normal", "stalled", "horizon"}
    assert mm.run_case("open8").colocated > 0  # collisions on the way
    d = mm.run_case("dispatch3000")
    assert d.next == 2000 and np.all(d.tasks[2000:] == mm.NONE) and np.all(d.tasks[:2000, 0] == np.arange(2000))
    w = mm.run_case("warehouse")
    assert w.next > 300  # all 300 dispatched in step 0, and re-dispatch after a delivery
