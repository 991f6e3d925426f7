"""GPU: tsw_plan_mapd_online (tasks with release times, run as k_plan segments) against the CPU model
(tests/online_model.py), bit for bit: records, goals and T. Every case asserts from the model's counters that it
takes the path it is there for (segments split, columns held, tasks never released). Grids are 8x8 to 32x32 and
max_t <= 128, so a case takes well under a second apart from a context's first table build."""
import ctypes

import numpy as np
import pytest

from online_model import online_mapd
from oracle import OracleGraph
from p2p_distributed_tswap_amd import (TSW_EINVAL, TSW_F_EAGER_NEXTHOP, TSW_F_EXIT_MODE, TSW_HOST_ASTAR_OFF, TSW_OK, Planner,
                                       TswapError, _Point, _Rec, _Task, maps)

pytestmark = pytest.mark.gpu

SENT64 = np.uint64(0xABABABABABABABAB)
SENT32 = np.uint32(0xABABABAB)


def raw_online(p, starts, tasks, rel, max_t):
    """The C entry point itself on sentinel-filled outputs: (rc, out (n, max_t + 1) raw u64, goals, T)."""
    starts = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1, 2)
    tasks = np.ascontiguousarray(tasks, dtype=np.uint32).reshape(-1, 4)
    n, m = len(starts), len(tasks)
    out = np.full((max(n, 1), max_t + 1), SENT64, dtype=np.uint64)
    goals = np.full((max(n, 1), max_t + 1), SENT32, dtype=np.uint32)
    relp = None
    if rel is not None:
        rel = np.ascontiguousarray(rel, dtype=np.uint32)
        relp = rel.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    T = ctypes.c_uint32(0)
    rc = p._lib.tsw_plan_mapd_online(p._ctx, starts.ctypes.data_as(ctypes.POINTER(_Point)), n,
                                     tasks.ctypes.data_as(ctypes.POINTER(_Task)), relp, m, max_t,
                                     out.ctypes.data_as(ctypes.POINTER(_Rec)),
                                     goals.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(T))
    return rc, out, goals, T.value


def model(rows, starts, tasks, rel, max_t):
    return online_mapd(maps.rows_to_array(rows), starts, tasks, rel, max_t)


def check(p, rows, starts, tasks, rel, max_t, ref=None):
    """The library's online plan equals the model's; returns the model's (rec, goals, T, counters)."""
    ref = ref or model(rows, starts, tasks, rel, max_t)
    rec, goals = p.plan_mapd_online(starts, tasks, rel, max_t, trace_goals=True)
    assert rec.shape == ref[0].shape, (rec.shape, ref[0].shape)
    assert rec.shape[1] == ref[2]
    assert np.array_equal(rec, ref[0])
    assert np.array_equal(goals, ref[1])
    return ref


# ---- instances -----------------------------------------------------------------------------------------------
ROWS16 = maps.random_map(16, 16, 0.15, 0x0516)
ROWS24 = maps.random_map(24, 24, 0.2, 0x0524)
ROWS32 = maps.random_map(32, 32, 0.2, 0x0532)
OPEN12 = maps.open_map(12, 12)


@pytest.fixture(scope="module")
def p16():
    with Planner(ROWS16) as p:
        yield p


@pytest.fixture(scope="module")
def p24():
    with Planner(ROWS24) as p:
        yield p


@pytest.fixture(scope="module")
def p32():
    with Planner(ROWS32) as p:
        yield p


@pytest.fixture(scope="module")
def popen():
    with Planner(OPEN12) as p:
        yield p


def gap_instance():
    """Six agents, six tasks at 0 and six more after a gap (well-formed: no task endpoint is a parking cell)."""
    return maps.make_wf_instance(ROWS16, 6, 12, 0x6A9)


# ---- equivalence -----------------------------------------------------------------------------------------------
def test_release_zero_and_null_equal_the_trace_plan(p16):
    starts, tasks = maps.make_instance(ROWS16, 10, 20, 7)
    base, bgoals = p16.plan_mapd_arrays(starts, tasks, 128, trace_goals=True)
    ref = check(p16, ROWS16, starts, tasks, np.zeros(20, dtype=np.uint32), 128)
    assert ref[3]["segments"] == 1 and ref[3]["never_released"] == 0
    assert np.array_equal(ref[0], base) and np.array_equal(ref[1], bgoals)
    rc, out, goals, T = raw_online(p16, starts, tasks, None, 128)  # release == NULL through the C call
    assert rc == TSW_OK and T == base.shape[1]
    assert np.array_equal(out[:, :T] & np.uint64(0xFFFFFFFFFF), base) and np.array_equal(goals[:, :T], bgoals)


# ---- one task per step -------------------------------------------------------------------------------------------
def test_one_task_released_per_step(p24):
    starts, tasks = maps.make_wf_instance(ROWS24, 12, 64, 0x24)
    rel = np.arange(1, 65, dtype=np.uint32)
    ref = check(p24, ROWS24, starts, tasks, rel, 128)
    assert ref[3]["segments"] >= 60 and ref[3]["segments"] == 65


# ---- a gap between two batches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("second,max_t", [(70, 128), (300, 100)])
def test_gap_between_batches_holds_the_column(p16, second, max_t):
    starts, tasks = gap_instance()
    rel = np.array([0] * 6 + [second] * 6, dtype=np.uint32)
    rec, goals, T, cnt = check(p16, ROWS16, starts, tasks, rel, max_t)
    assert cnt["held"] >= 10
    if second > max_t:  # the gap runs past max_t: the hold is capped there
        assert cnt["never_released"] == 6 and cnt["segments"] == 1 and T == max_t + 1
        assert (rec[:, -1] >> np.uint64(32) == 3).all()
    else:
        assert cnt["segments"] == 2 and T > second and cnt["never_released"] == 0
        assert (rec[:, second:] >> np.uint64(32) != 3).any()  # the second batch was carried


@pytest.mark.parametrize("seed,second,max_t", [(26, 90, 128), (53, 90, 128), (9, 300, 100)])
def test_idle_agents_off_their_goals_walk_on_before_the_hold(p16, seed, second, max_t):
    # k_plan stops when every visible task is used and every agent idle, but a goal swap can leave an idle agent
    # off its goal: the fleet walks on (a column per launch) until it rests, and only then is the column held
    starts, tasks = maps.make_instance(ROWS16, 8, 12, seed)  # endpoints may be parking cells: swaps with resting agents
    rel = np.array([0] * 6 + [second] * 6, dtype=np.uint32)
    rec, goals, T, cnt = check(p16, ROWS16, starts, tasks, rel, max_t)
    assert cnt["idle_walking"] >= 1 and cnt["held"] >= 10


def test_release_at_max_t_and_one_past_it(p16):
    starts, tasks = maps.make_wf_instance(ROWS16, 5, 8, 0x3A7)
    max_t = 40
    rel = np.array([0, 0, 0, 0, 0, 0, max_t, max_t + 1], dtype=np.uint32)
    rec, goals, T, cnt = check(p16, ROWS16, starts, tasks, rel, max_t)
    assert cnt["segments"] == 2 and cnt["never_released"] == 1 and T == max_t + 1
    assert cnt["held"] >= 1  # the first batch was done before max_t: the fleet waited for the late task
    assert (rec[:, max_t] >> np.uint64(32) == 0).any()  # ... and took it in the last column


# ---- the choice among visible tasks --------------------------------------------------------------------------------
def test_release_order_does_not_reorder_equal_distance_tasks(popen):
    # two agents, pickups on the diamonds of radius 2 around them (all ties): the lowest index among the VISIBLE wins
    starts = np.array([[3, 5], [8, 5]], dtype=np.uint32)
    pk = [(1, 5), (5, 5), (3, 3), (3, 7), (10, 5), (6, 5), (8, 3), (8, 7)]
    dl = [(0, 0), (11, 11), (0, 11), (11, 0), (5, 0), (5, 11), (0, 6), (11, 6)]
    tasks = np.array([[*a, *b] for a, b in zip(pk, dl)], dtype=np.uint32)
    rel = np.array([9, 0, 30, 0, 9, 30, 0, 9], dtype=np.uint32)  # not monotone in the task index
    assert (np.diff(rel.astype(np.int64)) < 0).any()
    rec, goals, T, cnt = check(popen, OPEN12, starts, tasks, rel, 128)
    assert cnt["segments"] == 3
    # at t = 0 agent 0 sees tasks 1, 3, 6: 1 and 3 tie at distance 2, the lower index wins
    w = 12
    assert goals[0, 0] == 5 * w + 5


def test_duplicate_pickup_cells(p16):
    starts, tasks = maps.make_wf_instance(ROWS16, 6, 16, 0xD0B)
    tasks[4:8, :2] = tasks[0, :2]  # five tasks share one pickup cell, released at different times
    tasks[9, :2] = tasks[8, :2]
    rel = np.array([0, 0, 0, 0, 6, 0, 6, 12, 0, 12, 3, 3, 0, 20, 20, 0], dtype=np.uint32)
    ref = check(p16, ROWS16, starts, tasks, rel, 128)
    assert ref[3]["segments"] == 5


# ---- the release kernel's edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 257])
def test_release_kernel_edges(p32, k):
    # ~600 tasks with pickups clustered in an 8x8 window (so a release lands many in the same 32-entry chunks),
    # k of them released in one epoch at t = 3
    n, m, max_t = 24, 600, 40
    starts, far = maps.make_wf_instance(ROWS32, n, m, 0x600)
    _, near = maps.make_wf_instance(ROWS32, n, m, 0x601, window=(12, 12, 8, 8))
    tasks = far.copy()
    tasks[:, :2] = near[:, :2]
    r = maps.SplitMix64(0x5EED + k)
    idx = list(range(m))
    r.shuffle(idx)
    rel = np.zeros(m, dtype=np.uint32)
    rel[idx[:k]] = 3
    rel[idx[k:k + 300]] = max_t + 50  # most of the rest stay hidden, so the released ones are wanted at once
    rec, goals, T, cnt = check(p32, ROWS32, starts, tasks, rel, max_t)
    assert cnt["segments"] == 2 and cnt["never_released"] == 300 and T == max_t + 1


# ---- the hold kernel's edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("gap", [1, 100])
def test_hold_kernel_edges(p32, n, gap):
    starts, tasks = maps.make_wf_instance(ROWS32, n, 8, 0x401D + n)
    rel = np.full(8, gap + 1, dtype=np.uint32)  # column 0 is planned, columns 1 .. gap repeat it
    rec, goals, T, cnt = check(p32, ROWS32, starts, tasks, rel, 128)
    assert cnt["held"] == gap and cnt["segments"] == 2 and T > gap + 1
    assert (rec[:, :gap + 1] == rec[:, :1]).all()


# ---- edge shapes ---------------------------------------------------------------------------------------------------
def test_no_agents_no_tasks_duplicate_starts(p16):
    starts, tasks = maps.make_wf_instance(ROWS16, 6, 10, 0xE0)
    rel = np.array([0, 2, 2, 5, 0, 9, 9, 14, 1, 30], dtype=np.uint32)
    # n = 0: nobody takes a task, the run goes to max_t
    rec, goals, T, cnt = check(p16, ROWS16, starts[:0], tasks, rel, 12)
    assert rec.shape == (0, 13) and cnt["never_released"] == 2 and cnt["segments"] == 5
    # m = 0: one column
    rec, goals, T, cnt = check(p16, ROWS16, starts, tasks[:0], np.zeros(0, dtype=np.uint32), 12)
    assert T == 1 and cnt["segments"] == 1
    # duplicate starts: the serial-movement path
    dup = starts.copy()
    dup[1] = dup[0]
    dup[4] = dup[3]
    rec, goals, T, cnt = check(p16, ROWS16, dup, tasks, rel, 64)
    assert cnt["segments"] == 7


# ---- context options -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(flags=TSW_F_EXIT_MODE), dict(flags=TSW_F_EAGER_NEXTHOP),
                                  dict(host_astar=TSW_HOST_ASTAR_OFF)], ids=["exit_mode", "eager", "no_host_astar"])
def test_context_options_give_the_same_plan(p16, opts):
    starts, tasks = maps.make_wf_instance(ROWS16, 8, 14, 0x0F7)
    rel = np.array([0, 0, 0, 4, 4, 9, 9, 9, 60, 60, 61, 62, 0, 60], dtype=np.uint32)
    ref = check(p16, ROWS16, starts, tasks, rel, 128)
    assert ref[3]["segments"] == 6 and ref[3]["held"] >= 1
    with Planner(ROWS16, **opts) as q:
        check(q, ROWS16, starts, tasks, rel, 128, ref=ref)


# ---- lazy bad cells ------------------------------------------------------------------------------------------------
def test_bad_pickup_fails_only_when_released(p16):
    starts, tasks = maps.make_wf_instance(ROWS16, 4, 3, 0xBAD)
    blocked = [(x, y) for y, r in enumerate(ROWS16) for x, ch in enumerate(r) if ch == "@"]
    tasks[2, :2] = blocked[0]
    max_t = 60
    rel = np.array([0, 0, 5], dtype=np.uint32)
    with pytest.raises(ValueError):
        model(ROWS16, starts, tasks, rel, max_t)
    with pytest.raises(TswapError) as ei:
        p16.plan_mapd_online(starts, tasks, rel, max_t)
    assert ei.value.code == TSW_EINVAL
    # never released: never looked up
    rel[2] = max_t + 1
    rec, goals, T, cnt = check(p16, ROWS16, starts, tasks, rel, max_t)
    assert cnt["never_released"] == 1 and T == max_t + 1
    # the context works after the failure
    good, gtasks = maps.make_instance(ROWS16, 10, 20, 7)
    rec, goals = p16.plan_mapd_arrays(good, gtasks, 128, trace_goals=True)
    ref, rgoals = OracleGraph(maps.rows_to_array(ROWS16)).mapd(good, gtasks, 128, trace_goals=True)
    assert np.array_equal(rec, ref) and np.array_equal(goals, rgoals)


# ---- context state -------------------------------------------------------------------------------------------------
def test_context_state_across_calls(p16):
    starts, tasks = maps.make_wf_instance(ROWS16, 8, 14, 0x57A)
    rel = np.array([0, 3, 0, 3, 7, 7, 0, 40, 40, 41, 0, 12, 12, 90], dtype=np.uint32)
    a = p16.plan_mapd_online(starts, tasks, rel, 128, trace_goals=True)
    b = p16.plan_mapd_online(starts, tasks, rel, 128, trace_goals=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    after = p16.plan_mapd_arrays(starts, tasks, 128, trace_goals=True)
    with Planner(ROWS16) as fresh:
        first = fresh.plan_mapd_arrays(starts, tasks, 128, trace_goals=True)
    assert np.array_equal(after[0], first[0]) and np.array_equal(after[1], first[1])


# ---- untouched output ----------------------------------------------------------------------------------------------
def test_columns_from_T_on_are_untouched(p16):
    starts, tasks = gap_instance()
    rel = np.array([0] * 6 + [45] * 6, dtype=np.uint32)
    ref = model(ROWS16, starts, tasks, rel, 128)
    T = ref[2]
    assert ref[3]["held"] >= 1 and T < 128
    rc, out, goals, gT = raw_online(p16, starts, tasks, rel, 128)
    assert rc == TSW_OK and gT == T
    assert np.array_equal(out[:, :T] & np.uint64(0xFFFFFFFFFF), ref[0]) and np.array_equal(goals[:, :T], ref[1])
    assert (out[:, :T] >> np.uint64(40) == 0).all()  # the records' padding bytes are written as zero
    assert (out[:, T:] == SENT64).all() and (goals[:, T:] == SENT32).all()
