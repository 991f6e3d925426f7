"""GPU: tsw_fleet_mapd, the MAPD run on the lock-step decentralized tick. Every comparison is records,
goals, tasks, T and stalled bit-equal to the CPU model (fleet_mapd_model.run_model: the sequential task
phase + brute-force lists + the oracle's decisions + apply_model), on cases that end in each of the three
ways; then the documented edges: NULL traces, untouched columns, the up-front TSW_EINVAL checks, the
composition with Planner.fleet_run and the shared device buffers."""
import ctypes

import numpy as np
import pytest

from p2p_distributed_tswap_amd import Planner, TswapError, maps, TSW_EINVAL, TSW_OK
from p2p_distributed_tswap_amd import _Point, _Rec, _Task

import fleet_cases as fc
import fleet_mapd_model as mm
import fleet_run_model as fm

pytestmark = pytest.mark.gpu

_U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xDEADBEEF
FILL64 = 0xDEADBEEFDEADBEEF


@pytest.fixture(scope="module")
def planners():
    """One context per map for the whole module (tables stay warm between tests)."""
    made = {}

    def get(rows):
        key = tuple(rows)
        if key not in made:
            made[key] = Planner(rows)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def _raw(p, starts, tasks, r, max_t, trace=True, with_stalled=True):
    """The C entry point on sentinel-filled outputs: (rc, out, goals, tasks, T, stalled)."""
    starts = np.ascontiguousarray(starts, dtype=np.uint32).reshape(-1, 2)
    tasks = np.ascontiguousarray(tasks, dtype=np.uint32).reshape(-1, 4)
    n = starts.shape[0]
    cols = max_t + 1 if max_t <= 1 << 20 else 1
    out = np.full((n, cols), FILL64, dtype=np.uint64)
    go = np.full((n, cols), FILL, dtype=np.uint32)
    to = np.full((n, cols), FILL, dtype=np.uint32)
    T, stalled = ctypes.c_uint32(FILL), ctypes.c_uint32(FILL)
    rc = p._lib.tsw_fleet_mapd(p._ctx, starts.ctypes.data_as(ctypes.POINTER(_Point)), n,
                               tasks.ctypes.data_as(ctypes.POINTER(_Task)), tasks.shape[0], r, max_t,
                               out.ctypes.data_as(ctypes.POINTER(_Rec)), go.ctypes.data_as(_U32P) if trace else None,
                               to.ctypes.data_as(_U32P) if trace else None, ctypes.byref(T),
                               ctypes.byref(stalled) if with_stalled else None)
    return rc, out, go, to, T.value, stalled.value


def _first_diff(got, ref):
    if got.shape != ref.shape:
        return f"shapes {got.shape} vs {ref.shape}"
    agents, cols = np.nonzero(got != ref)
    k = int(np.lexsort((agents, cols))[0])
    t, i = int(cols[k]), int(agents[k])
    return f"column {t} agent {i}: gpu {int(got[i, t]):#x} model {int(ref[i, t]):#x}"


def _assert_run(got, ref):
    rec, goals, tasks, stalled = got
    assert rec.dtype == np.uint64 and goals.dtype == tasks.dtype == np.uint32
    assert rec.shape[1] == ref.T, f"T: gpu {rec.shape[1]} model {ref.T}"
    assert np.array_equal(rec, ref.rec), "rec: " + _first_diff(rec, ref.rec)
    assert np.array_equal(goals, ref.goals), "goals: " + _first_diff(goals, ref.goals)
    assert np.array_equal(tasks, ref.tasks), "tasks: " + _first_diff(tasks, ref.tasks)
    assert stalled == ref.stalled


# ---- the run against the model ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(mm.CASES))
def test_run_matches_model(planners, name):
    rows, starts, tasks, r, max_t, ending = mm.instance(name)
    ref = mm.run_case(name)
    assert mm.ending(ref, max_t) == ending  # the case still ends the way its row names
    _assert_run(planners(rows).fleet_mapd(starts, tasks, max_t, r, trace=True), ref)


@pytest.mark.parametrize("name", list(mm.HAND_CASES))
def test_hand_made_endings_match_model(planners, name):
    rows, starts, tasks, r, max_t, _ = mm.instance(name)
    _assert_run(planners(rows).fleet_mapd(starts, tasks, max_t, r, trace=True), mm.run_case(name))


def test_no_tasks_and_max_t_zero_give_one_column(planners):
    for name, state in (("no-tasks", mm.REC_IDLE), ("max_t-0", mm.PICKING)):
        rows, starts, tasks, r, max_t, _ = mm.instance(name)
        rc, out, _, _, T, stalled = _raw(planners(rows), starts, tasks, r, max_t)
        assert (rc, T, stalled) == (TSW_OK, 1, 0), name
        assert np.all((out[:, 0] >> np.uint64(32)) == state), name  # the pad bytes are zero


def test_empty_fleet(planners):
    p = planners(maps.open_map(6, 6))
    _, _, tasks, r, max_t, _ = mm.instance("single")
    rc, _, _, _, T, stalled = _raw(p, np.zeros((0, 2), dtype=np.uint32), tasks, r, max_t)
    assert (rc, T, stalled) == (TSW_OK, 0, 0)
    rec, stalled = p.fleet_mapd(np.zeros((0, 2), dtype=np.uint32), tasks, max_t, r)
    assert rec.shape == (0, 0) and stalled is False


# ---- outputs ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["open8", "rand20"])
def test_null_traces_give_the_same_records(planners, name):
    rows, starts, tasks, r, max_t, _ = mm.instance(name)
    ref = mm.run_case(name)
    rc, out, go, to, T, stalled = _raw(planners(rows), starts, tasks, r, max_t, trace=False, with_stalled=False)
    assert rc == TSW_OK and T == ref.T and stalled == FILL  # a NULL stalled is not written
    assert np.array_equal(out[:, :T], ref.rec), _first_diff(out[:, :T], ref.rec)
    assert np.all(go == FILL) and np.all(to == FILL)
    rec, st = planners(rows).fleet_mapd(starts, tasks, max_t, r)
    assert np.array_equal(rec, ref.rec) and st == ref.stalled


def test_columns_from_out_T_on_stay_untouched(planners):
    rows, starts, tasks, r, max_t, _ = mm.instance("rand20")
    ref = mm.run_case("rand20")
    rc, out, go, to, T, stalled = _raw(planners(rows), starts, tasks, r, max_t)
    assert (rc, T, stalled) == (TSW_OK, ref.T, 1) and T < max_t + 1
    assert np.array_equal(out[:, :T], ref.rec) and np.array_equal(go[:, :T], ref.goals)
    assert np.array_equal(to[:, :T], ref.tasks)
    assert np.all(out[:, T:] == FILL64) and np.all(go[:, T:] == FILL) and np.all(to[:, T:] == FILL)


# ---- errors -------------------------------------------------------------------------------------------

def test_einval_before_anything_runs_and_the_context_stays_usable():
    """The single case's 6 x 6 grid with a blocked seventh row: same cell ids, same run."""
    rows, starts, tasks, r, max_t, _ = mm.instance("single")
    ref = mm.run_case("single")
    walled = list(rows) + ["@" * 6]
    blocked_start = np.array([[2, 6]], dtype=np.uint32)
    # the bad task is the appended one, index 3: one agent and max_t = 0 hand out task 0 only, so it is
    # never dispatched; blocked delivery in one variant, off-grid pickup in the other
    bad_delivery = np.concatenate([tasks, np.array([[1, 1, 3, 6]], dtype=np.uint32)])
    bad_pickup = np.concatenate([tasks, np.array([[6, 0, 1, 1]], dtype=np.uint32)])
    with Planner(walled) as p:
        for label, args in (("blocked start", (blocked_start, tasks, r, max_t)),
                            ("blocked delivery of a task never dispatched", (starts, bad_delivery, r, 0)),
                            ("off-grid pickup of a task never dispatched", (starts, bad_pickup, r, 0)),
                            ("max_t too large", (starts, tasks, r, (1 << 20) + 1))):
            rc, out, go, to, T, stalled = _raw(p, *args)
            assert rc == TSW_EINVAL, label
            assert T == 0 and np.all(out == FILL64) and np.all(go == FILL) and np.all(to == FILL), label
            _assert_run(p.fleet_mapd(starts, tasks, max_t, r, trace=True), ref)
        n = starts.shape[0]
        sp = starts.ctypes.data_as(ctypes.POINTER(_Point))
        tp = tasks.ctypes.data_as(ctypes.POINTER(_Task))
        out = np.zeros((n, max_t + 1), dtype=np.uint64)
        T = ctypes.c_uint32(0)
        assert p._lib.tsw_fleet_mapd(p._ctx, sp, n, tp, 3, r, max_t, out.ctypes.data_as(ctypes.POINTER(_Rec)), None,
                                     None, None, None) == TSW_EINVAL  # NULL out_T
        assert p._lib.tsw_fleet_mapd(p._ctx, sp, n, tp, 3, r, max_t, None, None, None, ctypes.byref(T),
                                     None) == TSW_EINVAL  # NULL out with n > 0
        with pytest.raises(TswapError):
            p.fleet_mapd(blocked_start, tasks, max_t, r)
        _assert_run(p.fleet_mapd(starts, tasks, max_t, r, trace=True), ref)


# ---- composition with the existing entry points -------------------------------------------------------

def test_run_equals_fleet_run_ticks_plus_the_task_phase(planners):
    """What a caller had to do before: per step the task phase on the host and fleet_run(ticks=1)."""
    rows, starts, tasks, r, max_t, _ = mm.instance("open8")
    p = planners(rows)
    W = len(rows[0])
    pick, dlv = mm.cells_of(tasks[:, :2], W), mm.cells_of(tasks[:, 2:], W)
    v = mm.cells_of(starts, W)
    g = v.copy()
    st, tk = np.zeros(v.size, dtype=np.uint32), np.full(v.size, mm.NONE, dtype=np.uint32)
    nxt, cols, gcols, tcols, stalled = 0, [], [], [], False
    while True:
        nxt, tchanged = mm.task_phase_scan(v, g, st, tk, nxt, pick, dlv)
        v, g, ticked = p.fleet_run(v, g, 1, r)
        done = nxt == pick.size and bool(np.all(st == mm.IDLE))
        if not done and not tchanged and not ticked:
            stalled = True
            break
        cols.append(mm.pack(v, g, st, W))
        gcols.append(g.copy())
        tcols.append(tk.copy())
        if done or len(cols) > max_t:
            break
    rec, goals, tks, got_stalled = p.fleet_mapd(starts, tasks, max_t, r, trace=True)
    assert np.array_equal(rec, np.stack(cols, axis=1)), _first_diff(rec, np.stack(cols, axis=1))
    assert np.array_equal(goals, np.stack(gcols, axis=1)) and np.array_equal(tks, np.stack(tcols, axis=1))
    assert got_stalled == stalled


def test_fleet_run_is_the_same_before_and_after_a_mapd_run(planners):
    """tsw_fleet_run and tsw_fleet_mapd share the context's fleet buffers (lists, apply state, records)."""
    name, r, ticks = fm.RUN_CASES[0]
    rows, v, g = fc.fleet_case(name)
    mrows, starts, tasks, mr, max_t, _ = mm.instance("dense12")
    assert mrows == rows  # the same map: one context
    p = planners(rows)
    before = p.fleet_run(v, g, ticks, r, record=True)
    _assert_run(p.fleet_mapd(starts, tasks, max_t, mr, trace=True), mm.run_case("dense12"))
    after = p.fleet_run(v, g, ticks, r, record=True)
    ref = fm.run_case(name)
    assert before[2] == after[2] == ref[4]
    for a, b, c in zip(before, after, (ref[0], ref[1], None, ref[2], ref[3])):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    _assert_run(p.fleet_mapd(starts, tasks, max_t, mr, trace=True), mm.run_case("dense12"))
