"""GPU: tsw_task_timeline / tsw_task_timeline_device. The library's task table and every summary field must equal
the CPU model's (tests/timeline_model.py) exactly: forward's own task log for the records of real plans, replay
and truncated for tampered records. Every case asserts from the model's counters that it exercises what it is
there for. Grids are 12x12 to 32x32 and max_t <= 128."""
import ctypes

import numpy as np
import pytest

import fleet_mapd_model as mm
import timeline_model as tm
import p2p_distributed_tswap_amd as pkg
from p2p_distributed_tswap_amd import (TSW_EINVAL, TSW_F_LAZY_NEXTHOP, TSW_OK, Planner, Timeline, TswapError, _Point, _Rec,
                                       _Task, maps)

pytestmark = pytest.mark.gpu

_U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xDEADBEEF
NONE = tm.NONE


@pytest.fixture(scope="module")
def planners():
    """One context per map for the whole module."""
    made = {}

    def get(rows):
        key = tuple(rows)
        if key not in made:
            made[key] = Planner(list(rows))
        return made[key]

    yield get
    for p in made.values():
        p.close()


def _plan(p, name):
    """The library's own records of a named case: they equal the model's."""
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case(name)
    got = p.plan_mapd_arrays(starts, tasks, max_t)[0] if rel is None else p.plan_mapd_online(starts, tasks, rel, max_t)[0]
    assert got.shape == rec.shape and np.array_equal(got, rec), name
    return got


def _check_case(planners, name):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case(name)
    p = planners(rows)
    got = p.task_timeline(_plan(p, name), starts, tasks, rel)
    tm.assert_equal(got, tm.expected(name), name)
    assert got["consistent"] == 1 and got["bad_kind"] == got["bad_t"] == got["bad_agent"] == NONE
    return got, cnt


def _raw(p, rec, n, T, stride, starts, tasks, rel, m, rule, fn="tsw_task_timeline", with_sum=True, rec_ptr=...):
    """The C entry point on sentinel-filled outputs: (rc, sum bytes, task words)."""
    sm = Timeline()
    ctypes.memset(ctypes.byref(sm), 0xAB, ctypes.sizeof(sm))
    tw = np.full((max(m, 1), 4), FILL, dtype=np.uint32)
    if rec_ptr is ...:
        rec_ptr = rec.ctypes.data_as(ctypes.POINTER(_Rec)) if rec is not None else None
    rc = getattr(p._lib, fn)(
        p._ctx, rec_ptr, n, T, stride, starts.ctypes.data_as(ctypes.POINTER(_Point)) if starts is not None else None,
        tasks.ctypes.data_as(ctypes.POINTER(_Task)) if tasks is not None else None,
        rel.ctypes.data_as(_U32P) if rel is not None else None, m, rule, ctypes.byref(sm) if with_sum else None,
        tw.ctypes.data_as(_U32P))
    return rc, bytes(sm), tw


# ---- 1. a plain plan -----------------------------------------------------------------------------------------

def test_plain_plan(planners):
    got, cnt = _check_case(planners, "plain")
    assert got["assigned"] == 20 and got["delivered"] >= 10 and got["unreleased"] == 0
    done = got["task"][:, 3] != NONE
    assert got["wait_sum"] == int(got["task"][:, 1].sum()) and got["makespan"] == int(got["task"][done, 3].max())


def test_fewer_tasks_than_agents(planners):
    got, cnt = _check_case(planners, "fewer-tasks")
    assert got["assigned"] == 6 and len(set(got["task"][:, 0].tolist())) == 6  # four agents never take a task


def test_summary_alone(planners):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("plain")
    p = planners(rows)
    sm = Timeline()
    assert p._lib.tsw_task_timeline(p._ctx, rec.ctypes.data_as(ctypes.POINTER(_Rec)), *rec.shape, rec.shape[1],
                                    starts.ctypes.data_as(ctypes.POINTER(_Point)), tasks.ctypes.data_as(ctypes.POINTER(_Task)),
                                    None, len(tasks), 0, ctypes.byref(sm), None) == TSW_OK
    ref = tm.expected("plain")
    assert sm.as_dict() == {k: ref[k] for k in tm.SUMMARY}


# ---- 2. online plans -----------------------------------------------------------------------------------------

def test_one_task_released_per_step(planners):
    got, cnt = _check_case(planners, "paced")
    assert got["assigned"] >= 60 and got["wait_sum"] > 0
    assert (got["task"][:64, 1] >= np.arange(1, 65)).all()  # nobody is assigned a task before its release


def test_random_releases_and_a_column_prefix(planners):
    got, cnt = _check_case(planners, "random-release")
    rows, starts, tasks, rel, max_t, rec, log, _ = tm.case("random-release")
    late = np.flatnonzero(rel > max_t)
    assert got["unreleased"] == 2 == late.size and (got["task"][late] == NONE).all()
    # any prefix of the columns is a valid input: tasks still open at T = 40 keep their 0xFFFFFFFF times
    T = 40
    cut = planners(rows).task_timeline(rec[:, :T], starts, tasks, rel)
    tm.assert_equal(cut, tm.replay(rec[:, :T], starts, tasks, rel), "prefix")
    full = log.astype(np.int64)
    assert np.array_equal(cut["task"][:, 1:], np.where(full[:, 1:] < T, full[:, 1:], NONE).astype(np.uint32))
    assert cut["consistent"] == 1 and cut["assigned"] > cut["carried"] >= cut["delivered"] >= 1
    assert cut["unreleased"] == np.count_nonzero(rel > T - 1) > 2


# ---- 3. ties, 4. hand-overs and several takes in one column -----------------------------------------------------

def test_distance_ties_go_to_the_lowest_index(planners):
    got, cnt = _check_case(planners, "ties")
    assert cnt["ties"] > 0
    # tasks k, k + 6, k + 12 share a pickup point: they are assigned in index order
    ta = got["task"][:, 1].astype(np.int64)
    assert (ta[:6] <= ta[6:12]).all() and (ta[6:12] <= ta[12:]).all()


def test_hand_overs_and_several_takes_in_one_column(planners):
    got, cnt = _check_case(planners, "busy")
    assert cnt["handovers"] > 0 and cnt["multi_take"] > 0 and got["assigned"] > 8


# ---- 5. the scan's edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c for c in tm.CASES if c.startswith("scan-")])
def test_scan_edges(planners, name):
    """m on either side of a wave, of the workgroup's 1,024 lanes and of two strides of them, and 20,000: more
    candidates than the kernel keeps in LDS (18,432 at most), so the array continues in global memory, the last
    entry moves from there into LDS places and the staggered release appends across the boundary. Only a few
    tasks are ever taken. Staggered: 30 tasks at 0 and the rest at 30, so takes happen while most of the released tasks are
    gone (what would be a compaction in a release-ordered scan is here the removal of entries near the end of
    the array, and appends behind removals)."""
    got, cnt = _check_case(planners, name)
    m = int(name.split("-")[1])
    assert got["assigned"] >= min(m, 20)
    if name.endswith("staggered"):
        assert cnt["half_dead"] > 0 and got["assigned"] > 20
    p = planners(tm.ROWS32)
    probe = p.timeline_probe()
    assert probe["takes"] == got["assigned"] and probe["candidates_scanned"] >= got["assigned"]


# ---- 6. the smallest shapes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (0, 0)])
def test_nothing_to_replay(planners, shape):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("random-release")
    p = planners(rows)
    n, T = shape
    got = p.task_timeline(np.zeros(shape, dtype=np.uint64), starts[:n], tasks, rel)
    tm.assert_equal(got, tm.replay(np.zeros(shape, dtype=np.uint64), starts[:n], tasks, rel), str(shape))
    assert got["consistent"] == 1 and got["assigned"] == 0 and (got["task"] == NONE).all()
    assert got["unreleased"] == (len(tasks) if T == 0 else np.count_nonzero(rel > T - 1))
    assert got["service_min"] == got["makespan"] == NONE and got["service_max"] == 0
    # NULL rec and starts are fine when there is nothing to read
    rc, sm, tw = _raw(p, None, n, T, T, None, np.ascontiguousarray(tasks), np.ascontiguousarray(rel), len(tasks), 0)
    assert rc == TSW_OK and (tw == NONE).all()
    assert Timeline.from_buffer_copy(sm).as_dict() == {k: got[k] for k in tm.SUMMARY}


def test_no_tasks_and_one_column(planners):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("plain")
    p = planners(rows)
    idle = p.plan_mapd_arrays(starts, tasks[:0], max_t)[0]  # m = 0: one column, everybody idle
    assert idle.shape == (10, 1)
    got = p.task_timeline(idle, starts, tasks[:0])
    tm.assert_equal(got, tm.replay(idle, starts, tasks[:0]), "m = 0")
    assert got["consistent"] == 1 and got["task"].shape == (0, 4) and got["assigned"] == 0
    one = p.task_timeline(rec[:, :1], starts, tasks)  # T = 1: the ten takes of column 0
    tm.assert_equal(one, tm.replay(rec[:, :1], starts, tasks), "T = 1")
    assert one["assigned"] == 10 and one["carried"] == 0 and one["consistent"] == 1
    # the same column against no tasks: the first agent is PICKING with nothing to take
    bad = p.task_timeline(rec[:, :1], starts, tasks[:0])
    assert (bad["consistent"], bad["bad_kind"], bad["bad_t"], bad["bad_agent"]) == (0, 1, 0, 0)


# ---- 7. the device entry point -------------------------------------------------------------------------------

def test_device_form_reads_in_place(planners):
    """The device memory comes from the HIP runtime the library links (GuardedDevBuf), as in test_gpu_audit: a torch
    tensor's runtime cannot open the device in a process where the library's already has. The entry point sees an
    address either way."""
    from table_io_cases import GuardedDevBuf

    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("random-release")
    p = planners(rows)
    ref = p.task_timeline(rec, starts, tasks, rel)
    tm.assert_equal(ref, tm.expected("random-release"))
    n, T = rec.shape
    wide = np.full((n, T + 5), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # sentinel columns past T, pad bytes all ones
    wide[:, :T] = rec | np.uint64(0xFFFFFF << 40)
    for host, stride, shift in ((np.ascontiguousarray(rec), T, 0), (wide, T + 5, 8)):
        dev = GuardedDevBuf(host.nbytes, shift)
        dev.from_host(host)
        there = p.task_timeline_device(dev.addr, n, T, stride, starts, tasks, rel)
        tm.assert_equal(there, ref, f"stride {stride}")
        dev.guards_intact(f"stride {stride}")
        assert np.array_equal(dev.read(np.uint64, host.shape), host)  # read, never written
    # the host form with stride > T
    rc, sm, tw = _raw(p, wide, n, T, T + 5, np.ascontiguousarray(starts), np.ascontiguousarray(tasks),
                      np.ascontiguousarray(rel), len(tasks), 0)
    assert rc == TSW_OK and np.array_equal(tw, ref["task"])
    assert Timeline.from_buffer_copy(sm).as_dict() == {k: ref[k] for k in tm.SUMMARY}


# ---- 8. rule STREAM on fleet_mapd's records --------------------------------------------------------------------

@pytest.mark.parametrize("name", ["open8", "pickup-is-delivery", "fewer-tasks"])
def test_stream_rule_on_fleet_records(planners, name):
    rows, starts, tasks, r, max_t, _ = mm.instance(name)
    run = mm.run_case(name)
    assert run.delivered >= 1
    p = planners(rows)
    rec, goals, tks, stalled = p.fleet_mapd(starts, tasks, max_t, r, trace=True)
    assert np.array_equal(rec, run.rec) and np.array_equal(tks, run.tasks)
    got = p.task_timeline(rec, None, tasks, rule="stream")
    tm.assert_equal(got, tm.replay(rec, None, tasks, None, "stream"), name)
    assert got["consistent"] == 1 and got["assigned"] == run.next and got["delivered"] == run.delivered
    for k in range(run.next):  # agent and t_assign: the first appearance of task k in task_out
        i, t = np.argwhere(tks == k)[np.argmin(np.argwhere(tks == k)[:, 1])]
        assert (got["task"][k, 0], got["task"][k, 1]) == (i, t), k


# ---- 9. tampered records ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain", "random-release", "fewer-tasks", "scan-1025-staggered"])
def test_tampered_records(planners, name):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case(name)
    p = planners(rows)
    T = rec.shape[1]
    tampers = [tm.tamper_picking_to_idle(rec), tm.tamper_take_to_stay(rec, log)]
    if name != "fewer-tasks":
        tampers.append(tm.tamper_take_to_stay(rec, log, 5))
    if name not in ("plain", "scan-1025-staggered"):
        tampers.append(tm.tamper_idle_to_picking(rec, log, rel))
    kinds = set()
    for bad, kind, t, i in tampers:
        got = p.task_timeline(bad, starts, tasks, rel)
        assert (got["consistent"], got["bad_kind"], got["bad_t"], got["bad_agent"]) == (0, kind, t, i)
        # the events before the bound are forward's, nothing at or after it is recorded
        tm.assert_equal(got, tm.truncated(log, rel, T, kind, t, i), f"{name} kind {kind}")
        kinds.add(kind)
    assert kinds >= ({0, 2} if name in ("plain", "scan-1025-staggered") else {0, 1, 2})


def test_bad_state_and_the_earliest_inconsistency_wins(planners):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("plain")
    p = planners(rows)
    T = rec.shape[1]
    bad = tm._with_state(rec, 4, 9, 7)
    tm.assert_equal(p.task_timeline(bad, starts, tasks), tm.truncated(log, rel, T, 0, 9, 4), "state 7")
    # a kind 2 before it in (t, agent) order is the one reported, a kind 0 before that one again
    both, kind, t, i = tm.tamper_take_to_stay(bad, log)
    assert (t, i) < (9, 4)
    tm.assert_equal(p.task_timeline(both, starts, tasks), tm.truncated(log, rel, T, 2, t, i), "kind 2 first")
    late, _, t2, i2 = tm.tamper_take_to_stay(bad, log, 12)
    assert (t2, i2) > (9, 4)
    tm.assert_equal(p.task_timeline(late, starts, tasks), tm.truncated(log, rel, T, 0, 9, 4), "kind 0 first")


def test_fleet_records_contradict_the_nearest_rule(planners):
    rows, starts, tasks, r, max_t, _ = mm.instance("open8")
    rec = mm.run_case("open8").rec
    p = planners(rows)
    # Every task at 0: both rules hand out a task whenever one is left, so the records pass, but the nearest rule
    # names other tasks than the stream did
    ref = tm.replay(rec, starts, tasks)
    assert ref["consistent"] == 1 and not np.array_equal(ref["task"], tm.replay(rec, None, tasks, None, "stream")["task"])
    tm.assert_equal(p.task_timeline(rec, starts, tasks), ref, "fleet records under NEAREST")
    # With release times the fleet never knew of, the fifth agent takes a task in column 0 that is not there yet
    rel = np.array([0] * 4 + [10] * (len(tasks) - 4), dtype=np.uint32)
    ref = tm.replay(rec, starts, tasks, rel)
    assert (ref["consistent"], ref["bad_kind"], ref["bad_t"], ref["bad_agent"]) == (0, 1, 0, 4) and ref["assigned"] == 4
    tm.assert_equal(p.task_timeline(rec, starts, tasks, rel), ref, "fleet records under NEAREST with releases")


# ---- 10. errors ------------------------------------------------------------------------------------------------

def test_einval_leaves_the_outputs_untouched(planners):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("random-release")
    p = planners(rows)
    rec, starts, tasks, rel = (np.ascontiguousarray(a) for a in (rec, starts, tasks, rel))
    n, T = rec.shape
    m = len(tasks)
    untouched = b"\xab" * ctypes.sizeof(Timeline)
    big = (1 << 20) + 2
    cases = (("NULL rec", (None, n, T, T, starts, tasks, rel, m, 0)),
             ("NULL tasks", (rec, n, T, T, starts, None, rel, m, 0)),
             ("NULL starts", (rec, n, T, T, None, tasks, rel, m, 0)),
             ("stride < T", (rec, n, T, T - 1, starts, tasks, rel, m, 0)),
             ("T past the limit", (rec, n, big, big, starts, tasks, rel, m, 0)),
             ("rule 2", (rec, n, T, T, starts, tasks, None, m, 2)),
             ("release with STREAM", (rec, n, T, T, starts, tasks, rel, m, 1)))
    for fn in ("tsw_task_timeline", "tsw_task_timeline_device"):
        for label, args in cases:
            rc, sm, tw = _raw(p, *args, fn=fn)
            assert rc == TSW_EINVAL, (fn, label)
            assert sm == untouched and (tw == FILL).all(), (fn, label)
        rc, _, tw = _raw(p, rec, n, T, T, starts, tasks, rel, m, 0, fn=fn, with_sum=False)
        assert rc == TSW_EINVAL and (tw == FILL).all(), fn
    with pytest.raises(TswapError) as ei:
        p.task_timeline(np.zeros(3, dtype=np.uint64), starts, tasks)
    assert ei.value.code == TSW_EINVAL
    tm.assert_equal(p.task_timeline(rec, starts, tasks, rel), tm.expected("random-release"), "after the refusals")


def test_refused_inside_a_resolver():
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("plain")
    refused = []
    with Planner(rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        def resolve(start, goal):
            with pytest.raises(TswapError) as ei:
                p.task_timeline(rec, starts, tasks)
            refused.append(ei.value.code)
            return pkg.host_next_hop_codes(rows, start, goal)

        p.plan_mapd_resolved(starts, tasks, max_t, resolve)
    assert refused and set(refused) == {TSW_EINVAL}


# ---- 11. the context is untouched ------------------------------------------------------------------------------

def test_a_plan_is_the_same_around_a_timeline():
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("plain")
    with Planner(rows) as p:
        first = p.plan_mapd_arrays(starts, tasks, max_t, trace_goals=True)
        before = p.stats()
        tm.assert_equal(p.task_timeline(first[0], starts, tasks), tm.expected("plain"))
        after = p.stats()
        assert after["tables"] == before["tables"] and after == before  # the timeline touches no counter
        second = p.plan_mapd_arrays(starts, tasks, max_t, trace_goals=True)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
