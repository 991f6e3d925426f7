"""GPU: one context, many calls — the table store as a per-tick manager uses it.

* Different entry points one after another on ONE context under a table budget (plan, step ticks, decide_fleet,
  fleet_run, next_hop_codes, another plan, the first plan again): every result equals the oracle or the CPU
  model, the store passes the audit (table_io_cases.check_store) after every call, tables are evicted and
  rebuilt on the way.
* tsw_clear_tables on a fresh and on a warm context: the tables are really dropped and rebuilt.
* A table-less (u16-overflow) goal's slot evicted and reused for a real table, and the reverse: the
  per-slot table-less flag follows the slot's current goal.
* tsw_plan_mapd_resolved whose resolver fails (raises, answers a code > 4, answers the wrong length): the call
  fails, no next hop stays queued for a K3 pass that did not run, and the same context plans exactly afterwards;
  the entry points refuse re-entry from inside the resolver.
* A plan that fails on a bad task cell half-way leaves a store that passes the audit and a context that plans.
"""
import functools

import numpy as np
import pytest

import fleet_cases as fc
import fleet_run_model as fm
from p2p_distributed_tswap_amd import (TSW_EINVAL, TSW_EOVERFLOW, TSW_F_EAGER_NEXTHOP, TSW_F_EXIT_MODE,
                                       TSW_F_LAZY_NEXTHOP, Planner, TswapError, maps)
from table_io_cases import check_store, goalset
from test_gpu_fleet import _assert_fleet_equal
from test_gpu_store import _serpentine_plus_room
from worker_cases import MapRef

pytestmark = pytest.mark.gpu

FLAGS = {"default": 0, "exit": TSW_F_EXIT_MODE, "lazy": TSW_F_LAZY_NEXTHOP}
MIXED_FLAGS = {**FLAGS, "eager": TSW_F_EAGER_NEXTHOP}
RADIUS, RUN_TICKS, MAX_T = 15, 10, 60


@functools.lru_cache(maxsize=None)
def _rand32() -> MapRef:
    return MapRef(maps.random_map(32, 32, 0.2, 0x3232))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _plan(seed):
    """(starts, tasks, oracle records, oracle goals, goal set) of make_instance(rand32, 40, 80, seed), MAX_T steps."""
    ref = _rand32()
    starts, tasks = maps.make_instance(ref.rows, 40, 80, seed)
    rec, goal = ref.og.mapd(starts, tasks, MAX_T, trace_goals=True)
    return _ro(starts, tasks, rec, goal, goalset(ref.rows, starts, tasks))


def _comp(ref):
    return np.array([y * ref.W + x for x, y in maps.largest_component(ref.rows)], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _ticks():
    """5 step ticks of 20 agents with fresh seeded goals every tick: [(v, g, v', g')] by the oracle."""
    ref = _rand32()
    cid = _comp(ref)
    rng = np.random.default_rng(0x57E9)
    v = cid[rng.choice(cid.size, 20, replace=False)]
    out = []
    for _ in range(5):
        g = cid[rng.choice(cid.size, 20, replace=True)]
        rv, rg = ref.og.step(v, g)
        out.append(_ro(v, g, rv, rg))
        v = rv.copy()
    return out


@functools.lru_cache(maxsize=None)
def _fleet():
    """(v, g, oracle decisions of one tick, model run of RUN_TICKS ticks) of a fleet_cases recipe fleet."""
    ref = _rand32()
    v, g, rings = fc.recipe_fleet(ref.rows, 60, 3, 4)
    assert rings > 0
    off, idx = fc.brute_nearby(v, ref.W, RADIUS)
    dec = fc.oracle_fleet(ref.og, v, g, off, idx)
    run = fm.run_model(ref.og, ref.rows, v, g, RADIUS, RUN_TICKS)
    return v, g, dec, run


@functools.lru_cache(maxsize=None)
def _pairs():
    """300 seeded (start, goal) pairs toward 120 distinct goals and get_path's codes for them."""
    ref = _rand32()
    cid = _comp(ref)
    rng = np.random.default_rng(0x9A185)
    st = cid[rng.choice(cid.size, 300)]
    gl = rng.choice(cid[rng.choice(cid.size, 120, replace=False)], 300)
    st[:4] = gl[:4]  # start == goal: code 4
    want = ref.astar_codes([(int(a), int(b)) for a, b in zip(st, gl)])
    return _ro(st, gl, want)


def _assert_plan(p, seed, what, again=None):
    starts, tasks, rrec, rgoal, _ = _plan(seed)
    rec, goal = p.plan_mapd_arrays(starts, tasks, MAX_T, trace_goals=True)
    assert np.array_equal(goal, rgoal), f"{what}: goals differ from the oracle's"
    assert np.array_equal(rec, rrec), f"{what}: records differ from the oracle's"
    if again is not None:
        assert np.array_equal(rec, again[0]) and np.array_equal(goal, again[1]), f"{what}: differs from the first run"
    return rec, goal


def _per_table(ncell):
    return (ncell + 7) // 8 * 8 * 2  # detour byte + next-hop code per cell


# ---- mixed sequence under a budget -----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MIXED_FLAGS))
def test_mixed_entry_points_on_one_budgeted_context(mode):
    ref = _rand32()
    fv, fg, fdec, frun = _fleet()
    st, gl, want = _pairs()
    counts = ([_plan(1)[4].size] + [np.unique(t[1]).size for t in _ticks()] + [np.unique(fg).size] * 2 +
              [np.unique(gl).size, _plan(2)[4].size, _plan(1)[4].size])
    budget = max(counts)
    assert sum(counts) >= 2 * budget  # the sequence cannot fit: tables are evicted, yet no single call can hit ENOMEM
    with Planner(ref.rows, flags=MIXED_FLAGS[mode], table_budget_bytes=budget * _per_table(ref.W * ref.H)) as p:
        first = _assert_plan(p, 1, "plan A")
        check_store(p, ref, _plan(1)[4], "after plan A")
        for k, (v, g, rv, rg) in enumerate(_ticks()):
            hv, hg = p.step(v, g)
            assert np.array_equal(hv, rv) and np.array_equal(hg, rg), f"step tick {k}"
            check_store(p, ref, g, f"after step tick {k}")
        _assert_fleet_equal(p.decide_fleet(fv, fg, RADIUS), fdec)
        check_store(p, ref, fg, "after decide_fleet")
        rv, rg, rvr, rgr, rdone, _ = frun
        hv, hg, done, vr, gr = p.fleet_run(fv, fg, RUN_TICKS, RADIUS, record=True)
        assert done == rdone and np.array_equal(vr, rvr) and np.array_equal(gr, rgr)
        assert np.array_equal(hv, rv) and np.array_equal(hg, rg)
        check_store(p, ref, fg, "after fleet_run")
        assert np.array_equal(p.next_hop_codes(st, gl), want)
        check_store(p, ref, gl, "after next_hop_codes")
        _assert_plan(p, 2, "plan B")
        check_store(p, ref, _plan(2)[4], "after plan B")
        _assert_plan(p, 1, "plan A again", again=first)
        check_store(p, ref, _plan(1)[4], "after plan A again")
        stats = p.stats()
    assert stats["table_evictions"] > 0 and stats["tables"] <= budget


# ---- clear_tables ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(FLAGS))
def test_clear_tables_drops_and_rebuilds(mode):
    ref = _rand32()
    st, gl, want = _pairs()
    goals = _plan(1)[4]
    with Planner(ref.rows, flags=FLAGS[mode]) as p:
        p.clear_tables()  # nothing to clear: TSW_OK
        assert p.stats()["tables"] == 0
        _assert_plan(p, 1, "warm-up plan")
        v, g, rv, rg = _ticks()[0]
        hv, hg = p.step(v, g)
        assert np.array_equal(hv, rv) and np.array_equal(hg, rg)
        assert np.array_equal(p.next_hop_codes(st, gl), want)
        assert p.stats()["tables"] >= goals.size
        p.clear_tables()
        assert p.stats()["tables"] == 0
        p.clear_tables()
        assert p.stats()["tables"] == 0
        p.reset_stats()
        _assert_plan(p, 1, "plan after clear")
        stats = p.stats()
        assert stats["bfs_goals"] == goals.size and stats["tables"] == goals.size  # every table was built again
        check_store(p, ref, goals, "after clear and plan")
        hv, hg = p.step(v, g)
        assert np.array_equal(hv, rv) and np.array_equal(hg, rg)


# ---- table-less slot reuse ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _big() -> MapRef:
    return MapRef(_serpentine_plus_room())


@functools.lru_cache(maxsize=None)
def _big_steps():
    """Steps on the 512x512 serpentine + room, by the oracle: `far` an agent deep in the serpentine heading for its
    entry (cell 0: no u16 table) beside two room agents, `room[k]` four room agents with four fresh room goals."""
    ref, W = _big(), 512
    rng = np.random.default_rng(0x512)
    cells = (rng.choice(np.arange(445, 510), 40)[:, None] * W + rng.choice(np.arange(2, 510), (40, 1))).reshape(-1)
    cells = np.unique(cells.astype(np.uint32))[:32]
    rng.shuffle(cells)
    assert cells.size == 32
    v = np.array([200 * W + 100, cells[0], cells[1]], dtype=np.uint32)
    g = np.array([0, cells[2], cells[3]], dtype=np.uint32)
    far = _ro(v, g, *ref.og.step(v, g))
    room = []
    for k in range(3):
        v, g = cells[4 + 8 * k:8 + 8 * k].copy(), cells[8 + 8 * k:12 + 8 * k].copy()
        room.append(_ro(v, g, *ref.og.step(v, g)))
    return far, room


def _assert_step(p, case, what):
    v, g, rv, rg = case
    hv, hg = p.step(v, g)
    assert np.array_equal(hv, rv) and np.array_equal(hg, rg), what


def _assert_real_tables(p, ref, goals, what):
    got = p.dist_tables(goals[:1])
    assert np.array_equal(got[0], ref.og.bfs(int(goals[0]))), what
    check_store(p, ref, goals, what)


@pytest.mark.parametrize("order", ["tableless-first", "real-first"])
@pytest.mark.parametrize("mode", list(FLAGS))
def test_tableless_slot_reuse(mode, order):
    ref = _big()
    far, room = _big_steps()
    zero = np.array([0], dtype=np.uint32)
    with Planner(ref.rows, flags=FLAGS[mode], table_budget_bytes=4 * _per_table(512 * 512)) as p:
        if order == "tableless-first":
            _assert_step(p, far, "step toward cell 0")
            assert p.stats()["tableless_goals"] >= 1
            _assert_step(p, room[0], "room step 1")  # 4 fresh goals into 4 slots: cell 0's slot is evicted ...
            _assert_step(p, room[1], "room step 2")  # ... and all four are reused for real tables
            assert p.stats()["table_evictions"] >= 5
            _assert_real_tables(p, ref, room[1][1], "room goals in reused slots")
            _assert_step(p, far, "step toward cell 0 again")
        else:
            _assert_step(p, room[0], "room step 1")
            _assert_real_tables(p, ref, room[0][1], "room goals")
            _assert_step(p, far, "step toward cell 0")  # cell 0 takes a slot that held a real table
            assert p.stats()["tableless_goals"] >= 1 and p.stats()["table_evictions"] >= 3
            _assert_step(p, room[2], "room step 2")     # and gives it back to a real table
            _assert_real_tables(p, ref, room[2][1], "room goals in reused slots")
            _assert_step(p, far, "step toward cell 0 again")
        assert p.stats()["tables"] <= 4
        with pytest.raises(TswapError) as ei:
            p.dist_tables(zero)
        assert ei.value.code == TSW_EOVERFLOW


# ---- resolver failures -------------------------------------------------------------------------------------------

def _resolver(owner, fail=None, inside=None):
    """A resolver answering from `owner`; its second call fails in the way `fail` names, or runs `inside` first."""
    calls = []

    def resolve(st, gl):
        calls.append(st.size)
        if len(calls) == 2:
            if fail == "raise":
                raise RuntimeError("resolver down")
            if inside is not None:
                inside()
        codes = owner.next_hop_codes(st, gl)
        if len(calls) == 2 and fail == "code5":
            codes[codes.size // 2] = 5
        if len(calls) == 2 and fail == "short":
            codes = codes[:-1]
        return codes

    return resolve, calls


@pytest.fixture(scope="module")
def owner():
    """The answering context of the resolver tests (its own store, as a goal owner's rank)."""
    with Planner(_rand32().rows) as o:
        yield o


def test_resolver_is_called_several_times(owner):
    """The premise of the failure cases: the instance stops for next hops at least 3 times."""
    starts, tasks, rrec, rgoal, _ = _plan(1)
    resolve, calls = _resolver(owner)
    with Planner(_rand32().rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        rec, goal = p.plan_mapd_resolved(starts, tasks, MAX_T, resolve, trace_goals=True)
        assert p.stats()["astar_launches"] == 0
    assert len(calls) >= 3 and min(calls) > 0, calls
    assert np.array_equal(goal, rgoal) and np.array_equal(rec, rrec)


@pytest.mark.parametrize("fail", ["raise", "code5", "short"])
def test_resolver_failure_leaves_a_clean_store(owner, fail):
    ref = _rand32()
    starts, tasks, _, _, goals = _plan(1)
    resolve, calls = _resolver(owner, fail)
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        if fail == "raise":
            with pytest.raises(RuntimeError, match="resolver down"):
                p.plan_mapd_resolved(starts, tasks, MAX_T, resolve)
        elif fail == "code5":
            with pytest.raises(TswapError) as ei:
                p.plan_mapd_resolved(starts, tasks, MAX_T, resolve)
            assert ei.value.code == TSW_EINVAL
        else:
            with pytest.raises(ValueError, match="resolver returned"):
                p.plan_mapd_resolved(starts, tasks, MAX_T, resolve)
        assert len(calls) == 2
        # nothing queued for the K3 pass that did not run stays pending, nothing wrong got in
        check_store(p, ref, goals, f"after the failed plan ({fail})")
        _assert_plan(p, 1, f"plan after the failed one ({fail})")
        check_store(p, ref, goals, f"after the second plan ({fail})")


def test_entry_points_refuse_reentry_from_the_resolver(owner):
    ref = _rand32()
    starts, tasks, rrec, rgoal, goals = _plan(1)
    refused = []
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        v, g = _ticks()[0][:2]

        def inside():
            for name, call in (("next_hop_codes", lambda: p.next_hop_codes(v, g)), ("step", lambda: p.step(v, g)),
                               ("dist_tables", lambda: p.dist_tables(g[:2])), ("clear_tables", p.clear_tables)):
                with pytest.raises(TswapError) as ei:
                    call()
                assert ei.value.code == TSW_EINVAL, name
                refused.append(name)

        resolve, calls = _resolver(owner, inside=inside)
        rec, goal = p.plan_mapd_resolved(starts, tasks, MAX_T, resolve, trace_goals=True)
        assert refused == ["next_hop_codes", "step", "dist_tables", "clear_tables"] and len(calls) >= 3
        assert np.array_equal(goal, rgoal) and np.array_equal(rec, rrec)
        check_store(p, ref, goals, "after the plan")


# ---- a bad task cell half-way ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _task_ref(rows) -> MapRef:
    return MapRef(list(rows))


@pytest.mark.parametrize("case", [1, 2])
@pytest.mark.parametrize("mode", list(FLAGS))
def test_bad_task_cell_mid_plan_leaves_a_clean_store(mode, case):
    """test_gpu_parity.test_mapd_task_cells_checked_when_used, continued on the same context: after the TSW_EINVAL
    the store passes the audit over every valid cell of the failed instance, and a well-formed instance plans."""
    from test_oracle import _lazy_task_cases

    rows, starts, bad_tasks, max_t, fails = _lazy_task_cases()[case]
    assert fails
    ref = _task_ref(tuple(rows))
    _, tasks = maps.make_instance(rows, 4, 12, 5)
    W, H = ref.W, ref.H
    ok = [(x, y) for x, y in np.concatenate([starts, bad_tasks[:, :2], bad_tasks[:, 2:]]).tolist()
          if x < W and y < H and ref.free[y * W + x]]
    goals = np.unique(np.array([y * W + x for x, y in ok], dtype=np.uint32))
    rrec, rgoal = ref.og.mapd(starts, tasks, 200, trace_goals=True)
    with Planner(rows, flags=FLAGS[mode]) as p:
        with pytest.raises(TswapError) as ei:
            p.plan_mapd_arrays(starts, bad_tasks, max_t)
        assert ei.value.code == TSW_EINVAL
        check_store(p, ref, goals, "after the failed plan")
        rec, goal = p.plan_mapd_arrays(starts, tasks, 200, trace_goals=True)
        assert np.array_equal(goal, rgoal) and np.array_equal(rec, rrec)
        check_store(p, ref, goalset(rows, starts, tasks), "after the well-formed plan")

