"""GPU: the lock-step decentralized run. tsw_fleet_apply against the sequential definition
(fleet_run_model.apply_model) on hand-made decisions and on tsw_decide_fleet's own, tsw_fleet_run against
the CPU model run (brute-force lists + the oracle's decisions + apply_model) tick by tick, the fixed-point
stop, the record layout and the documented error codes."""
import ctypes

import numpy as np
import pytest

from p2p_distributed_tswap_amd import (Planner, TswapError, maps, TSW_EINVAL, TSW_EOVERFLOW, TSW_OK)

import fleet_cases as fc
import fleet_run_model as fm

pytestmark = pytest.mark.gpu

_U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xDEADBEEF


def _p(a):
    return a.ctypes.data_as(_U32P)


@pytest.fixture(scope="module")
def planners():
    """One context per map for the whole module (tables stay warm between tests, as between ticks)."""
    made = {}

    def get(rows):
        key = tuple(rows)
        if key not in made:
            made[key] = Planner(rows)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def _raw_apply(p, v, g, act, cell, partner, part_off, part):
    v, g = v.copy(), g.copy()
    rc = p._lib.tsw_fleet_apply(p._ctx, _p(v), _p(g), v.size, _p(act), _p(cell), _p(partner), _p(part_off),
                                _p(part) if part.size else None)
    return rc, v, g


def _raw_run(p, v, g, r, ticks, record=True):
    v, g = v.copy(), g.copy()
    n = v.size
    vr = np.full((n, ticks + 1), FILL, dtype=np.uint32)
    gr = np.full((n, ticks + 1), FILL, dtype=np.uint32)
    done = ctypes.c_uint32(FILL)
    rc = p._lib.tsw_fleet_run(p._ctx, _p(v), _p(g), n, r, ticks, _p(vr) if record else None,
                              _p(gr) if record else None, ctypes.byref(done))
    return rc, v, g, done.value, vr, gr


def _first_diff(got, ref):
    """First differing (tick, agent) of two (n, T) records."""
    if got.shape != ref.shape:
        return f"shapes {got.shape} vs {ref.shape}"
    agents, ticks = np.nonzero(got != ref)
    k = int(np.lexsort((agents, ticks))[0])
    t, i = int(ticks[k]), int(agents[k])
    return f"tick {t} agent {i}: gpu {int(got[i, t])} model {int(ref[i, t])}"


def _assert_state(got_v, got_g, ref_v, ref_g):
    for name, a, b in (("v", got_v, ref_v), ("g", got_g, ref_g)):
        assert a.dtype == np.uint32 and a.shape == b.shape, name
        assert np.array_equal(a, b), f"{name}: first difference at agent {int(np.flatnonzero(a != b)[0])}"


# ---- fleet_apply vs the sequential definition ---------------------------------------------------------

@pytest.mark.parametrize("name", fm.APPLY_CASES)
def test_apply_matches_model_on_hand_made_cases(planners, name):
    rows, v, g, *dec = fm.apply_case(name)
    ref_v, ref_g = fm.apply_model(v, g, *dec)
    got_v, got_g = planners(rows).fleet_apply(v, g, *dec)
    _assert_state(got_v, got_g, ref_v, ref_g)
    if name in fm.KEPT_CASES:  # kept ops in more than one chunk of the compaction: no give-up, and an effect
        rc, raw_v, raw_g = _raw_apply(planners(rows), v, g, *dec)
        assert rc == TSW_OK  # FLEET_STUCK would be TSW_EHIP
        assert np.array_equal(raw_v, v) and not np.array_equal(raw_g, g)
        _assert_state(raw_v, raw_g, ref_v, ref_g)


@pytest.mark.parametrize("name,r,ticks", fm.RUN_CASES)
def test_apply_matches_model_on_decide_fleet_outputs(planners, name, r, ticks):
    rows, v, g = fc.fleet_case(name)
    p = planners(rows)
    dec = p.decide_fleet(v, g, r)
    assert dec[3][-1] > 0 and (dec[0] == fm.SWAP).any()  # rotations and swaps to apply
    ref_v, ref_g = fm.apply_model(v, g, *dec)
    got_v, got_g = p.fleet_apply(v, g, *dec)
    _assert_state(got_v, got_g, ref_v, ref_g)


# ---- fleet_run vs the model run -----------------------------------------------------------------------

@pytest.mark.parametrize("name,r,ticks", fm.RUN_CASES)
def test_run_matches_model_tick_by_tick(planners, name, r, ticks):
    rows, v, g = fc.fleet_case(name)
    ref_v, ref_g, ref_vr, ref_gr, ref_done, _ = fm.run_case(name)
    got_v, got_g, done, vr, gr = planners(rows).fleet_run(v, g, ticks, r, record=True)
    assert np.array_equal(vr, ref_vr), "v_rec: " + _first_diff(vr, ref_vr)
    assert np.array_equal(gr, ref_gr), "g_rec: " + _first_diff(gr, ref_gr)
    assert done == ref_done
    _assert_state(got_v, got_g, ref_v, ref_g)


def test_run_equals_decide_fleet_plus_apply(planners):
    rows, v, g = fc.fleet_case("rand20")
    p = planners(rows)
    sv, sg = v, g
    for _ in range(10):
        sv, sg = p.fleet_apply(sv, sg, *p.decide_fleet(sv, sg, 15))
    got_v, got_g, done = p.fleet_run(v, g, 10, 15)
    assert done == 10
    _assert_state(got_v, got_g, sv, sg)


def test_run_without_records_and_with_one_record(planners):
    rows, v, g = fc.fleet_case("dense12")
    p = planners(rows)
    _, _, ref_vr, ref_gr, _, _ = fm.run_case("dense12")
    n = v.size
    gr = np.full((n, 6), FILL, dtype=np.uint32)
    done = ctypes.c_uint32(FILL)
    v1, g1 = v.copy(), g.copy()
    assert p._lib.tsw_fleet_run(p._ctx, _p(v1), _p(g1), n, 2, 5, None, _p(gr), ctypes.byref(done)) == TSW_OK
    assert done.value == 5 and np.array_equal(gr, ref_gr[:, :6]), _first_diff(gr, ref_gr[:, :6])
    _assert_state(v1, g1, ref_vr[:, 5], ref_gr[:, 5])


# ---- fixed point, ticks == 0, n == 0 ------------------------------------------------------------------

def test_single_agent_stops_at_its_goal_and_leaves_later_columns(planners):
    rows, v, g = fm.single_agent()
    rc, v1, g1, done, vr, gr = _raw_run(planners(rows), v, g, 15, 20)
    assert rc == TSW_OK and done == 10
    assert v1.tolist() == [35] and g1.tolist() == [35]
    assert vr[0, 0] == 0 and vr[0, 10] == 35 and np.all(gr[0, :11] == 35)
    assert np.all(np.isin(np.abs(np.diff(vr[0, :11].astype(np.int64))), (1, 6)))  # one cell per tick
    assert np.all(vr[:, 11:] == FILL) and np.all(gr[:, 11:] == FILL)  # columns past ticks_done: untouched


def test_fleet_at_its_goals_is_a_fixed_point(planners):
    rows, v, _ = fc.fleet_case("rand20")
    rc, v1, g1, done, vr, gr = _raw_run(planners(rows), v, v, 15, 7)
    assert rc == TSW_OK and done == 0
    _assert_state(v1, g1, v, v)
    assert np.array_equal(vr[:, 0], v) and np.array_equal(gr[:, 0], v)
    assert np.all(vr[:, 1:] == FILL) and np.all(gr[:, 1:] == FILL)


def test_zero_ticks_writes_column_zero_only(planners):
    rows, v, g = fc.fleet_case("rand20")
    rc, v1, g1, done, vr, gr = _raw_run(planners(rows), v, g, 15, 0)
    assert rc == TSW_OK and done == 0
    _assert_state(v1, g1, v, g)
    assert vr.shape == (v.size, 1) and np.array_equal(vr[:, 0], v) and np.array_equal(gr[:, 0], g)


def test_empty_fleet(planners):
    p = planners(maps.open_map(6, 6))
    e = np.zeros(0, dtype=np.uint32)
    rc, _, _, done, _, _ = _raw_run(p, e, e, 15, 5)
    assert rc == TSW_OK and done == 0
    assert _raw_apply(p, e, e, e, e, e, np.zeros(1, dtype=np.uint32), e)[0] == TSW_OK
    v1, g1, done = p.fleet_run(e, e, 5)
    assert v1.size == g1.size == 0 and done == 0


# ---- errors -------------------------------------------------------------------------------------------

def test_blocked_cell_is_einval_and_context_stays_usable():
    rows, v, g = fc.fleet_case("dense12")
    blocked = int(np.flatnonzero(maps.rows_to_array(rows).reshape(-1) == ord("@"))[0])
    bad = v.copy()
    bad[5] = blocked
    with Planner(rows) as p:
        rc, v1, g1, done, vr, _ = _raw_run(p, bad, g, 2, 3)
        assert rc == TSW_EINVAL and done == 0 and np.array_equal(v1, bad) and np.all(vr == FILL)
        badg = g.copy()
        badg[7] = len(rows) * len(rows[0])
        assert _raw_run(p, v, badg, 2, 3)[0] == TSW_EINVAL
        with pytest.raises(TswapError):
            p.fleet_run(bad, g, 3, 2)
        _, _, ref_vr, ref_gr, _, _ = fm.run_case("dense12")
        got_v, got_g, done = p.fleet_run(v, g, 3, 2)
        assert done == 3
        _assert_state(got_v, got_g, ref_vr[:, 3], ref_gr[:, 3])


def test_list_past_the_limit_reaching_rule4_is_overflow(planners):
    """1,100 agents at r = 80: every list has 1,099 entries, and agent 0's next hop is occupied by an
    agent that is not at its goal, so the first tick's decision reaches Rule 4 with a list past the
    1,024-entry limit: TSW_EOVERFLOW, the state before that tick, and a context that still works."""
    W, H, rows, v = fc.nearby_shape("open40")
    v = v.copy()
    occupied = set(v.tolist())
    a = next(i for i, c in enumerate(v.tolist()) if c % W != W - 1 and c + 1 in occupied)
    v[[0, a]] = v[[a, 0]]  # agent 0 now stands left of an occupied cell
    b = int(np.flatnonzero(v == v[0] + 1)[0])
    g = np.full_like(v, v[-1])  # three goal cells in all: three tables to build
    g[0] = v[b]
    g[b] = v[0]
    p = planners(rows)
    rc, v1, g1, done, _, _ = _raw_run(p, v, g, 80, 4)
    assert rc == TSW_EOVERFLOW and done == 0
    assert "1024" in p._lib.tsw_last_error(p._ctx).decode()
    _assert_state(v1, g1, v, g)
    v1, g1, done = p.fleet_run(v, g, 1, 5)  # below the limit the same fleet runs
    assert done == 1 and v1[0] == v[0]  # agent 0 waits (Rule 5 finds nobody at its cell), the others move


def test_long_lists_run_on_rules_1_to_3_until_the_model_reaches_rule4(planners):
    """1,100 agents at r = 80 whose first tick is decided by Rules 1-3 alone: the run's ticks go through the
    brute-force fill's nb_v / nb_g. Three ticks equal the model's, unless the model says that an earlier
    tick reaches Rule 4 (lists of 1,099 entries: over the limit): then TSW_EOVERFLOW at exactly that tick,
    with the state and the records of the ticks before it."""
    rows, v, g, _ = fc.long_rules123()
    ref_v, ref_g, ref_vr, ref_gr, ref_done, overflow = fm.long_run_case(3)
    p = planners(rows)
    rc, v1, g1, done, vr, gr = _raw_run(p, v, g, 80, 3)
    if overflow:
        assert rc == TSW_EOVERFLOW and "1024" in p._lib.tsw_last_error(p._ctx).decode()
    else:
        assert rc == TSW_OK
    assert done == ref_done
    assert np.array_equal(vr[:, :done + 1], ref_vr), "v_rec: " + _first_diff(vr[:, :done + 1], ref_vr)
    assert np.array_equal(gr[:, :done + 1], ref_gr), "g_rec: " + _first_diff(gr[:, :done + 1], ref_gr)
    assert np.all(vr[:, done + 1:] == FILL) and np.all(gr[:, done + 1:] == FILL)
    _assert_state(v1, g1, ref_v, ref_g)


def _invalid_decisions():
    """(label, decisions) of every input tsw_fleet_apply rejects, each one change away from a valid set."""
    _, v, g, act, cell, partner, part_off, part = fm.apply_case("rotation_then_swap")
    rows = maps.open_map(8, 8)[:7] + ["@" * 8]  # the same 8 x 8 grid with a blocked last row
    good = dict(act=act, cell=cell, partner=partner, part_off=part_off, part=part)

    def change(key, index, value):
        d = {k: a.copy() for k, a in good.items()}
        d[key][index] = value
        return [d[k] for k in ("act", "cell", "partner", "part_off", "part")]

    moved = change("act", 3, fm.MOVE)
    cases = [("act > 3", change("act", 3, 4)),
             ("move off-grid", [moved[0], change("cell", 3, 64)[1], *moved[2:]]),
             ("move blocked", [moved[0], change("cell", 3, 60)[1], *moved[2:]]),
             ("partner >= n", change("partner", 1, 4)),
             ("participant >= n", change("part", 1, 4)),
             ("participant twice", change("part", 1, 2)),
             ("part_off decreasing", change("part_off", 2, 3)),
             ("rotation of one", [act, cell, partner, np.array([0, 1, 1, 1, 1], dtype=np.uint32), part[:1]])]
    return rows, v, g, [good[k] for k in ("act", "cell", "partner", "part_off", "part")], cases


def test_apply_rejects_invalid_decisions_and_leaves_v_g(planners):
    rows, v, g, good, cases = _invalid_decisions()
    p = planners(rows)
    for label, dec in cases:
        rc, v1, g1 = _raw_apply(p, v, g, *dec)
        assert rc == TSW_EINVAL, label
        assert np.array_equal(v1, v) and np.array_equal(g1, g), label
    with pytest.raises(TswapError):
        p.fleet_apply(v, g, *cases[0][1])
    rc, v1, g1 = _raw_apply(p, v, g, *good)  # the unchanged set is accepted, on the same context
    assert rc == TSW_OK
    _assert_state(v1, g1, *fm.apply_model(v, g, *good))


# ---- determinism --------------------------------------------------------------------------------------

def test_two_runs_return_identical_arrays(planners):
    rows, v, g = fc.fleet_case("warehouse")
    p = planners(rows)
    r1, r2 = p.fleet_run(v, g, 8, 15, record=True), p.fleet_run(v, g, 8, 15, record=True)
    assert r1[2] == r2[2] == 8
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2) if isinstance(a, np.ndarray))
    dec = p.decide_fleet(v, g, 15)
    a1, a2 = p.fleet_apply(v, g, *dec), p.fleet_apply(v, g, *dec)
    assert all(np.array_equal(a, b) for a, b in zip(a1, a2))
