"""GPU: the planner's step-start walk-ahead (nextnext_prefetch, round 10) only decides when a pair is queued,
never what a code is, so plans are bit-identical whatever its budget (TSW_WALK_STEP: 0 the whole depth at
once, 1, the default), with and without its cached frontier (TSW_WALK_CACHE), and with the host A* service
off (TSW_HOST_ASTAR=0: the K3 workers alone carry the speculation). In every run the workers must have
resolved speculative pairs (coop_worker_queries[1] > 0) and the watchdog must not have fired.

The instance is the one of tests/test_gpu_host_astar_early.py: warehouse 60x30, 40 agents, 400 tasks, 150
steps, lazy next hops, the oracle plan as reference. Beside it: tsw_step chained over 20 steps (MODE_STEP: no
budget, the frontier is re-armed per call), and a 9x9 open grid on which two agents meet head-on in row 3 and
the rules rotate their goals at step 3 — each then holds a goal whose path the other had walked ahead."""
import numpy as np
import pytest

from p2p_distributed_tswap_amd import Planner, TSW_F_LAZY_NEXTHOP, maps
from oracle import OracleGraph

pytestmark = pytest.mark.gpu

STEPS = 150
SEED_A = 1  # the oracle plan of this instance moves agents in every one of its 150 steps


@pytest.fixture(scope="module")
def inst_a():
    rows = maps.warehouse_map(60, 30, 5)
    starts, tasks = maps.make_wf_instance(rows, 40, 400, SEED_A)
    ref, _ = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, STEPS)
    assert maps.moving_timesteps(ref) == STEPS
    ref.setflags(write=False)
    return rows, starts, tasks, ref


def _plan(inst, steps=STEPS, **kw):
    rows, starts, tasks = inst[:3]
    with Planner(rows, flags=TSW_F_LAZY_NEXTHOP, **kw) as p:
        rec = p.plan_mapd_arrays(starts, tasks, steps)
        st = p.stats()
    return (rec[0] if isinstance(rec, tuple) else rec), st


def _check(tag, rec, st, ref):
    print(f"{tag}: worker queries {st['coop_worker_queries']} coop_waits {st['coop_waits']} "
          f"host used {st['host_astar_used']} watchdog {st['watchdog_fires']}")
    assert rec.shape == ref.shape and np.array_equal(rec, ref), tag
    assert st["watchdog_fires"] == 0, tag
    assert st["coop_worker_queries"][1] > 0, tag  # speculation really ran


def test_product_library_equals_oracle(inst_a):
    rec, st = _plan(inst_a)
    _check("product", rec, st, inst_a[3])


@pytest.mark.parametrize("host", [None, "0"])
@pytest.mark.parametrize("cache", ["1", "0"])
def test_budgets_equal_oracle_and_each_other(inst_a, monkeypatch, cache, host):
    """Diagnostic library: TSW_WALK_STEP 0, 1 and the default, with and without the frontier cache, with the
    host A* service as configured and off."""
    monkeypatch.setenv("TSW_WALK_CACHE", cache)
    if host is not None:
        monkeypatch.setenv("TSW_HOST_ASTAR", host)
    recs = []
    for step in ("0", "1", None):
        if step is None:
            monkeypatch.delenv("TSW_WALK_STEP", raising=False)
        else:
            monkeypatch.setenv("TSW_WALK_STEP", step)
        rec, st = _plan(inst_a, diag=True)
        _check(f"cache {cache} host {host} walk_step {step}", rec, st, inst_a[3])
        recs.append(rec)
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[1], recs[2])


def test_step_mode_chained_20_steps(inst_a):
    """tsw_step (MODE_STEP) chained over 20 steps from the instance's start cells toward fixed random goals."""
    rows, starts = inst_a[0], inst_a[1]
    cells = maps.rows_to_array(rows)
    w = cells.shape[1]
    comp = maps.largest_component(rows)
    cid = np.array([y * w + x for (x, y) in comp], dtype=np.uint32)
    rng = np.random.default_rng(10)
    v = (starts[:, 1] * w + starts[:, 0]).astype(np.uint32)
    g = cid[rng.choice(cid.size, v.size, replace=False)]
    og = OracleGraph(cells)
    with Planner(rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        for tick in range(20):
            rv, rg = og.step(v, g)
            hv, hg = p.step(v, g)
            assert np.array_equal(hv, rv) and np.array_equal(hg, rg), f"tick {tick}"
            v, g = rv, rg
        assert p.stats()["watchdog_fires"] == 0


def test_goals_exchanged_by_a_rotation_9x9(monkeypatch):
    """Two agents pick up at (7,3) and (2,3) and deliver at (0,3) and (8,3): they meet head-on in row 3 after
    two steps (five apart, an odd distance, so they stand on adjacent cells) and the rules phase of step 3
    rotates their goals. Product and diagnostic library (default budget and the whole depth at once)."""
    rows = maps.open_map(9, 9)
    starts = np.array([[7, 4], [2, 4]], dtype=np.uint32)
    tasks = np.array([[7, 3, 0, 3], [2, 3, 8, 3]], dtype=np.uint32)
    ref, rgoals = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, 30, trace_goals=True)
    a, b = 3 * 9 + 0, 3 * 9 + 8
    assert list(rgoals[:, 2]) == [a, b] and list(rgoals[:, 3]) == [b, a]  # the known step
    for kw, step in (({}, None), ({"diag": True}, None), ({"diag": True}, "0")):
        if step is not None:
            monkeypatch.setenv("TSW_WALK_STEP", step)
        with Planner(rows, flags=TSW_F_LAZY_NEXTHOP, **kw) as p:
            rec, goals = p.plan_mapd_arrays(starts, tasks, 30, trace_goals=True)
            st = p.stats()
        assert np.array_equal(rec, ref) and np.array_equal(goals, rgoals), (kw, step)
        assert st["watchdog_fires"] == 0
