"""GPU: the host A* service of the plan dispatch (tsw_opts.host_astar; coop mode). While k_plan runs,
the calling host thread answers the planner's needed (start, goal) pairs from a request ring in mapped
host memory with the host's exact A*; the K3 workers answer the same pairs, and the planner takes
whichever code arrives first. Both compute get_path's code (tswap.rs:288-390), so plans are bit-identical
with the service on, off, slow (late replies are ignored) or with a ring too small for a step's burst."""
import numpy as np
import pytest

from p2p_distributed_tswap_amd import Planner, TSW_F_LAZY_NEXTHOP, TSW_HOST_ASTAR_OFF, maps
from oracle import OracleGraph

pytestmark = pytest.mark.gpu

STEPS = 150
SEED_A = 1  # chosen on the CPU: the oracle plan of instance (a) moves agents in every one of its 150 steps


@pytest.fixture(scope="module")
def inst_a():
    """(a) warehouse 60x30, 40 agents, a well-formed 400-task stream, lazy next hops forced."""
    rows = maps.warehouse_map(60, 30, 5)
    starts, tasks = maps.make_wf_instance(rows, 40, 400, SEED_A)
    ref, _ = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, STEPS)
    assert maps.moving_timesteps(ref) == STEPS
    ref.setflags(write=False)
    return rows, starts, tasks, ref


@pytest.fixture(scope="module")
def inst_c3():
    """(b) the C3 map (warehouse 170x84), 100 agents, a well-formed 1,000-task stream."""
    rows = maps.warehouse_map(170, 84, 0x170084)
    starts, tasks = maps.make_wf_instance(rows, 100, 1000, 0x170084)
    ref, _ = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, STEPS)
    ref.setflags(write=False)
    return rows, starts, tasks, ref


def _plan(inst, flags=0, **kw):
    rows, starts, tasks, _ = inst
    with Planner(rows, flags=flags, **kw) as p:
        rec = p.plan_mapd_arrays(starts, tasks, STEPS)
        st = p.stats()
    return (rec[0] if isinstance(rec, tuple) else rec), st


def _on_off_oracle(inst, flags):
    ref = inst[3]
    on, st_on = _plan(inst, flags)
    off, st_off = _plan(inst, flags, host_astar=TSW_HOST_ASTAR_OFF)
    assert on.shape == ref.shape and np.array_equal(on, ref)
    assert off.shape == ref.shape and np.array_equal(off, ref)
    assert np.array_equal(on, off)
    assert st_off["host_astar_queries"] == 0 and st_off["host_astar_used"] == 0
    print(f"on: coop_waits {st_on['coop_waits']} wait ms {st_on['coop_wait_ms']:.2f} host queries "
          f"{st_on['host_astar_queries']} used {st_on['host_astar_used']} host ms {st_on['host_astar_ms']:.2f} | "
          f"off: coop_waits {st_off['coop_waits']} wait ms {st_off['coop_wait_ms']:.2f}")
    if st_on["coop_waits"] > 0:
        assert st_on["host_astar_queries"] > 0
    assert st_on["host_astar_used"] <= st_on["host_astar_queries"]
    assert st_on["watchdog_fires"] == 0 and st_off["watchdog_fires"] == 0


def test_lazy_warehouse_service_on_off(inst_a):
    _on_off_oracle(inst_a, TSW_F_LAZY_NEXTHOP)


def test_c3_map_service_on_off(inst_c3):
    _on_off_oracle(inst_c3, 0)


def test_late_replies_are_ignored(inst_a, monkeypatch):
    """Diagnostic library, every host reply held back 5 ms: the planner never depends on the host (the
    workers' codes end its waits) and a late reply is ignored or rewrites the same code."""
    monkeypatch.setenv("TSW_HOST_ASTAR_DELAY_US", "5000")
    rec, st = _plan(inst_a, TSW_F_LAZY_NEXTHOP, diag=True)
    print(f"delay 5 ms: coop_waits {st['coop_waits']} host queries {st['host_astar_queries']} used {st['host_astar_used']}")
    assert np.array_equal(rec, inst_a[3])
    assert st["watchdog_fires"] == 0


def test_ring_full_path(inst_a, monkeypatch):
    """Diagnostic library, a ring of 8 entries: a step's burst does not fit, the planner asks for what
    fits (or nothing) and never waits for room."""
    monkeypatch.setenv("TSW_HOST_ASTAR_RING", "8")
    rec, st = _plan(inst_a, TSW_F_LAZY_NEXTHOP, diag=True)
    print(f"ring 8: coop_waits {st['coop_waits']} host queries {st['host_astar_queries']} used {st['host_astar_used']}")
    assert np.array_equal(rec, inst_a[3])
    assert st["watchdog_fires"] == 0
