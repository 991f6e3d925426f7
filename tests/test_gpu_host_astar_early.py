"""GPU: early asks of the host A* service (PlanArgs::hask; coop mode). A pair the walk-ahead queues as urgent
is put on the host request ring at once, a step before its code is read; refresh_codes takes the reply when
it finds the agent's code unresolved (no wait), and coop_wait spins on the remembered ticket instead of asking
again. The host and the K3 workers compute get_path's code (tswap.rs:288-390), and a late, missing or foreign
reply is ignored, so plans are bit-identical whatever TSW_HOST_ASTAR_EARLY says (0 off, 1 on, 2 early asks
only: coop_wait neither asks nor polls the host), with a ring of 8 entries (slot reuse) and with replies held
back 200 us (they arrive after their pair has moved on).

The instance is the one of tests/test_gpu_host_astar.py: warehouse 60x30, 40 agents, 400 tasks, 150 steps,
lazy next hops, the oracle plan as reference."""
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


def _plan(inst, **kw):
    rows, starts, tasks, _ = inst
    with Planner(rows, flags=TSW_F_LAZY_NEXTHOP, **kw) as p:
        rec = p.plan_mapd_arrays(starts, tasks, STEPS)
        st = p.stats()
    return (rec[0] if isinstance(rec, tuple) else rec), st


def _show(tag, st):
    print(f"{tag}: coop_waits {st['coop_waits']} wait ms {st['coop_wait_ms']:.2f} host queries "
          f"{st['host_astar_queries']} used {st['host_astar_used']} host ms {st['host_astar_ms']:.2f}")


def test_product_library_equals_oracle(inst_a):
    rec, st = _plan(inst_a)
    _show("product", st)
    assert rec.shape == inst_a[3].shape and np.array_equal(rec, inst_a[3])
    assert st["watchdog_fires"] == 0
    assert st["host_astar_used"] <= st["host_astar_queries"]


def test_early_modes_equal_oracle_and_each_other(inst_a, monkeypatch):
    """Diagnostic library, TSW_HOST_ASTAR_EARLY 0, 1 and 2. With 2 coop_wait leaves the host alone, so every
    code counted in host_astar_used was taken by refresh_codes' lazy path: > 0 proves that path runs (measured
    on this instance before the assertion was kept: 21, 22, 21, 21, 20 codes in 5 of 5 runs,
    profiles/r9/ab_c3.txt)."""
    recs = {}
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("TSW_HOST_ASTAR_EARLY", mode)
        rec, st = _plan(inst_a, diag=True)
        _show(f"early {mode}", st)
        assert rec.shape == inst_a[3].shape and np.array_equal(rec, inst_a[3])
        assert st["watchdog_fires"] == 0
        assert st["host_astar_used"] <= st["host_astar_queries"]
        if mode == "2":
            assert st["host_astar_used"] > 0
        recs[mode] = rec
    assert np.array_equal(recs["0"], recs["1"]) and np.array_equal(recs["1"], recs["2"])


@pytest.mark.parametrize("delay_us", [0, 200])
def test_ring_of_8_with_early_asks(inst_a, monkeypatch, delay_us):
    """Diagnostic library, a ring of 8 entries with early asks on: slots are reused within a few steps, so
    remembered tickets leave their window and reply slots carry other tickets' seqs; with every reply held
    back 200 us the replies also arrive after their pair has moved on."""
    monkeypatch.setenv("TSW_HOST_ASTAR_EARLY", "1")
    monkeypatch.setenv("TSW_HOST_ASTAR_RING", "8")
    if delay_us:
        monkeypatch.setenv("TSW_HOST_ASTAR_DELAY_US", str(delay_us))
    rec, st = _plan(inst_a, diag=True)
    _show(f"ring 8, delay {delay_us} us", st)
    assert np.array_equal(rec, inst_a[3])
    assert st["watchdog_fires"] == 0
    assert st["host_astar_used"] <= st["host_astar_queries"]
