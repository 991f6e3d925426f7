"""GPU: a context's buffers over its lifetime. One cycle runs two contexts on the 16x16 smoke map.

The default context (eager next hops on a grid this small) plans the smoke instance (10 agents / 20 tasks),
then 40 / 80 and 80 / 160 on the same context, makes one tsw_step, one tsw_fleet_run and one tsw_fleet_mapd
call, and closes. ensure_agents allocates for 64 agents at least, so it is the 80-agent plan that regrows the
thirteen agent arrays; every plan regrows the task arrays, the K4 index (32 -> 96 -> 160 entries), the
records, the K1 batch buffer and the temporaries. The eager path sizes the query queue once (65,536 entries).

The lazy context (TSW_F_LAZY_NEXTHOP: the coop dispatch) plans 10 / 20 and 80 / 160 over 300 timesteps. Its first plan regrows
the query queue (4 n + 4096 -> 2^18 entries) and allocates the coop members (control blocks, speculative,
chain, hot and predicted queues, early asks, walk frontier, worker scratch); its second regrows the agent
arrays and the per-agent / per-task ones of them.

Every plan and the step are checked bit-exact against the oracle, so the regrown buffers are proven usable;
after twelve cycles the device's free memory must be what it was after two."""
import functools

import numpy as np
import pytest

from p2p_distributed_tswap_amd import Planner, TSW_F_LAZY_NEXTHOP, maps
from oracle import OracleGraph

pytestmark = pytest.mark.gpu

MAX_T = 2000
LAZY_MAX_T = 300  # the lazy context's plans: its buffers do not depend on the horizon (below 2^21 agent-steps)
# Free-memory drop allowed over cycles 3 .. 12, bytes. The expected drop is zero; the bound only keeps the
# runtime's own allocator caching from failing the test. profiles/r13/ctx_cycle_mem.txt:
#   parent (4caa351), three repeats of this test: free 308109377536 -> 308109377536 bytes each, drop 0, 0, 0
#   bound (MAX_DROP_BYTES) = largest drop + spread = 0 bytes
MAX_DROP_BYTES = 0


@functools.lru_cache(maxsize=None)
def _case():
    """The instances of one cycle and their oracle results, computed once (do not modify)."""
    rows = maps.random_map(16, 16, 0.2, 7)
    cells = maps.rows_to_array(rows)
    og = OracleGraph(cells)
    plans = []
    # the smoke() instance, one that outgrows its task buffers, one that outgrows the 64-agent floor too
    for n, m in ((10, 20), (40, 80), (80, 160)):
        starts, tasks = maps.make_instance(rows, n, m, 7)
        plans.append((starts, tasks, MAX_T, *og.mapd(starts, tasks, MAX_T, trace_goals=True)))
    lazy = [(p[0], p[1], LAZY_MAX_T, *og.mapd(p[0], p[1], LAZY_MAX_T, trace_goals=True)) for p in (plans[0], plans[2])]
    # the smallest sizes of the existing tests: test_step_matches_oracle's 40 agents, the single agent of
    # test_gpu_fleet_run and the 1 agent / 3 tasks of fleet_mapd_model's "single"
    comp = maps.largest_component(rows)
    cellid = np.array([y * cells.shape[1] + x for (x, y) in comp], dtype=np.uint32)
    idx = np.random.default_rng(1).choice(len(comp), size=80, replace=True)
    v, g = cellid[idx[:40]], cellid[idx[40:]].copy()
    g[:8] = v[:8]
    step = (v, g, *og.step(v, g))
    one = (cellid[:1].copy(), cellid[-1:].copy())
    mapd = maps.make_instance(rows, 1, 3, 2)
    return rows, plans, lazy, step, one, mapd


def _plan(p, plan):
    starts, tasks, max_t, ref, ref_goals = plan
    rec, goals = p.plan_mapd_arrays(starts, tasks, max_t, trace_goals=True)
    assert rec.shape == ref.shape and np.array_equal(rec, ref) and np.array_equal(goals, ref_goals), \
        f"plan of {starts.shape[0]} agents differs from the oracle"


def _cycle():
    rows, plans, lazy, (v, g, ref_v, ref_g), (v1, g1), (starts1, tasks1) = _case()
    with Planner(rows, device=0, flags=TSW_F_LAZY_NEXTHOP) as p:
        for plan in lazy:
            _plan(p, plan)
        st = p.stats()
        assert st["coop_workers"] > 0 and st["bfs_goals"] > 0  # the coop dispatch ran, on tables built here
    with Planner(rows, device=0) as p:
        for plan in plans:
            _plan(p, plan)
        hv, hg = p.step(v, g)
        assert np.array_equal(hv, ref_v) and np.array_equal(hg, ref_g)
        rv, rg, done, vr, gr = p.fleet_run(v1, g1, 20, 15, record=True)
        assert done <= 20 and rv[0] == vr[0, done] and vr.shape == (1, done + 1) and gr.shape == vr.shape
        rec, stalled = p.fleet_mapd(starts1, tasks1, 100, 15)
        assert rec.shape[0] == 1 and rec.shape[1] > 0 and not stalled


def _free_bytes():
    """The device's free memory, the figure torch.cuda.mem_get_info() reports: hipMemGetInfo of the HIP runtime
    the library itself links. torch's bundled runtime cannot open the device in a process where the library's
    is already up ("No HIP GPUs are available"; test_gpu_bfs._DevBuf has the same constraint)."""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so.7")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_context_cycles_return_their_memory():
    for _ in range(2):  # the runtime's own first-use allocations (code objects, pools) happen here
        _cycle()
    before = _free_bytes()
    for _ in range(10):
        _cycle()
    after = _free_bytes()
    print(f"ctx cycles: free {before} -> {after} bytes, drop {before - after}")
    assert before - after <= MAX_DROP_BYTES, f"free device memory dropped by {before - after} bytes over 10 cycles"
