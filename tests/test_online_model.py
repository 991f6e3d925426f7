"""CPU: the Python model of tsw_plan_mapd_online (tests/online_model.py) against the oracle. With every task
released at 0 the model is the reference loop, so it must give OracleGraph.mapd(..., trace_goals=True) bit for bit on
the committed golden instances; a release time changes what it may change and nothing else."""
import os

import numpy as np
import pytest

from online_model import online_mapd
from oracle import OracleGraph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["mapd_rand12", "mapd_rand16_dense", "mapd_open8"])
@pytest.mark.parametrize("release", ["zeros", "none"])
def test_model_release_zero_is_the_oracle(name, release):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    grid, starts, tasks, max_t = z["grid"], z["starts"], z["tasks"], int(z["max_t"])
    graph = OracleGraph(grid)
    ref, rgoals = graph.mapd(starts, tasks, max_t, trace_goals=True)
    rel = np.zeros(len(tasks), dtype=np.uint32) if release == "zeros" else None
    rec, goals, T, cnt = online_mapd(grid, starts, tasks, rel, max_t, graph=graph)
    assert T == ref.shape[1]
    assert np.array_equal(rec, ref)
    assert np.array_equal(goals, rgoals)
    assert cnt["segments"] == 1 and cnt["never_released"] == 0
    # the committed records are the same plan
    assert np.array_equal(ref, z["rec"][:, :T])


def test_model_release_changes_only_what_it_may():
    z = np.load(os.path.join(GOLDEN, "mapd_open8.npz"))
    grid, starts, tasks = z["grid"], z["starts"], z["tasks"]
    m = len(tasks)
    # nothing released until column 7: seven columns at rest, then the release-0 plan shifted by 7
    base, bgoals, bT, _ = online_mapd(grid, starts, tasks, None, 200)
    rec, goals, T, cnt = online_mapd(grid, starts, tasks, np.full(m, 7), 200)
    assert T == bT + 7 and cnt["segments"] == 2 and cnt["held"] >= 6
    assert np.array_equal(rec[:, 7:], base) and np.array_equal(goals[:, 7:], bgoals)
    assert (rec[:, :7] == rec[:, :1]).all() and ((rec[:, :7] >> np.uint64(32)) == 3).all()
    # a task that is never released keeps the run alive to max_t
    rel = np.zeros(m, dtype=np.uint32)
    rel[3] = 41
    rec, goals, T, cnt = online_mapd(grid, starts, tasks, rel, 40)
    assert T == 41 and cnt["never_released"] == 1 and cnt["segments"] == 1
