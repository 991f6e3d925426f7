"""CPU: the audit model (audit_model.audit_model, the definitions above tsw_audit_records in include/tswap.h
as brute force) on hand-built records whose counts are worked out by hand in audit_model.HAND, against
maps.moving_timesteps, on the oracle's plans (no colocation or swap in a centralized TSWAP plan) and against the colocation
counter of the decentralized run model."""
import numpy as np
import pytest

from p2p_distributed_tswap_amd import maps

import audit_model as am
import fleet_mapd_model as mm


@pytest.mark.parametrize("name", list(am.HAND))
def test_hand_built_counts(name):
    rec = am.HAND[name][0]
    got, col, agents = am.audit_model(am.HAND_ROWS, rec)
    want = am.hand_expected(name)
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)
    assert sum(got["state_steps"]) + got["bad_state"] == rec.size
    assert col.shape == (rec.shape[1], am.NCOL) and agents.shape == (rec.shape[0], am.NAGENT)


def test_hand_built_agent_words():
    # three on a cell: agents 1 and 2 are charged in column 0, agent 0 is not
    _, col, agents = am.audit_model(am.HAND_ROWS, am.HAND["three-on-a-cell"][0])
    assert agents.tolist() == [[0, 0, 0, am.NONE], [0, 0, 1, 0], [0, 0, 1, 0]]
    assert col[0].tolist() == [0, 0, 0, 3, 0, 0, 0, 2, 0, 0, 0]
    # two cross one: everybody swaps in column 1; agent 1 is also behind agent 0 in column 0
    _, col, agents = am.audit_model(am.HAND_ROWS, am.HAND["two-cross-one"][0])
    assert agents.tolist() == [[1, 0, 1, 1], [1, 0, 2, 0], [1, 0, 1, 1]]
    assert col[:, 7].tolist() == [1, 1] and col[:, 8].tolist() == [0, 3] and col[:, 5].tolist() == [0, 3]
    # deliveries per agent and per column
    _, col, agents = am.audit_model(am.HAND_ROWS, am.HAND["delivered-again"][0])
    assert agents[0].tolist() == [0, 2, 0, am.NONE] and col[:, 6].tolist() == [1, 0, 0, 1]
    # a jump and an off-map record in one column charge the agent once
    rec = am.records([[(0, 0), (6, 3)], [(1, 0), (1, 0)]])
    got, _, agents = am.audit_model(am.HAND_ROWS, rec)
    assert (got["jumps"], got["off_map"]) == (1, 1) and agents[0].tolist() == [1, 0, 1, 1]


def test_blocked_cells_are_on_grid_for_conflicts():
    # two agents on the blocked cell: both off_map, the second also a colocation
    got, _, agents = am.audit_model(am.HAND_ROWS, am.records([[(2, 1)], [(2, 1)]]))
    assert (got["off_map"], got["colocations"]) == (2, 1) and agents[:, 2].tolist() == [1, 1]
    # two agents at the same off-grid coordinates are no colocation, and a step from off the grid is no swap
    rec = am.records([[(6, 0), (5, 0)], [(6, 0), (5, 0)], [(5, 0), (6, 0)]])
    got, _, _ = am.audit_model(am.HAND_ROWS, rec)
    assert (got["colocations"], got["swaps"], got["off_map"]) == (1, 0, 3)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_moving_columns_is_moving_timesteps(seed):
    rows, rec, (got, col, _) = am.random_case(seed)
    assert got["moving_columns"] == maps.moving_timesteps(rec & np.uint64(0xFFFFFFFFFF))
    assert got["colocations"] and got["swaps"] and got["jumps"] and got["off_map"] and got["bad_state"]  # the case is busy
    still = rec.copy()
    still[:, 1:] = still[:, :1]
    assert am.audit_model(rows, still)[0]["moving_columns"] == maps.moving_timesteps(still) == 0
    # on-grid agents minus distinct cells among them, column by column
    w, h = len(rows[0]), len(rows)
    x, y = rec & np.uint64(0xFFFF), (rec >> np.uint64(16)) & np.uint64(0xFFFF)
    for t in range(rec.shape[1]):
        on = (x[:, t] < w) & (y[:, t] < h)
        assert col[t, 7] == int(on.sum()) - np.unique((y[on, t] << np.uint64(16)) | x[on, t]).size


def test_swap_walks_all_swap():
    rows = maps.random_map(20, 16, 0.2, 5)
    rec = am.swap_walks(rows, 40, 6, 4)
    got, col, _ = am.audit_model(rows, rec)
    assert col[1:, 8].tolist() == [40] * 5 and got["jumps"] == got["off_map"] == 0


@pytest.mark.parametrize("make", [
    lambda: (lambda rows: (rows, *maps.make_instance(rows, 10, 20, 7)))(maps.random_map(16, 16, 0.2, 7)),   # the smoke instance
    lambda: (lambda rows: (rows, *maps.make_instance(rows, 40, 120, 3)))(maps.random_map(20, 16, 0.2, 5)),  # rand20
], ids=["smoke", "rand20"])
def test_oracle_plans_are_clean(make):
    """No colocation, swap, off_map or bad_state in the oracle's plans. Jumps are NOT asserted: the oracle's
    plan of rand20 moves an agent two cells in one timestep 41 times (first: agent 28, column 4, (10,13) ->
    (11,12)). The oracle restates the reference's tswap_mapd step by step, so the finding belongs to the
    planner being mirrored, not to the audit."""
    from oracle import OracleGraph

    rows, starts, tasks = make()
    rec, _ = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, 2000)
    got, _, _ = am.audit_model(rows, rec)
    for kind, k in ((0, "colocations"), (1, "swaps"), (3, "off_map"), (4, "bad_state")):
        assert got[k] == 0 and got["first_t"][kind] == am.NONE, k
    assert got["moving_columns"] == maps.moving_timesteps(rec)
    assert 0 < got["deliveries"] <= tasks.shape[0]


@pytest.mark.parametrize("name", ["dense12", "rand20"])
def test_colocations_equal_the_run_models_counter(name):
    rows = mm.instance(name)[0]
    run = mm.run_case(name)
    got, _, _ = am.audit_model(rows, run.rec)
    assert got["colocations"] == run.colocated
    assert got["jumps"] == got["off_map"] == got["bad_state"] == 0
