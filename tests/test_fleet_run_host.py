"""CPU: the lock-step decentralized run (tsw_fleet_apply / tsw_fleet_run) is declared in every mirror of
the C ABI without an ABI bump, and the plain-Python model of it (fleet_run_model.py) reaches on the recipe
fleets what the GPU comparison relies on, and gives the literal results worked out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg
from p2p_distributed_tswap_amd import maps
from oracle import OracleGraph

import fleet_cases as fc
import fleet_run_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsw_fleet_apply", "tsw_fleet_run")


def test_fleet_run_entry_points_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tswap.h")).read()
    rs = open(os.path.join(ROOT, "rust", "tswap-amd-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in pkg.EXPORTED_SYMBOLS
        assert re.search(rf"\bint {name}\(tsw_ctx \*ctx", hdr), name
        assert re.search(rf"pub fn {name}\(ctx: \*mut TswCtx", rs), name
    assert re.search(r"pub fn fleet_apply\(&mut self", rs) and re.search(r"pub fn fleet_run\(&mut self", rs)
    assert hasattr(pkg.Planner, "fleet_apply") and hasattr(pkg.Planner, "fleet_run")
    # two functions were added, nothing else changed: the revision stays
    assert re.search(r"#define TSW_ABI_VERSION 8\b", hdr)
    if os.path.exists(pkg.LIB_PATH):
        for path in (pkg.LIB_PATH, pkg.DIAG_LIB_PATH):
            lib = ctypes.CDLL(path)
            for name in NAMES:
                assert hasattr(lib, name), (path, name)


@pytest.mark.parametrize("name,r,ticks", fm.RUN_CASES)
def test_model_run_reaches_what_the_gpu_test_relies_on(name, r, ticks):
    rows, v0, g0 = fc.fleet_case(name)
    free = maps.rows_to_array(rows).reshape(-1) != ord("@")
    v, g, v_rec, g_rec, done, dec = fm.run_case(name)
    assert done == ticks  # no fixed point within the ticks
    assert v_rec.shape == g_rec.shape == (v0.size, ticks + 1)
    assert np.array_equal(v_rec[:, 0], v0) and np.array_equal(v_rec[:, -1], v)
    assert np.array_equal(g_rec[:, 0], g0) and np.array_equal(g_rec[:, -1], g)
    assert set(np.unique(g_rec).tolist()) <= set(g0.tolist())  # goals stay within the initial goal set
    assert np.all(free[v_rec])  # cells stay free
    kinds, contended, shared = set(), 0, 0
    for t, (act, cell, partner, part_off, part) in enumerate(dec):
        kinds |= set(act.tolist())
        count = {}
        for i in np.flatnonzero((act == fm.SWAP) | (act == fm.ROTATION)):
            i = int(i)
            if act[i] == fm.SWAP:
                assert v_rec[partner[i], t] == g_rec[partner[i], t]  # every swap partner is at its goal
            else:
                P = fm.touched(i, act, partner, part_off, part)
                assert len(P) >= 2 and len(set(P)) == len(P) and i not in P
            for a in set(fm.touched(i, act, partner, part_off, part)):
                count[a] = count.get(a, 0) + 1
        contended += bool(count) and max(count.values()) >= 2
        entered = cell[(act == fm.MOVE) & (cell != v_rec[:, t])]
        shared += np.unique(entered).size < entered.size
    assert kinds == {fm.MOVE, fm.SWAP, fm.ROTATION, fm.WAIT}
    assert contended == {"dense12": 2, "rand20": 4, "warehouse": 6}[name]  # ticks with an agent in 2+ goal ops
    assert shared > 0  # moves into a shared cell


def test_two_requesters_of_one_partner():
    _, v, g, *dec = fm.apply_case("two_requesters")
    v1, g1 = fm.apply_model(v, g, *dec)
    # turn 1: G = [g1, g0, g2]; turn 2 exchanges G[2] with what agent 0 holds by then
    assert g.tolist() == [10, 11, 12] and g1.tolist() == [12, 10, 11]
    assert np.array_equal(v1, v)
    assert fm.goal_op_rounds(dec[0], dec[2], dec[3], dec[4]) == 2


def test_three_rotations_duplicate_a_goal():
    """Each of three agents initiates a rotation over the other two. Every request carries tick-start
    goals, so the last writer of each agent wins and goal 10 ends up twice, goal 12 nowhere: that is the
    reference's protocol (handler agent.rs:1090-1107), not something to repair here."""
    _, v, g, *dec = fm.apply_case("rotation_3cycle")
    v1, g1 = fm.apply_model(v, g, *dec)
    assert g.tolist() == [10, 11, 12] and g1.tolist() == [11, 10, 10]
    assert fm.goal_op_rounds(dec[0], dec[2], dec[3], dec[4]) == 3


def test_rotation_and_swap_order_matters():
    _, v, g, *dec = fm.apply_case("rotation_then_swap")
    assert fm.apply_model(v, g, *dec)[1].tolist() == [10, 13, 11, 12]  # rotation [.., .., 13, 12], then 1 <-> 2
    _, v, g, *dec = fm.apply_case("swap_then_rotation")
    assert fm.apply_model(v, g, *dec)[1].tolist() == [12, 11, 13, 12]  # swap [12, .., 10, ..], then g0 values


def test_two_moves_into_one_cell():
    _, v, g, *dec = fm.apply_case("two_moves_one_cell")
    v1, g1 = fm.apply_model(v, g, *dec)
    assert v1.tolist() == [1, 1, 20] and np.array_equal(g1, g)


def test_single_agent_reaches_its_goal_in_ten_ticks():
    rows, v, g = fm.single_agent()
    v1, g1, v_rec, g_rec, done, _ = fm.run_model(OracleGraph(maps.rows_to_array(rows)), rows, v, g, 15, 20)
    assert done == 10 and v1.tolist() == [35] and g1.tolist() == [35]
    assert v_rec.shape == (1, 11) and np.all(g_rec == 35)
    steps = np.abs(np.diff(v_rec[0].astype(np.int64)))
    assert set(steps.tolist()) <= {1, 6}  # one cell per tick


def test_big_cases_are_what_they_claim():
    _, v, g, act, cell, partner, part_off, part = fm.apply_case("chain200")
    assert fm.goal_op_rounds(act, partner, part_off, part) == 200
    _, v, g, act, cell, partner, part_off, part = fm.apply_case("disjoint1500")
    assert int((act == fm.SWAP).sum()) == 1500 and fm.goal_op_rounds(act, partner, part_off, part) == 1
    _, v, g, act, cell, partner, part_off, part = fm.apply_case("rotation70")
    assert part_off[1] - part_off[0] == 70 and 0 not in part.tolist() and np.unique(part).size == 70
