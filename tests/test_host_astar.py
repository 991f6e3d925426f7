"""CPU: the host's exact A* (tsw_host_next_hop_codes, csrc/tsw_host_astar.cpp — the search the plan
dispatch's host service runs) against the oracle's get_path (tswap.rs:288-390): BinaryHeap tie order,
S,E,N,W neighbour order, label propagation, the unreachable-goal fallback and start == goal. No device
is involved: the entry point takes the cell array itself."""
import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg
from p2p_distributed_tswap_amd import maps
from oracle import OracleGraph


def _lib_or_skip():
    import os

    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("libtswap_hip.so not built (run __graft_entry__.build())")


def _next_cells(rows, start, goal):
    """The host A*'s codes as next cells (code 4 = stay)."""
    w = len(rows[0])
    code = pkg.host_next_hop_codes(rows, start, goal)
    assert code.max(initial=0) <= 4
    step = np.array([w, 1, -w, -1, 0], dtype=np.int64)
    return (np.asarray(start, dtype=np.int64) + step[code]).astype(np.uint32), code


def _check(rows, start, goal):
    og = OracleGraph(maps.rows_to_array(rows))
    got, code = _next_cells(rows, start, goal)
    ref = np.array([og.get_path_next(int(s), int(g))[0] for s, g in zip(start, goal)], dtype=np.uint32)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, (f"{bad.size} of {len(start)} differ; first: start {start[bad[0]]} goal {goal[bad[0]]} "
                           f"host {got[bad[0]]} (code {code[bad[0]]}) oracle {ref[bad[0]]}")
    return code


def _free_cells(rows):
    a = maps.rows_to_array(rows)
    return np.nonzero(a.reshape(-1) != ord("@"))[0].astype(np.uint32)


def _pairs(rows, k, seed):
    """k seeded pairs of free cells (any two: pairs across components take the fallback)."""
    free = _free_cells(rows)
    rng = np.random.default_rng(seed)
    return free[rng.integers(0, free.size, k)], free[rng.integers(0, free.size, k)]


def test_open_8x8_all_pairs():
    """An open grid ties everywhere: every (start, goal) pair, start == goal included."""
    _lib_or_skip()
    rows = maps.open_map(8, 8)
    s, g = np.meshgrid(np.arange(64, dtype=np.uint32), np.arange(64, dtype=np.uint32), indexing="ij")
    code = _check(rows, s.reshape(-1), g.reshape(-1))
    assert (code.reshape(64, 64).diagonal() == 4).all()


@pytest.mark.parametrize("name,rows,seed", [
    ("random24", maps.random_map(24, 24, 0.2, 7), 11),
    ("warehouse60x30", maps.warehouse_map(60, 30, 5), 12),
    ("cave40x41", maps.cave_map(40, 41, 3), 13),
])
def test_seeded_pairs(name, rows, seed):
    _lib_or_skip()
    s, g = _pairs(rows, 400, seed)
    _check(rows, s, g)


def test_unreachable_goal_takes_the_fallback():
    """A wall splits the grid: the next hop is the first S,E,N,W neighbour closer in Manhattan
    distance (tswap.rs:378-389), or the start itself when there is none."""
    _lib_or_skip()
    rows = ["....@...",
            "....@...",
            "....@...",
            "....@..."]
    w = 8
    start = np.array([0 * w + 0, 1 * w + 3, 3 * w + 3, 0 * w + 7], dtype=np.uint32)
    goal = np.array([3 * w + 7, 1 * w + 6, 0 * w + 5, 2 * w + 1], dtype=np.uint32)
    code = _check(rows, start, goal)
    assert code[1] == 4  # (3, 1) -> (6, 1): east is the wall and no other neighbour is closer


def test_start_equals_goal():
    _lib_or_skip()
    rows = maps.random_map(24, 24, 0.2, 7)
    free = _free_cells(rows)[:50]
    code = _check(rows, free, free)
    assert (code == 4).all()


def test_corridor_1xn():
    _lib_or_skip()
    rows = ["." * 37]
    s, g = np.meshgrid(np.arange(37, dtype=np.uint32), np.arange(37, dtype=np.uint32), indexing="ij")
    _check(rows, s.reshape(-1), g.reshape(-1))
    rows = [["."] for _ in range(19)]
    rows = ["".join(r) for r in rows]
    s, g = np.meshgrid(np.arange(19, dtype=np.uint32), np.arange(19, dtype=np.uint32), indexing="ij")
    _check(rows, s.reshape(-1), g.reshape(-1))


def test_bad_cells_are_refused():
    _lib_or_skip()
    rows = ["..@", "..."]
    for s, g in (([2], [0]), ([0], [2]), ([6], [0]), ([0], [6])):
        with pytest.raises(pkg.TswapError):
            pkg.host_next_hop_codes(rows, np.array(s, dtype=np.uint32), np.array(g, dtype=np.uint32))
