"""Instances for the tests of the in-dispatch K3 workers (tsw_worker.h), chosen by the CPU oracle. No GPU use.

The workers' A* branches on the start cell's detour toward its goal, delta(v) = (D[v] - |v - goal|_1) / 2
(D = the goal's BFS distance): the byte g-scores (astar_wave_par<2>) hold a node's detour from the START in
5 bits, and the goal's own g-score byte is delta(v), so a query overflows to tier 2 from delta = 32 on; the
table store's detour bytes hold delta up to 254 and saturate at 255 (DAG early exit off). The serpentine map
has cells of every such class for any goal, and step_instance() picks multi-candidate cells (the ones K1
leaves at 0xFF, i.e. the ones that need the A*) of each class around these edges.
"""
from __future__ import annotations

import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from p2p_distributed_tswap_amd import maps

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
from py_restatement import Graph, RustBinaryHeap, _Node  # noqa: E402

INF = 0xFFFF
NH_STAY, NH_UNKNOWN = 4, 0xFF
ASTAR = 0xFE  # in MapRef.k1: the oracle's get_path decides (several candidates)
_NONE = 0xEE  # in MapRef._memo: not computed yet
DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0))  # S, E, N, W (tswap.rs:62)
# delta classes: 30..33 straddle the byte g-scores' 5-bit field (delta 31 = a 62-cell detour fits, 32 overflows
# to tier 2), 61..64 lie well past it (every query of these classes is a tier-2 query unless the early exit
# ends it first), 253..256 straddle the detour-byte saturation (254 the last exact byte, 255 the saturated one)
CLASSES = (0, 1, 30, 31, 32, 33, 61, 62, 63, 64, 253, 254, 255, 256)
SEED = 7


def serpentine(W: int, H: int) -> list:
    """Walls down every 4th column from x = 3, one gap per wall alternating between row H - 2 and row 1:
    paths snake through the gaps, so detours reach hundreds of cells."""
    a = np.zeros((H, W), dtype=bool)
    for i, x in enumerate(range(3, W, 4)):
        a[:, x] = True
        a[(1 if i % 2 else H - 2), x] = False
    return maps.to_rows(a)


def detour_classes(og, cells: np.ndarray, goal: int):
    """(delta, multi) per cell for `goal`: delta = (D - Manhattan) / 2 (-1 at blocked and unreachable cells),
    multi = at least 2 free neighbours at distance D - 1 (K1 leaves the cell's code at 0xFF: get_path's
    tie-break decides)."""
    H, W = cells.shape
    D = og.bfs(goal).astype(np.int64).reshape(H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    man = np.abs(xs - goal % W) + np.abs(ys - goal // W)
    ok = D != INF
    delta = np.where(ok, (D - man) // 2, -1)
    P = np.pad(D, 1, constant_values=INF)  # blocked cells hold INF in the oracle's table too
    cand = sum((P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == D - 1).astype(np.int64)
               for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0)))
    multi = ok & (cand >= 2)
    return delta.reshape(-1), multi.reshape(-1)


def step_instance(rows, seed: int = SEED, n_goals: int = 8, per_class: int = 4, bulk: int = 120):
    """(v, g) of distinct agent cells: for each of n_goals goals up to per_class multi-candidate cells of
    every delta class of CLASSES plus `bulk` random multi-candidate cells, all heading to that goal."""
    from oracle import OracleGraph

    cells = maps.rows_to_array(rows)
    og = OracleGraph(cells)
    free = np.flatnonzero(cells.reshape(-1) != ord("@"))
    rng = np.random.default_rng(seed)
    goals = rng.choice(free, n_goals, replace=False)
    taken = np.zeros(cells.size, dtype=bool)
    v, g = [], []
    for goal in goals:
        delta, multi = detour_classes(og, cells, int(goal))
        for cl in CLASSES:
            pool = np.flatnonzero(multi & (delta == cl) & ~taken)
            pick = rng.choice(pool, min(per_class, pool.size), replace=False)
            taken[pick] = True
            v.extend(int(c) for c in pick)
            g.extend([int(goal)] * pick.size)
        pool = np.flatnonzero(multi & ~taken)
        pick = rng.choice(pool, min(bulk, pool.size), replace=False)
        taken[pick] = True
        v.extend(int(c) for c in pick)
        g.extend([int(goal)] * pick.size)
    return np.array(v, dtype=np.uint32), np.array(g, dtype=np.uint32)


def saturation_instance(rows, seed: int = SEED, n_goals: int = 8):
    """(v, g) for step_instance's goals: ALL multi-candidate cells whose detour byte is the last exact one (254),
    just saturated (255: d* = h + 2 * 255 still holds, but DAG cells with byte 255 are invisible to the byte
    test, so the early exit must be off) or past it (256)."""
    from oracle import OracleGraph

    cells = maps.rows_to_array(rows)
    og = OracleGraph(cells)
    free = np.flatnonzero(cells.reshape(-1) != ord("@"))
    goals = np.random.default_rng(seed).choice(free, n_goals, replace=False)
    taken = np.zeros(cells.size, dtype=bool)
    v, g = [], []
    for goal in goals:
        delta, multi = detour_classes(og, cells, int(goal))
        pick = np.flatnonzero(multi & (delta >= 254) & (delta <= 256) & ~taken)
        taken[pick] = True
        v.extend(int(c) for c in pick)
        g.extend([int(goal)] * pick.size)
    return np.array(v, dtype=np.uint32), np.array(g, dtype=np.uint32)


class _LabNode(_Node):
    __slots__ = ("lab",)


def byte_exit_model(rows, det, v: int, goal: int, mask: int, off_when_saturated: bool = True):
    """Direction of path[1] as astar_wave_par<*, *, DAG> decides it, on the restated BinaryHeap: after every
    (mask + 1)-th pop the heap entries with byte != 255 and g + h + 2 * byte == d* = h(v) + 2 * byte(v) are
    the visible DAG nodes; one label among them (or the goal among them) ends the search. det: the goal's
    detour bytes. off_when_saturated=False drops the `byte(v) != 255` condition (what the tests must catch)."""
    W, H = len(rows[0]), len(rows)
    gx, gy = goal % W, goal // W

    def h(c):
        return abs(c % W - gx) + abs(c // W - gy)

    dstar = h(v) + 2 * int(det[v])
    ee = det[v] != 255 or not off_when_saturated
    heap = RustBinaryHeap()
    gs = {v: 0}
    first = _LabNode(v, 0, h(v))
    first.lab = NH_STAY
    heap.push(first)
    pops = 0
    while heap.data:
        cur = heap.pop()
        pops += 1
        c = cur.node_id
        if c == goal:
            return cur.lab
        for d, (dx, dy) in enumerate(DIRS):
            nx, ny = c % W + dx, c // W + dy
            if not (0 <= nx < W and 0 <= ny < H and rows[ny][nx] != "@"):
                continue
            n, tg = ny * W + nx, cur.g_cost + 1
            if tg < gs.get(n, 1 << 30):
                gs[n] = tg
                e = _LabNode(n, tg, tg + h(n))
                e.lab = d if c == v else cur.lab
                heap.push(e)
        if ee and (pops & mask) == 0:
            dag = [e for e in heap.data if det[e.node_id] != 255 and e.g_cost + h(e.node_id) + 2 * int(det[e.node_id]) == dstar]
            at_goal = [e.lab for e in dag if e.node_id == goal]
            if at_goal:
                return at_goal[0]
            if len({e.lab for e in dag}) == 1:
                return dag[0].lab
    return NH_STAY


def instance_classes(rows, v, g):
    """(delta, multi) of every agent's own (v[i], g[i]) pair."""
    from oracle import OracleGraph

    cells = maps.rows_to_array(rows)
    og = OracleGraph(cells)
    delta = np.zeros(v.size, dtype=np.int64)
    multi = np.zeros(v.size, dtype=bool)
    for goal in np.unique(g):
        d, m = detour_classes(og, cells, int(goal))
        sel = g == goal
        delta[sel] = d[v[sel]]
        multi[sel] = m[v[sel]]
    return delta, multi


# the two plan instances of tests/test_gpu_workers.py: (map, agents, tasks, instance seed, max_t)
def plan_serpentine():
    rows = serpentine(200, 130)
    starts, tasks = maps.make_instance(rows, 40, 80, SEED)
    return rows, starts, tasks, 60


def plan_cave():
    rows = maps.cave_map(128, 97, 9)
    starts, tasks = maps.make_instance(rows, 100, 200, SEED)
    return rows, starts, tasks, 40


def plan_pairs(rows, starts, tasks, n: int, seed: int):
    """n seeded (cell, goal) pairs of a plan instance, as its agents and task chains query them: a cell of the
    largest component toward a task cell (pickup or delivery)."""
    W = len(rows[0])
    comp = np.array([y * W + x for (x, y) in maps.largest_component(rows)], dtype=np.uint32)
    ends = np.concatenate([tasks[:, 1] * W + tasks[:, 0], tasks[:, 3] * W + tasks[:, 2]]).astype(np.uint32)
    rng = np.random.default_rng(seed)
    return rng.choice(comp, n), rng.choice(ends, n)


class _PeakHeap(RustBinaryHeap):
    peak = 0

    def push(self, item):
        super().push(item)
        _PeakHeap.peak = max(_PeakHeap.peak, len(self.data))


def heap_peaks(rows, v, g) -> list:
    """The restated BinaryHeap's peak length in get_path(v[i], g[i]) (oracle/py_restatement.py), per pair."""
    import py_restatement

    gr = Graph(rows)
    W = len(rows[0])
    out = []
    saved = py_restatement.RustBinaryHeap
    py_restatement.RustBinaryHeap = _PeakHeap
    try:
        for a, b in zip(v, g):
            _PeakHeap.peak = 0
            gr.get_path(gr.pos2id[(int(a) % W, int(a) // W)], gr.pos2id[(int(b) % W, int(b) // W)])
            out.append(_PeakHeap.peak)
    finally:
        py_restatement.RustBinaryHeap = saved
    return out


class MapRef:
    """The oracle side of one map for the store checks, computed once per module and shared (read-only
    results): per goal the codes the BFS table alone decides, and a memo of get_path's codes for the rest."""

    def __init__(self, rows):
        from oracle import OracleGraph

        self._OG = OracleGraph
        self.rows = rows
        self.cells = maps.rows_to_array(rows)
        self.H, self.W = self.cells.shape
        self.free = self.cells.reshape(-1) != ord("@")
        self.og = OracleGraph(self.cells)
        self._k1 = {}
        self._memo = {}
        self._pool = None
        self.oracle_s = 0.0
        self.oracle_calls = 0

    def k1(self, goal: int) -> np.ndarray:
        """Per cell: 0xFF blocked, 4 the goal, 0..3 the one free neighbour at D - 1, ASTAR with several; a free
        cell that does not reach the goal holds get_path's fallback (tswap.rs:378-389): the first neighbour
        in S, E, N, W order that is closer to the goal in Manhattan distance, else 4."""
        if goal not in self._k1:
            H, W = self.H, self.W
            D = self.og.bfs(goal).astype(np.int64).reshape(H, W)
            P = np.pad(D, 1, constant_values=INF)
            F = np.pad(self.free.reshape(H, W), 1, constant_values=False)
            ys, xs = np.mgrid[0:H, 0:W]
            gx, gy = goal % W, goal // W
            cnt = np.zeros((H, W), dtype=np.int64)
            code = np.zeros((H, W), dtype=np.uint8)
            fall = np.full((H, W), NH_STAY, dtype=np.uint8)
            closer = (ys < gy, xs < gx, ys > gy, xs > gx)  # stepping S, E, N, W brings the cell closer
            for d in (3, 2, 1, 0):  # descending: the first direction in S, E, N, W order wins
                dx, dy = DIRS[d]
                fall[F[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] & closer[d]] = d
            for d, (dx, dy) in enumerate(DIRS):
                m = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == D - 1
                cnt += m
                code[m] = d
            out = np.where(D == INF, fall, np.where(cnt == 1, code, ASTAR)).astype(np.uint8).reshape(-1)
            out[~self.free] = NH_UNKNOWN
            out[goal] = NH_STAY
            out.setflags(write=False)
            self._k1[goal] = out
        return self._k1[goal]

    def _code(self, og, c: int, goal: int) -> int:
        nx = og.get_path_next(c, goal)[0]
        W = self.W
        return 4 if nx == c else 0 if nx == c + W else 1 if nx == c + 1 else 2 if nx + W == c else 3

    def astar_codes(self, pairs) -> np.ndarray:
        """get_path's code for every (cell, goal) of `pairs`, memoised; new pairs go to the C oracle over at
        most 16 threads with one OracleGraph each (the library call releases the GIL)."""
        todo = []
        for c, goal in pairs:
            memo = self._memo.get(goal)
            if memo is None:
                memo = self._memo[goal] = np.full(self.free.size, _NONE, dtype=np.uint8)
            if memo[c] == _NONE:
                todo.append((c, goal))
        if todo:
            t0 = time.perf_counter()
            nthr = max(1, min(16, os.cpu_count() or 1, len(todo) // 256))
            if nthr == 1:
                res = [self._code(self.og, c, goal) for c, goal in todo]
            else:
                if self._pool is None:
                    self._pool = (ThreadPoolExecutor(16), [self._OG(self.cells) for _ in range(16)])
                ex, ogs = self._pool
                parts = [todo[k::nthr] for k in range(nthr)]
                outs = list(ex.map(lambda a: [self._code(a[0], c, goal) for c, goal in a[1]], zip(ogs, parts)))
                res = [0] * len(todo)
                for k, o in enumerate(outs):
                    res[k::nthr] = o
            for (c, goal), r in zip(todo, res):
                self._memo[goal][c] = r
            self.oracle_s += time.perf_counter() - t0
            self.oracle_calls += len(todo)
        return np.array([self._memo[goal][c] for c, goal in pairs], dtype=np.uint8)

    def next_codes(self, goal: int) -> np.ndarray:
        """Every cell's code (orc_next_codes' table) from k1() and astar_codes()."""
        out = self.k1(goal).copy()
        need = np.flatnonzero(out == ASTAR)
        out[need] = self.astar_codes([(int(c), goal) for c in need])
        return out
