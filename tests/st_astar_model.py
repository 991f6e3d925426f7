"""CPU model of tsw_astar_reserved (include/tswap.h): astar_with_reservation (src/algorithm/a_star.rs:32-112)
restated with dict and set state like the reference, the open set a RustBinaryHeap (oracle/py_restatement.py)
of nodes that carry TimeNode's order. Plus an independent formulation (a plain BFS over the time-expanded
graph with the same successor filter) and the case list the CPU and GPU tests share. Test infrastructure only.
"""
import random

import numpy as np

from py_restatement import RustBinaryHeap

FOUND, NONE, CAPACITY = 0, 1, 2
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (0, 0))  # a_star.rs:40, the last one WAIT


class TimeNode:
    """a_star.rs:15-19: cmp = other.f.cmp(&self.f).then(other.g.cmp(&self.g)); pos takes no part."""
    __slots__ = ("pos", "g", "f")

    def __init__(self, pos, g, f):
        self.pos, self.g, self.f = pos, g, f

    def le(self, other):  # self <= other in Rust's order: reversed on (f, g)
        return (other.f, other.g) <= (self.f, self.g)


def _h(a, b):
    return abs(a[0] - b[0]) + abs(a[1] - b[1])


def successors(rows, pos, g, node_res, edge_res):
    """The successor filter of the issue's section 1 without the visited test: [(np, nt)] in push order."""
    h, w = len(rows), len(rows[0])
    nt = g + 1
    out = []
    for dx, dy in DIRS:
        nx, ny = pos[0] + dx, pos[1] + dy
        if nx < 0 or ny < 0 or nx >= w or ny >= h or rows[ny][nx] == "@":
            continue
        np_ = (nx, ny)
        if (np_, nt) in node_res or (pos, nt) in node_res:
            continue
        if ((pos, np_), nt) in edge_res or ((np_, pos), nt) in edge_res:
            continue
        out.append((np_, nt))
    return out


def astar_reserved(rows, start, goal, start_time, node_res, edge_res, max_time, max_nodes=65536):
    """Returns (path [(x, y)], status, pops, pushes); astar_reserved.peak is the last call's largest heap. node_res: {((x, y), t)}; edge_res: {(((x, y), (x, y)), t)}."""
    open_ = RustBinaryHeap()
    came_from = {}
    pushed = {(start, start_time)}
    open_.push(TimeNode(start, start_time, start_time + _h(start, goal)))
    pops, pushes = 0, 1
    astar_reserved.peak = 1
    while True:
        n = open_.pop()
        if n is None:
            return [], NONE, pops, pushes
        if n.f > max_time:  # the horizon: at a pop, never at a push
            return [], NONE, pops, pushes
        pops += 1
        if n.pos == goal:
            path, cur = [], (n.pos, n.g)
            while cur in came_from:
                path.append(cur[0])
                cur = came_from[cur]
            path.append(start)
            path.reverse()
            return path, FOUND, pops, pushes
        for key in successors(rows, n.pos, n.g, node_res, edge_res):
            if key in pushed:
                continue
            if pushes == max_nodes:  # the capacity: the push that would be the (max_nodes + 1)-th
                return [], CAPACITY, pops, pushes
            came_from[key] = (n.pos, n.g)
            pushed.add(key)
            open_.push(TimeNode(key[0], key[1], key[1] + _h(key[0], goal)))
            pushes += 1
            astar_reserved.peak = max(astar_reserved.peak, len(open_.data))


def earliest_arrival(rows, start, goal, start_time, node_res, edge_res, max_time):
    """Independent formulation: layer-by-layer BFS over (cell, time), same filter; the first t <= max_time at
    which the goal is reached, or None."""
    layer = {start}
    t = start_time
    while layer and t <= max_time:
        if goal in layer:
            return t
        layer = {np_ for pos in layer for np_, _ in successors(rows, pos, t, node_res, edge_res)}
        t += 1
    return None


# ---- the case list ---------------------------------------------------------------------------------------
class Case:
    """One call: a grid, k queries, the reservations, the caps — and what the model says of it."""

    def __init__(self, name, rows, queries, node_res=(), edge_res=(), max_time=48, max_nodes=65536):
        self.name, self.rows = name, rows
        self.w, self.h = len(rows[0]), len(rows)
        self.queries = list(queries)  # (start (x, y), goal (x, y), start_time)
        self.node_res, self.edge_res = list(node_res), list(edge_res)  # lists: repeats are legal
        self.max_time, self.max_nodes = max_time, max_nodes
        self._exp = None

    def cell(self, p):
        return p[1] * self.w + p[0]

    def arrays(self):
        """start, goal, start_time (u32[k]); node_res (n, 2) u32 cell, t; edge_res (n, 3) u32 from, to, t. Points
        off the grid keep an id >= w * h."""
        def cid(p):
            return self.cell(p) if 0 <= p[0] < self.w and 0 <= p[1] < self.h else self.w * self.h + 7
        st = np.array([self.cell(q[0]) for q in self.queries], dtype=np.uint32)
        gl = np.array([self.cell(q[1]) for q in self.queries], dtype=np.uint32)
        t0 = np.array([q[2] for q in self.queries], dtype=np.uint32)
        nr = np.array([(cid(p), t) for p, t in self.node_res], dtype=np.uint32).reshape(-1, 2)
        er = np.array([(cid(a), cid(b), t) for (a, b), t in self.edge_res], dtype=np.uint32).reshape(-1, 3)
        return st, gl, t0, nr, er

    def expected(self):
        """(path_off u32[k+1], path u32[total], status u32[k], pops u32[k], pushes [k], heap peaks [k]) from the
        model; computed once and shared."""
        if self._exp is None:
            ns, es = set(self.node_res), set(self.edge_res)
            off, path, status, pops, pushes, peaks = [0], [], [], [], [], []
            for s, g, t0 in self.queries:
                p, stt, po, pu = astar_reserved(self.rows, s, g, t0, ns, es, self.max_time, self.max_nodes)
                path += [self.cell(c) for c in p]
                off.append(len(path))
                status.append(stt)
                pops.append(po)
                pushes.append(pu)
                peaks.append(astar_reserved.peak)
            self._exp = (np.array(off, dtype=np.uint32), np.array(path, dtype=np.uint32),
                         np.array(status, dtype=np.uint32), np.array(pops, dtype=np.uint32), pushes, peaks)
        return self._exp


def open8x8():
    rows = ["." * 8] * 8
    cells = [(x, y) for y in range(8) for x in range(8)]
    return Case("open8x8", rows, [(s, g, 0) for s in cells for g in cells if s != g], max_time=40)


RANDOM_SEED = 7


def random12(i):
    """Grid i of the random recipe: 12x12, 20 % obstacles, 50 queries, start_time in {0, 3}, max_time 48, vertex
    reservations on 10 % of (free cell, t in 1..24), 200 edge reservations (WAIT edges and non-adjacent pairs
    among them)."""
    rng = random.Random(RANDOM_SEED * 1000 + i)
    rows = ["".join("@" if rng.random() < 0.2 else "." for _ in range(12)) for _ in range(12)]
    free = [(x, y) for y in range(12) for x in range(12) if rows[y][x] == "."]
    node_res = [(c, t) for c in free for t in range(1, 25) if rng.random() < 0.1]
    edge_res = []
    for _ in range(200):
        a = rng.choice(free)
        kind = rng.random()
        if kind < 0.15:
            b = a  # a WAIT edge
        elif kind < 0.3:
            b = rng.choice(free)  # any pair: mostly not adjacent
        else:
            dx, dy = rng.choice(DIRS[:4])
            b = (a[0] + dx, a[1] + dy)  # may be blocked or off the grid
        edge_res.append(((a, b), rng.randint(1, 24)))
    queries = []
    for _ in range(50):
        s = rng.choice(free)
        g = rng.choice(free)
        queries.append((s, g, rng.choice((0, 3))))
    return Case(f"random12-{i}", rows, queries, node_res, edge_res, max_time=48)


def hand_cases():
    line = ["." * 6]
    walled = ["...", "@@@", "..."]
    return [
        # the goal (3, 0) is reserved until t = 5: arrival at 6
        Case("goal-reserved-until-5", line, [((0, 0), (3, 0), 0)], node_res=[((3, 0), t) for t in range(1, 6)], max_time=20),
        # the edge (1,0)-(2,0) is taken head-on at t = 2: wait or step back
        Case("head-on-edge", line, [((0, 0), (4, 0), 0)], edge_res=[(((2, 0), (1, 0)), 2)], max_time=20),
        Case("head-on-edge-3x3", ["...", ".@.", "..."], [((0, 0), (2, 0), 0)], edge_res=[(((2, 0), (1, 0)), 2), (((1, 0), (0, 0)), 1)],
             max_time=20),
        # the current cell (1, 0) is reserved at t = 2: a node popped there at g = 1 may not leave it
        Case("reserved-current-cell", line, [((0, 0), (3, 0), 0)], node_res=[((1, 0), 2)], max_time=20),
        # waiting at (1, 0) is forbidden at t = 1 while the way forward is reserved at t = 1: one step back
        Case("no-wait-edge", line, [((1, 0), (3, 0), 0)], node_res=[((2, 0), 1)], edge_res=[(((1, 0), (1, 0)), 1)], max_time=20),
        # every successor of the start at start_time + 1 is reserved: one pop, then the heap is empty
        Case("boxed-in", ["...", "...", "..."], [((1, 1), (2, 2), 4)],
             node_res=[((1, 1), 5), ((0, 1), 5), ((2, 1), 5), ((1, 0), 5), ((1, 2), 5)], max_time=30),
        Case("walled-off", walled, [((0, 0), (0, 2), 0)], max_time=12),
        Case("walled-off-capacity", walled, [((0, 0), (0, 2), 0)], max_time=12, max_nodes=8),
        Case("start-is-goal", line, [((2, 0), (2, 0), 5)], max_time=20),
        # beyond the horizon before the first pop: 0 pops
        Case("too-far", line, [((0, 0), (5, 0), 17)], max_time=20),
        # reservations that can never match: off the grid, far apart, past the horizon, repeated
        Case("inert-reservations", line, [((0, 0), (5, 0), 0)],
             node_res=[((9, 9), 1), ((1, 0), 900), ((1, 0), 900), ((1, 0), 0)],
             edge_res=[(((0, 0), (4, 0)), 1), (((0, 0), (9, 0)), 1), (((0, 0), (1, 0)), 0), (((5, 0), (0, 0)), 1)], max_time=20),
    ]


def packed_field_cases():
    wide = ["." * 2048, "." * 2048]
    return [
        Case("x-to-2047", wide, [((2047 - 40, 0), (2047, 1), 0), ((2047, 0), (2047 - 30, 1), 2)],
             node_res=[((2047 - 20, 0), 20), ((2047, 0), 41)], max_time=120),
        Case("late-start", ["." * 6] * 2, [((0, 0), (5, 1), (1 << 20) - 8), ((0, 0), (5, 0), (1 << 20) - 8),
                                         ((0, 0), (5, 0), (1 << 20) - 4)],
             node_res=[((1, 0), (1 << 20) - 7)], max_time=1 << 20),
    ]


def big_heap_case():
    """An open 40x40 grid whose goal vertex is reserved for 39 steps: the frontier piles up around it and the heap
    passes the 512 entries a search wave keeps in LDS (the kernel's move to its global heap)."""
    g = (20, 20)
    return Case("big-heap-40", ["." * 40] * 40, [((0, 0), g, 0), ((39, 3), g, 0), ((5, 30), g, 2)],
                node_res=[(g, t) for t in range(1, 40)], max_time=160)


def repeated(c, times):
    """c's queries `times` times over, with the model's results repeated likewise."""
    r = Case(f"{c.name}-x{times}", c.rows, c.queries * times, c.node_res, c.edge_res, c.max_time, c.max_nodes)
    off, path, status, pops, pushes, peaks = c.expected()
    lens = np.tile(np.diff(off.astype(np.int64)), times)
    r._exp = (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32), np.tile(path, times), np.tile(status, times),
              np.tile(pops, times), pushes * times, peaks * times)
    return r


_CACHE = {}


def all_cases():
    """Every case but the open 8x8 grid (its own test), built once."""
    if "all" not in _CACHE:
        _CACHE["all"] = [random12(i) for i in range(6)] + hand_cases() + packed_field_cases() + [big_heap_case()]
    return _CACHE["all"]


def open_case():
    if "open" not in _CACHE:
        _CACHE["open"] = open8x8()
    return _CACHE["open"]


def by_name(name):
    return next(c for c in all_cases() + [open_case()] if c.name == name)
