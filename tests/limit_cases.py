"""Maps and instances at the limits of the kernels' packed fields, shared by tests/test_limit_cases.py (CPU: the
properties, from the oracle alone) and tests/test_gpu_limits.py (GPU). No test in here.

The limits (csrc/tsw_internal.h, tsw_astar.h): x and y take 11 bits (MAX_WH = 2048), a K1 table holds u16
distances with 0xFFFF for "unreachable" (so 0xFFFE = 65,534 is the largest distance a table can hold), the wave
A* cores keep g in 15 bits and hand a query over to k_astar's 20-bit g once g reaches 2^15, and k_astar_lds
(grids of 1024 cells or fewer) packs f:11 | g:10 | cell:11.
"""
from __future__ import annotations

import functools

import numpy as np

from p2p_distributed_tswap_amd import maps

INF = 0xFFFF
G15 = 1 << 15          # first g the 15-bit field cannot hold
HALF = 1024            # first coordinate that needs the 11th bit
SEED = 0x2048
DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0))  # S, E, N, W


# ---- recipes --------------------------------------------------------------------------------------------------

def _snake_array(W: int, H: int, keep=None):
    """(blocked (H, W), order): even rows are open corridors, every odd row is a wall with one gap, at x = W - 1
    for the first wall, x = 0 for the second and so on; order = the free cells along the path from (0, 0). With
    `keep`, every cell of order[keep:] is blocked (the last corridor ends early)."""
    assert H % 2 == 1
    a = np.zeros((H, W), dtype=bool)
    order = []
    for y in range(0, H, 2):
        east = (y // 2) % 2 == 0
        order += [y * W + x for x in (range(W) if east else range(W - 1, -1, -1))]
        if y + 1 < H:
            gx = W - 1 if east else 0
            a[y + 1, :] = True
            a[y + 1, gx] = False
            order.append((y + 1) * W + gx)
    order = np.array(order, dtype=np.uint32)
    if keep is not None:
        a.reshape(-1)[order[keep:]] = True
        order = order[:keep]
    return a, order


def _finish(a: np.ndarray, order: np.ndarray, transpose: bool):
    H, W = a.shape
    if transpose:  # (x, y) -> (y, x): the new width is H
        a = np.ascontiguousarray(a.T)
        order = ((order % W) * H + order // W).astype(np.uint32)
    order.setflags(write=False)
    return maps.to_rows(a), order


def snake(W: int, H: int, keep=None, transpose: bool = False):
    """(rows, order) of _snake_array; transpose=True: the same map with x and y exchanged, order mapped with it."""
    return _finish(*_snake_array(W, H, keep), transpose)


ROOM_Y0, ROOM_H = 32, 16


def snake_room(transpose: bool = False):
    """(rows, order), 2048 x 48: rows 0..30 are snake(2048, 31) (16 corridors, 32,783 cells, ending at x = 0,
    y = 30), row 31 a wall with one gap below the snake's end (the door), rows 32..47 a room with
    Bernoulli(0.2) obstacles whose five cells under the door are cleared. order is the snake's."""
    W = 2048
    s, order = _snake_array(W, 31)
    a = np.zeros((ROOM_Y0 + ROOM_H, W), dtype=bool)
    a[:31] = s
    ex = int(order[-1]) % W
    a[31, :] = True
    a[31, ex] = False
    a[ROOM_Y0:] = np.random.default_rng(SEED).random((ROOM_H, W)) < 0.2
    a[ROOM_Y0:ROOM_Y0 + 5, ex] = False
    return _finish(a, order, transpose)


def random_map(w: int, h: int, p: float, seed: int) -> list:
    """maps.random_map, with the splitmix64 stream evaluated in numpy (the 2^20-cell maps take seconds in the
    per-cell loop): draw i is mix(seed + (i + 1) * gamma). test_limit_cases.py checks it against maps.random_map."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & maps.MASK64) + np.arange(1, w * h + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    return maps.to_rows((u < p).reshape(h, w))


def line(n: int, vertical: bool, walled: bool) -> list:
    """n x 1 (or 1 x n) open line; walled: cell n - 2 blocked (cell n - 1 is cut off from the rest)."""
    a = np.zeros(n, dtype=bool)
    a[n - 2] = walled
    return maps.to_rows(a.reshape(n, 1) if vertical else a.reshape(1, n))


STRIPS = {"strip2048x16": (2048, 16), "strip16x2048": (16, 2048), "strip2047x17": (2047, 17),
          "strip17x2047": (17, 2047)}
FULL = {"full2048x512": (2048, 512), "full512x2048": (512, 2048)}
SNAKES = {"wide": (33, None, False), "tall": (33, None, True), "exact": (63, 65535, False),
          "over": (63, 65536, False)}
LINES = {"line1024x1": (False, False), "line1x1024": (True, False), "wline1024x1": (False, True),
         "wline1x1024": (True, True)}


class Case:
    """One map: rows, cells (H, W) u8, free (flat bool), order (the snakes' path, else None), and the oracle,
    made on first use and shared (read-only results)."""

    def __init__(self, name, rows, order=None):
        self.name, self.rows, self.order = name, rows, order
        self.cells = maps.rows_to_array(rows)
        self.H, self.W = self.cells.shape
        self.free = self.cells.reshape(-1) != ord("@")
        self.free_ids = np.flatnonzero(self.free).astype(np.uint32)
        self.vertical = self.H > self.W
        self._og = None
        self._bfs = {}

    @property
    def og(self):
        if self._og is None:
            from oracle import OracleGraph

            self._og = OracleGraph(self.cells)
        return self._og

    def bfs(self, goal: int) -> np.ndarray:
        goal = int(goal)
        if goal not in self._bfs:
            t = self.og.bfs(goal)
            t.setflags(write=False)
            self._bfs[goal] = t
        return self._bfs[goal]

    def long_coord(self, ids) -> np.ndarray:
        """The coordinate along the long side (the one that reaches 2047)."""
        ids = np.asarray(ids, dtype=np.int64)
        return ids // self.W if self.vertical else ids % self.W

    def code(self, c: int, goal: int) -> int:
        """get_path's next hop from c toward goal as a code: 0..3 = S, E, N, W, 4 = stay."""
        nx = self.og.get_path_next(int(c), int(goal))[0]
        W = self.W
        return 4 if nx == c else 0 if nx == c + W else 1 if nx == c + 1 else 2 if nx + W == c else 3


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name in SNAKES:
        H, keep, tr = SNAKES[name]
        return Case(name, *snake(2048, H, keep, tr))
    if name in ("snake_room", "snake_room_t"):
        return Case(name, *snake_room(name.endswith("_t")))
    if name in STRIPS:
        return Case(name, random_map(*STRIPS[name], 0.2, SEED))
    if name in FULL:
        return Case(name, random_map(*FULL[name], 0.1, SEED))
    if name in LINES:
        return Case(name, line(1024, *LINES[name]))
    raise KeyError(name)


# ---- K1 goals -------------------------------------------------------------------------------------------------

def snake_goals(c: Case) -> np.ndarray:
    """wide / tall: both ends, the middle, and 5 seeded cells of the path."""
    o = c.order
    rng = np.random.default_rng(5)
    return np.concatenate([[o[0], o[-1], o[o.size // 2]], rng.choice(o, 5, replace=False)]).astype(np.uint32)


def strip_goals(c: Case, n: int = 40) -> np.ndarray:
    """n seeded distinct free cells, half of them with the long coordinate >= 1024."""
    rng = np.random.default_rng(40)
    hi = c.long_coord(c.free_ids) >= HALF
    return np.concatenate([rng.choice(c.free_ids[hi], n // 2, replace=False),
                           rng.choice(c.free_ids[~hi], n - n // 2, replace=False)]).astype(np.uint32)


def full_goals(c: Case) -> np.ndarray:
    """The first and the last free cell and 2 seeded ones."""
    rng = np.random.default_rng(4)
    return np.concatenate([[c.free_ids[0], c.free_ids[-1]], rng.choice(c.free_ids[1:-1], 2, replace=False)]).astype(np.uint32)


# ---- K3 queries -----------------------------------------------------------------------------------------------

def room_cells(c: Case) -> np.ndarray:
    """The room cells of snake_room / snake_room_t that the snake reaches, ascending."""
    far = (c.free_ids // c.W if not c.vertical else c.free_ids % c.W) >= ROOM_Y0
    ids = c.free_ids[far]
    return ids[c.bfs(c.order[0])[ids] != INF]


def room_queries(c: Case, n: int = 64, seed: int = 7):
    """n seeded (start, goal): start = order[k], k uniform in [0, 1200), goal a reachable room cell. The path runs
    down the whole snake (32,783 - k cells) and then through the room, so its length straddles 32,769."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1200, n)
    room = room_cells(c)
    return c.order[k].astype(np.uint32), room[rng.integers(0, room.size, n)].astype(np.uint32)


def boundary_pairs(c: Case):
    """(start, goal, len): along the snake, path lengths 32,768 (g = 32,767 at the goal: the last that 15 bits
    hold) and 32,769 (g = 32,768), in both directions."""
    o = c.order
    s = np.array([o[0], o[0], o[G15 - 1], o[G15]], dtype=np.uint32)
    g = np.array([o[G15 - 1], o[G15], o[0], o[0]], dtype=np.uint32)
    return s, g, np.array([G15, G15 + 1, G15, G15 + 1], dtype=np.int32)


def strip_pairs(c: Case, n: int = 300, seed: int = 300):
    """n seeded (start, goal) of free cells: the start's long coordinate is >= 1024, the goal lies within Manhattan
    150 of it. The goal is any free cell, and the goals of the last 8 pairs are drawn from outside the largest
    component: pairs across components take get_path's fallback (coordinate comparisons)."""
    rng = np.random.default_rng(seed)
    ids = c.free_ids.astype(np.int64)
    x, y = ids % c.W, ids // c.W
    s = rng.choice(ids[c.long_coord(ids) >= HALF], n)
    comp = np.array([b * c.W + a for (a, b) in maps.largest_component(c.rows)], dtype=np.int64)
    pocket = ~np.isin(ids, comp)
    g = np.empty(n, dtype=np.int64)
    for i, a in enumerate(s):
        near = (np.abs(x - a % c.W) + np.abs(y - a // c.W) <= 150) & (ids != a)
        if i >= n - 8 and (near & pocket).any():
            near &= pocket
        pick = ids[near]
        g[i] = pick[rng.integers(0, pick.size)]
    return s.astype(np.uint32), g.astype(np.uint32)


def full_pairs(c: Case, n: int = 32, seed: int = 32):
    """n seeded pairs of free cells, both within Manhattan 150 of the last free cell."""
    rng = np.random.default_rng(seed)
    ids = c.free_ids.astype(np.int64)
    last = int(ids[-1])
    near = ids[np.abs(ids % c.W - last % c.W) + np.abs(ids // c.W - last // c.W) <= 150]
    return rng.choice(near, n).astype(np.uint32), rng.choice(near, n).astype(np.uint32)


def high_cells(c: Case, n: int = 400, seed: int = 400) -> np.ndarray:
    """n seeded distinct free cells with the long coordinate >= 1024."""
    hi = c.free_ids[c.long_coord(c.free_ids) >= HALF]
    return np.random.default_rng(seed).choice(hi, n, replace=False).astype(np.uint32)


def eager_goals(c: Case) -> np.ndarray:
    """2 seeded goals of the strip's largest component with the long coordinate >= 1024."""
    comp = np.array([y * c.W + x for (x, y) in maps.largest_component(c.rows)], dtype=np.uint32)
    hi = comp[c.long_coord(comp) >= HALF]
    return np.random.default_rng(2).choice(hi, 2, replace=False).astype(np.uint32)


LINE_CELLS = (0, 1, 511, 512, 1022, 1023)


def line_pairs():
    """Open line: every ordered pair of LINE_CELLS (start == goal included); lengths reach 1024 (g = 1023)."""
    s, g = np.meshgrid(np.array(LINE_CELLS, dtype=np.uint32), np.array(LINE_CELLS, dtype=np.uint32), indexing="ij")
    return s.reshape(-1).copy(), g.reshape(-1).copy()


def walled_line_pairs():
    """Walled line (cell 1022 blocked): 1021 -> 1023 cannot arrive, the search runs to cell 0 (f up to
    1021 + 1023 = 2044) and no neighbour is closer: stay; 0 -> 1023: the fallback steps toward it."""
    return np.array([1021, 0], dtype=np.uint32), np.array([1023, 1023], dtype=np.uint32)


# ---- planning instances ---------------------------------------------------------------------------------------

def multi_candidate(c: Case, cell: int, goal: int) -> bool:
    """At least two free neighbours of `cell` are one step closer to `goal` (K1 leaves the code to the A*)."""
    D = c.bfs(goal)
    d, n = int(D[cell]), 0
    if d == INF or d == 0:
        return False
    x, y = cell % c.W, cell // c.W
    for dx, dy in DIRS:
        nx, ny = x + dx, y + dy
        if 0 <= nx < c.W and 0 <= ny < c.H and int(D[ny * c.W + nx]) == d - 1:
            n += 1
    return n >= 2


def room_plan_instance(seed: int = 11):
    """(starts (12, 2), tasks (24, 4), max_t) on snake_room: 12 agents on room cells 300..1200 steps from the door,
    24 tasks from pickups order[0..23] (the far end of the snake: every agent's distance to its pickup is 32,783
    or more) to deliveries in the room."""
    c = case("snake_room")
    W = c.W
    door = int(c.order[-1]) + W
    room = room_cells(c)
    d = c.bfs(door)[room]
    rng = np.random.default_rng(seed)
    st = rng.choice(room[(d >= 300) & (d <= 1200)], 12, replace=False)
    dl = rng.choice(room, 24, replace=False)
    starts = np.stack([st % W, st // W], axis=1).astype(np.uint32)
    pk = c.order[:24].astype(np.int64)
    tasks = np.stack([pk % W, pk // W, dl % W, dl // W], axis=1).astype(np.uint32)
    return starts, tasks, 8


def strip_window(c: Case):
    """(x0, y0, w, h): the part of the strip with the long coordinate >= 1100."""
    return (0, 1100, c.W, c.H - 1100) if c.vertical else (1100, 0, c.W - 1100, c.H)


def strip_plan_instance(c: Case):
    """(starts, tasks, max_t): 48 agents and 96 tasks drawn from strip_window."""
    starts, tasks = maps.make_window_instance(c.rows, 48, 96, 0x77, *strip_window(c))
    return starts, tasks, 80


def strip_step_instance(c: Case, seed: int = 5):
    """(v, g): the plan instance's starts with seeded goals from the same window's part of the largest component."""
    x0, y0, w, h = strip_window(c)
    starts, _, _ = strip_plan_instance(c)
    pool = np.array([y * c.W + x for (x, y) in maps.largest_component(c.rows)
                     if x0 <= x < x0 + w and y0 <= y < y0 + h], dtype=np.uint32)
    v = (starts[:, 1] * c.W + starts[:, 0]).astype(np.uint32)
    return v, np.random.default_rng(seed).choice(pool, v.size).astype(np.uint32)


def rec_xy(rec: np.ndarray):
    rec = np.asarray(rec, dtype=np.uint64)
    return (rec & np.uint64(0xFFFF)).astype(np.int64), ((rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)


def high_fleet(c: Case):
    """(v, g) of fleet_cases.recipe_fleet(rows, 90, 3, 6) on the half of the strip with the long coordinate
    >= 1024: the recipe runs on that half as a map of its own, and its cells are moved back."""
    import fleet_cases as fc

    if c.vertical:
        v, g, rings = fc.recipe_fleet(c.rows[HALF:], 90, 3, 6)
        shift = np.uint32(HALF * c.W)
        return v + shift, g + shift, rings
    sub = [r[HALF:] for r in c.rows]
    v, g, rings = fc.recipe_fleet(sub, 90, 3, 6)
    w2 = c.W - HALF

    def back(a):
        a = a.astype(np.int64)
        return ((a // w2) * c.W + a % w2 + HALF).astype(np.uint32)

    return back(v), back(g), rings
