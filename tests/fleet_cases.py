"""Shared inputs of the fleet tests (test_fleet_host.py on the CPU, test_gpu_fleet.py on the GPU): the
fleet recipe, the nearby shapes, the brute-force nearby lists and a numpy restatement of the binned
construction of tsw_nearby.hip. No test in here."""
import functools
import random

import numpy as np

from p2p_distributed_tswap_amd import maps


def recipe_fleet(rows, n0, seed, rings):
    """(v, g) cell ids of a fleet that exercises every rule of compute_next_move_with_tswap:
    n0 agents on distinct cells of the largest component (15 % at their goal, 40 % heading for another
    agent's cell, the rest anywhere), n0 // 10 more co-located with an earlier agent (stale information),
    and `rings` 2 x k loops (k in 2..3) of so far unused free cells with one agent per loop cell heading
    for the next one plus one more agent on the loop's first cell — the co-located entry that lets the
    reference's position-keyed check (agent.rs:403-411) close a rotation."""
    H, W = len(rows), len(rows[0])
    comp = maps.largest_component(rows)
    rng = random.Random(seed)
    pts = rng.sample(comp, n0)
    goals = [rng.choice(comp) for _ in range(n0)]
    for i in range(n0):
        r = rng.random()
        if r < 0.15:
            goals[i] = pts[i]
        elif r < 0.55:
            goals[i] = pts[rng.randrange(n0)]
    for _ in range(n0 // 10):
        pts.append(pts[rng.randrange(len(pts))])
        goals.append(rng.choice(comp))
    used = set(pts)
    placed = 0
    for _ in range(400 * rings):
        if placed >= rings:
            break
        k = rng.randrange(2, 4)
        x0, y0 = rng.randrange(0, W - k + 1), rng.randrange(0, H - 1)
        loop = [(x0 + i, y0) for i in range(k)] + [(x0 + i, y0 + 1) for i in reversed(range(k))]
        if any(rows[y][x] == "@" or (x, y) in used for x, y in loop):
            continue
        for i, c in enumerate(loop):
            pts.append(c)
            goals.append(loop[(i + 1) % len(loop)])
        pts.append(loop[0])
        goals.append(loop[rng.randrange(len(loop))])
        used.update(loop)
        placed += 1
    v = np.array([y * W + x for x, y in pts], dtype=np.uint32)
    g = np.array([y * W + x for x, y in goals], dtype=np.uint32)
    return v, g, placed


@functools.lru_cache(maxsize=None)
def fleet_case(name):
    """(rows, v, g) of the named recipe fleets of the issue's table."""
    rows, n0, seed, rings = {
        "rand20": (maps.random_map(20, 16, 0.2, 5), 90, 3, 6),
        "dense12": (maps.random_map(12, 12, 0.15, 9), 60, 1, 4),
        "warehouse": (maps.warehouse_map(170, 84, 0x170084), 400, 5, 8),
    }[name]
    v, g, _ = recipe_fleet(rows, n0, seed, rings)
    return rows, v, g


def _cells(W, pts):
    return np.array([y * W + x for x, y in pts], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def nearby_shape(name):
    """(W, H, rows, v) of the nearby-list shapes; rows is the map to plan on."""
    if name == "open6":  # 12 agents plus 6 duplicates of their positions
        rng = random.Random(6)
        pts = rng.sample([(x, y) for y in range(6) for x in range(6)], 12)
        pts += [pts[rng.randrange(12)] for _ in range(6)]
        return 6, 6, maps.open_map(6, 6), _cells(6, pts)
    if name == "edges13x7":  # every border cell (the four corners among them) and a few inner cells
        W, H = 13, 7
        pts = [(x, y) for y in range(H) for x in range(W) if x in (0, W - 1) or y in (0, H - 1)]
        pts += [(6, 3), (1, 1), (11, 5), (6, 3)]
        random.Random(13).shuffle(pts)
        return W, H, maps.open_map(W, H), _cells(W, pts)
    if name in ("rand20", "warehouse"):
        rows, v, _ = fleet_case(name)
        return len(rows[0]), len(rows), rows, v
    if name == "open40":  # 1,100 agents on distinct cells: at r = 80 every list has 1,099 entries
        rng = random.Random(40)
        pts = rng.sample([(x, y) for y in range(40) for x in range(40)], 1100)
        return 40, 40, maps.open_map(40, 40), _cells(40, pts)
    if name == "one":
        return 6, 6, maps.open_map(6, 6), np.array([17], dtype=np.uint32)
    if name == "none":
        return 6, 6, maps.open_map(6, 6), np.zeros(0, dtype=np.uint32)
    raise KeyError(name)


# (shape, radius) of every nearby comparison
NEARBY_CASES = [("open6", 0), ("open6", 1), ("open6", 2), ("edges13x7", 1), ("edges13x7", 5), ("edges13x7", 40),
                ("rand20", 3), ("rand20", 15), ("warehouse", 15), ("open40", 80), ("one", 15), ("none", 15)]


@functools.lru_cache(maxsize=None)
def _brute_cached(name, r):
    W, _, _, v = nearby_shape(name)
    return brute_nearby(v, W, r)


def brute_case(name, r):
    """Brute-force (nb_off, nb_idx) of a named shape, computed once and shared (do not modify)."""
    return _brute_cached(name, r)


def brute_nearby(v, W, r):
    """The definition: agent i's list is every j != i with |dx| + |dy| <= r, ascending j (CSR)."""
    v = np.asarray(v, dtype=np.int64)
    n = v.size
    x, y = v % W, v // W
    m = (np.abs(x[:, None] - x[None, :]) + np.abs(y[:, None] - y[None, :])) <= r
    m[np.arange(n), np.arange(n)] = False
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(m.sum(axis=1))
    return off, np.nonzero(m)[1].astype(np.uint32)


def binned_nearby(v, W, H, r):
    """numpy restatement of tsw_nearby.hip: per-cell histogram, exclusive prefix (cell_start), agent
    indices in cell order (the order inside a cell is arbitrary on the device: reversed here), then per
    agent the diamond's rows y-r..y+r clipped to the grid, each row the contiguous cells x +- (r - |dy|)
    clipped to [0, W), i.e. the entries cell_start[lo] .. cell_start[hi + 1] of the cell-sorted array;
    self dropped by index, the list sorted ascending."""
    v = np.asarray(v, dtype=np.int64)
    n = v.size
    r = min(int(r), W + H)
    cell_start = np.zeros(W * H + 1, dtype=np.int64)
    cell_start[1:] = np.cumsum(np.bincount(v, minlength=W * H))
    order = np.lexsort((-np.arange(n), v))
    lists = []
    for i in range(n):
        x, y = int(v[i] % W), int(v[i] // W)
        got = []
        for yy in range(max(0, y - r), min(H - 1, y + r) + 1):
            half = r - abs(yy - y)
            lo, hi = yy * W + max(0, x - half), yy * W + min(W - 1, x + half)
            got.append(order[cell_start[lo]:cell_start[hi + 1]])
        e = np.concatenate(got)
        lists.append(np.sort(e[e != i]))
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(e) for e in lists])
    idx = np.concatenate(lists).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    return off, idx


def oracle_fleet(og, v, g, off, idx):
    """The reference result of tsw_decide_fleet: OracleGraph.decide per agent on its brute-force list,
    partner and participants mapped through the list to agent indices."""
    n = len(v)
    act, cell, partner = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    part_off = np.zeros(n + 1, dtype=np.uint32)
    part = []
    for i in range(n):
        li = idx[off[i]:off[i + 1]]
        a, c, p, ps = og.decide(int(v[i]), int(g[i]), v[li], g[li])
        act[i], cell[i] = a, c
        partner[i] = 0xFFFFFFFF if p == 0xFFFFFFFF else li[p]
        part += [int(li[k]) for k in ps]
        part_off[i + 1] = len(part)
    return act, cell, partner, part_off, np.array(part, dtype=np.uint32)
