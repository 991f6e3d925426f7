"""Shared inputs of the fleet tests (test_fleet_host.py on the CPU, test_gpu_fleet.py on the GPU): the
fleet recipe, the nearby shapes, the brute-force nearby lists and a numpy restatement of the binned
construction of tsw_nearby.hip; the fleets that sit on the kernels' internal boundaries (chunks of 64
diamond rows, scan tiles of 2,048, lists of 1,024 entries) and the r = 0 grouping reference for fleets too
large for the n x n matrix. No test in here."""
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
        "tall9x200": (maps.open_map(9, 200), 140, 9, 6),  # diamonds taller than a wave's 64 rows
    }[name]
    v, g, _ = recipe_fleet(rows, n0, seed, rings)
    return rows, v, g


@functools.lru_cache(maxsize=None)
def cap_fleet(n):
    """(rows, v, g) of n >= 1,007 agents on open_map(40, 40), for r = 80 (everyone sees everyone: every
    list has n - 1 entries). A recipe fleet with 12 rings, then co-located agents inserted at the FRONT one
    by one until there are n, so that the rings keep the top agent indices; cap_fleet(n + 1) is
    cap_fleet(n) with one more agent in front."""
    rows = maps.open_map(40, 40)
    v, g, placed = recipe_fleet(rows, 850, 25, 12)
    assert placed == 12 and v.size <= n
    rng = random.Random(1025)
    front_v, front_g = [], []
    for _ in range(n - v.size):
        front_v.append(int(v[rng.randrange(v.size)]))
        front_g.append(rng.randrange(1600))
    v = np.concatenate([np.array(front_v[::-1], dtype=np.uint32), v])
    g = np.concatenate([np.array(front_g[::-1], dtype=np.uint32), g])
    return rows, v, g


@functools.lru_cache(maxsize=None)
def cap_oracle(n):
    """oracle_fleet of cap_fleet(n) at r = 80, computed once and shared (do not modify)."""
    from oracle import OracleGraph

    rows, v, g = cap_fleet(n)
    off, idx = brute_case(f"cap{n}", 80)
    return oracle_fleet(OracleGraph(maps.rows_to_array(rows)), v, g, off, idx)


@functools.lru_cache(maxsize=None)
def long_rules123():
    """(rows, v, g, oracle result) of the 1,100 agents of `open40` for r = 80 (lists of 1,099 entries: the
    brute-force fill), decided by Rules 1-3 alone, so that k_decide never meets its 1,024-entry limit:
    everyone at their goal but 200 seeded agents with random goals, and then g = v for whoever the oracle
    leaves in Wait or Rotation, until nobody is."""
    from oracle import OracleGraph

    _, _, rows, v = nearby_shape("open40")
    rng = random.Random(123)
    g = v.copy()
    for i in rng.sample(range(v.size), 200):
        g[i] = rng.randrange(1600)
    og = OracleGraph(maps.rows_to_array(rows))
    off, idx = brute_case("open40", 80)
    for _ in range(10):
        ref = oracle_fleet(og, v, g, off, idx)
        stuck = ref[0] >= 2  # Rotation or Wait: the decision went past Rule 3
        if not stuck.any():
            return rows, v, g, ref
        g[stuck] = v[stuck]
    raise AssertionError("the repair passes did not end")


@functools.lru_cache(maxsize=None)
def crowd_fleet():
    """(W, H, rows, v): 2,048 * 256 + 2 agents (257 scan tiles of agents) on open_map(1024, 1024) for r = 0.
    Three seeded samples of one pool of 260,000 cells, shuffled together: most agents share their cell with
    one or two others, some with nobody, so nb_off is no simple ramp."""
    W = H = 1024
    n = SCAN_TILE * TILES_PER_CHUNK + 2
    rs = np.random.RandomState(257)
    pool = rs.choice(W * H, 260000, replace=False)
    v = np.concatenate([rs.choice(pool, k, replace=False) for k in (200000, 200000, n - 400000)])
    return W, H, maps.open_map(W, H), rs.permutation(v).astype(np.uint32)


def grouped_nearby(v):
    """The r = 0 lists without the n x n matrix: agent i's list is the other agents of its cell, ascending.
    A stable argsort of v puts every cell's agents next to each other in ascending index (CSR as brute_nearby)."""
    v = np.asarray(v, dtype=np.int64)
    n = v.size
    order = np.argsort(v, kind="stable")
    sv = v[order]
    start = np.flatnonzero(np.r_[True, sv[1:] != sv[:-1]]) if n else np.zeros(0, dtype=np.int64)
    size = np.diff(np.r_[start, n])
    gid = np.repeat(np.arange(start.size), size)  # group of the agent at sorted position p
    reps = size[gid]
    first = np.cumsum(reps) - reps
    q = np.repeat(start[gid], reps) + np.arange(int(reps.sum())) - np.repeat(first, reps)
    a, e = np.repeat(order, reps), order[q]  # every (agent, agent of its cell) pair, e ascending per agent
    a, e = a[a != e], e[a != e]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.bincount(a, minlength=n))
    return off, e[np.argsort(a, kind="stable")].astype(np.uint32)


def second_chunk_agents(name, r):
    """How many agents of a nearby shape have a list member in a row >= max(0, y - r) + 64, i.e. in a row
    that k_nb_count's lanes and k_nb_fill's chunks reach in their second trip or later."""
    W, _, _, v = nearby_shape(name)
    off, idx = brute_case(name, r)
    y = v.astype(np.int64) // W
    owner = np.repeat(np.arange(v.size), np.diff(off.astype(np.int64)))
    late = y[idx] >= np.maximum(0, y[owner] - r) + 64
    return np.unique(owner[late]).size


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
    if name in ("rand20", "warehouse", "tall9x200"):
        rows, v, _ = fleet_case(name)
        return len(rows[0]), len(rows), rows, v
    if name in ("cap1025", "cap1026"):
        rows, v, _ = cap_fleet(int(name[-4:]))
        return 40, 40, rows, v
    if name == "tall3x683":  # 2,049 cells: the cell scan's second tile holds one element; up to 683 rows
        W, H = 3, 683
        rng = random.Random(683)
        pts = rng.sample([(x, y) for y in range(H - 1) for x in range(W)], 148) + [(1, H - 1), (2, H - 1)]
        pts += [pts[rng.randrange(150)] for _ in range(10)] + [(2, H - 1)]
        rng.shuffle(pts)
        return W, H, maps.open_map(W, H), _cells(W, pts)
    if name == "tile64x32":  # 2,048 cells: the cell scan is one full tile (no block sums)
        W, H = 64, 32
        rng = random.Random(2048)
        pts = rng.sample([(x, y) for y in range(H) for x in range(W - 2)], 300) + [(W - 1, H - 1), (W - 2, H - 1)]
        pts += [pts[rng.randrange(302)] for _ in range(20)] + [(W - 1, H - 1)]
        rng.shuffle(pts)
        return W, H, maps.open_map(W, H), _cells(W, pts)
    if name in ("grid1024x512", "grid1024x513"):  # 256 and 257 tiles of cells: the block-sum scan's carry
        W, H = 1024, int(name[-3:])
        rng = random.Random(H)
        tail = [H - 1] if H == 513 else [H - 3, H - 2, H - 1]  # 1024 x 513: the row of cells >= 524,288
        pts = {(0, 0), (1, 0), (2, 0), (W - 1, H - 1), (W - 2, H - 1), (0, tail[0]), (3, tail[0])}
        for k, cx in enumerate((90, 480, 1000)):  # clusters in the tail rows, the last one against the right border
            while len(pts) < 7 + 16 * (k + 1):
                pts.add((cx + rng.randrange(24), rng.choice(tail)))
        for _ in range(12):  # above the last cluster: their rows end at the first cell of a tail row
            pts.add((1004 + rng.randrange(20), tail[0] - 1 - rng.randrange(3)))
        while len(pts) < 290:  # the rest anywhere above
            pts.add((rng.randrange(W), rng.randrange(H - 8)))
        pts = sorted(pts)
        pts += [pts[rng.randrange(290)] for _ in range(8)] + [(W - 1, H - 1), (1001, H - 1)]
        rng.shuffle(pts)
        return W, H, maps.open_map(W, H), _cells(W, pts)
    if name in ("agents2048", "agents2049"):  # one full tile of agents, and a second tile of one agent
        n = int(name[-4:])
        rng = random.Random(n)
        pts = rng.sample([(x, y) for y in range(64) for x in range(64)], 1500)
        pts += [pts[rng.randrange(1500)] for _ in range(n - 1500)]  # with replacement: co-located agents
        rng.shuffle(pts)
        return 64, 64, maps.open_map(64, 64), _cells(64, pts)
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
                ("rand20", 3), ("rand20", 15), ("warehouse", 15), ("open40", 80), ("one", 15), ("none", 15),
                # diamonds of 63 rows (one partial chunk of 64), 65 (a second chunk of one row), up to 200, clamped
                ("tall9x200", 31), ("tall9x200", 32), ("tall9x200", 100), ("tall9x200", 300),
                ("tall3x683", 15), ("tall3x683", 64), ("tall3x683", 700),
                # the scan's tiles of 2,048: cells 2,048 (tall3x683: 2,049), 256 and 257 tiles; agents 2,048 / 2,049
                ("tile64x32", 15), ("grid1024x512", 15), ("grid1024x513", 15), ("agents2048", 1), ("agents2049", 1),
                # lists of exactly 1,024 entries (the LDS sort's capacity) and 1,025 (the first brute-force size)
                ("cap1025", 80), ("cap1026", 80)]

SCAN_TILE = 2048  # NB_SCAN_TILE of tsw_nearby.h
TILES_PER_CHUNK = 256  # tiles k_scan_sums scans per trip (NB_BLOCK)


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
