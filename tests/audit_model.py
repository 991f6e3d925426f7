"""The audit of plan records (include/tswap.h, above tsw_audit_records) as brute force in plain Python,
shared by test_audit_model.py (CPU) and test_gpu_audit.py (GPU): per column a dict from cell to the agents
on it and a set of the directed edges taken into it. It knows nothing of the kernels' two passes. Also the
hand-built cases with their counts worked out by hand, and the random records. No test in here."""
import functools

import numpy as np

NCOL, NAGENT, NKIND = 11, 4, 5
NONE = 0xFFFFFFFF
KINDS = ("colocation", "swap", "jump", "off_map", "bad_state")
PICKING, CARRYING, DELIVERED, IDLE = 0, 1, 2, 3
SUM_FIELDS = ("bad_state", "moves", "deliveries", "colocations", "swaps", "jumps", "off_map")  # col words 4 .. 10


def pack(x, y, state=IDLE):
    return int(x) | int(y) << 16 | int(state) << 32


def records(rows_of_columns):
    """(n, T) uint64 from one list per agent of (x, y) or (x, y, state) per column."""
    return np.array([[pack(*c) for c in agent] for agent in rows_of_columns], dtype=np.uint64).reshape(
        len(rows_of_columns), -1)


def audit_model(rows, rec):
    """(sum, col, agents) of the records on the grid `rows` (list of strings, '@' blocked): sum a dict with
    tsw_audit's fields, col (T, 11) uint32, agents (n, 4) uint32."""
    h, w = len(rows), len(rows[0])
    rec = np.asarray(rec, dtype=np.uint64)
    n, T = (rec.shape if rec.ndim == 2 else (0, 0))
    col = np.zeros((T, NCOL), dtype=np.uint32)
    agents = np.zeros((n, NAGENT), dtype=np.uint32)
    agents[:, 3] = NONE
    first = [None] * NKIND
    xs = (rec & np.uint64(0xFFFF)).astype(np.int64).tolist()
    ys = ((rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64).tolist()
    ss = ((rec >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64).tolist()
    for t in range(T):
        charged = [set() for _ in range(NKIND)]
        on_cell = {}   # cell -> agents on it, ascending
        edges = {}     # (from cell, to cell) -> agents taking it
        for i in range(n):
            x, y, s = xs[i][t], ys[i][t], ss[i][t]
            on = x < w and y < h
            if s <= 3:
                col[t, s] += 1
            else:
                col[t, 4] += 1
                charged[4].add(i)
            if not on or rows[y][x] == "@":
                col[t, 10] += 1
                charged[3].add(i)
            if on:
                on_cell.setdefault((x, y), []).append(i)
            delivered_before = False
            if t > 0:
                px, py = xs[i][t - 1], ys[i][t - 1]
                delivered_before = ss[i][t - 1] == DELIVERED
                dist = abs(x - px) + abs(y - py)
                if dist:
                    col[t, 5] += 1
                    agents[i, 0] += 1
                if dist > 1:
                    col[t, 9] += 1
                    charged[2].add(i)
                if dist == 1 and on and px < w and py < h:
                    edges.setdefault(((px, py), (x, y)), []).append(i)
            if s == DELIVERED and not delivered_before:
                col[t, 6] += 1
                agents[i, 1] += 1
        for members in on_cell.values():
            charged[0].update(members[1:])
        for (a, b), takers in edges.items():
            if (b, a) in edges:
                charged[1].update(takers)
        col[t, 7], col[t, 8] = len(charged[0]), len(charged[1])
        for k in range(NKIND):
            if charged[k] and first[k] is None:
                first[k] = (t, min(charged[k]))
        for i in set().union(*charged):
            agents[i, 2] += 1
            if agents[i, 3] == NONE:
                agents[i, 3] = t
    c64 = col.astype(np.uint64)
    out = {"state_steps": [int(c64[:, k].sum()) for k in range(4)]}
    for k, name in enumerate(SUM_FIELDS):
        out[name] = int(c64[:, 4 + k].sum())
    out["moving_columns"] = int(np.count_nonzero(col[1:, 5])) if T > 1 else 0
    out["first_t"] = [NONE if f is None else f[0] for f in first]
    out["first_agent"] = [NONE if f is None else f[1] for f in first]
    return out, col, agents


def assert_equal(got, ref, what=""):
    """A Planner.audit result (with col and agents) against audit_model's triple, word for word."""
    rsum, rcol, ragents = ref
    for k, v in rsum.items():
        assert got[k] == v, f"{what} sum.{k}: device {got[k]} model {v}"
    for name, a, b in (("col", got["col"], rcol), ("agents", got["agents"], ragents)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what} {name}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if not np.array_equal(a, b):
            r, k = (int(q[0]) for q in np.nonzero(a != b))
            raise AssertionError(f"{what} {name}[{r}, {k}]: device {int(a[r, k])} model {int(b[r, k])}")


# ---- hand-built cases -------------------------------------------------------------------------------

HAND_ROWS = ["......",
             "..@...",
             "......",
             "......"]  # 6 x 4, (2, 1) blocked

# name -> (records, the sum fields that are not zero; "first": kind -> (column, agent) of its first violation)
HAND = {
    # agents 0 and 1 exchange (0,0) and (1,0): each takes the edge against the other
    "exchange": (records([[(0, 0), (1, 0)], [(1, 0), (0, 0)]]),
                 dict(moves=2, swaps=2, first={1: (1, 0)})),
    # a closed 3-cycle: on a 4-connected grid its third leg is a diagonal (a jump); nobody meets anybody head-on
    "3-cycle": (records([[(0, 0), (1, 0)], [(1, 0), (1, 1)], [(1, 1), (0, 0)]]),
                dict(moves=3, jumps=1, first={2: (1, 2)})),
    # four agents rotate around a unit square, every leg a unit step
    "4-cycle": (records([[(0, 2), (1, 2)], [(1, 2), (1, 3)], [(1, 3), (0, 3)], [(0, 3), (0, 2)]]),
                dict(moves=4)),
    # three agents on one cell: the two larger indices are charged
    "three-on-a-cell": (records([[(3, 2)], [(3, 2)], [(3, 2)]]),
                        dict(colocations=2, first={0: (0, 1)})),
    # agents 0 and 1, co-located on (0,0), both cross agent 2 coming from (1,0): 3 swaps; agent 1 stands
    # behind agent 0 in both columns: 2 colocations
    "two-cross-one": (records([[(0, 0), (1, 0)], [(0, 0), (1, 0)], [(1, 0), (0, 0)]]),
                      dict(moves=3, swaps=3, colocations=2, first={0: (0, 1), 1: (1, 0)})),
    # a distance-2 hop and a diagonal step
    "jumps": (records([[(0, 0), (2, 0)], [(4, 3), (5, 2)]]),
              dict(moves=2, jumps=2, first={2: (1, 0)})),
    # (2,1) is blocked; x == w is off the grid
    "off-map": (records([[(2, 1)], [(6, 0)]]),
                dict(off_map=2, first={3: (0, 0)})),
    "state-7": (records([[(0, 0, 7)], [(1, 0, PICKING)]]),
                dict(bad_state=1, first={4: (0, 0)})),
    # DELIVERED held over two columns is one delivery
    "delivered-held": (records([[(0, 0, CARRYING), (0, 0, DELIVERED), (0, 0, DELIVERED), (0, 0, IDLE)]]),
                       dict(deliveries=1)),
    # DELIVERED in column 0 counts; DELIVERED again after CARRYING is a second delivery
    "delivered-again": (records([[(0, 0, DELIVERED), (0, 0, DELIVERED), (0, 0, CARRYING), (0, 0, DELIVERED)]]),
                        dict(deliveries=2)),
}


def hand_expected(name):
    """The whole expected sum of a hand-built case: the fields its row names, everything else zero / none.
    state_steps is left out (n * T spread over the states)."""
    given = HAND[name][1]
    out = {k: given.get(k, 0) for k in SUM_FIELDS}
    out["moving_columns"] = 1 if given.get("moves") else 0  # the moving cases have two columns
    out["first_t"], out["first_agent"] = [NONE] * NKIND, [NONE] * NKIND
    for kind, (t, agent) in given.get("first", {}).items():
        out["first_t"][kind], out["first_agent"][kind] = t, agent
    return out


# ---- random records ---------------------------------------------------------------------------------

def random_records(rows, n, T, seed, dup=0.05, off=0.01, bad=0.01, jump=0.01):
    """Random walks on the free cells of `rows` (stay or a unit step, never into a wall) with, sprinkled in:
    agents pulled onto another agent's cell (duplicates, and with them head-on exchanges), records off the
    grid or on a blocked cell, states > 3 and teleports. (n, T) uint64."""
    h, w = len(rows), len(rows[0])
    rng = np.random.default_rng(seed)
    free = [(x, y) for y in range(h) for x in range(w) if rows[y][x] != "@"]
    blocked = [(x, y) for y in range(h) for x in range(w) if rows[y][x] == "@"] or [(w, 0)]
    pos = [free[k] for k in rng.integers(0, len(free), n)]
    rec = np.zeros((n, T), dtype=np.uint64)
    steps = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))
    for t in range(T):
        for i in range(n):
            x, y = pos[i]
            u = rng.random()
            if u < jump:
                x, y = free[rng.integers(0, len(free))]
            elif u < jump + dup and n > 1:
                x, y = pos[int(rng.integers(0, n))]  # this column's cell of a smaller index, last column's of a larger
            else:
                dx, dy = steps[rng.integers(0, 5)]
                if 0 <= x + dx < w and 0 <= y + dy < h and rows[y + dy][x + dx] != "@":
                    x, y = x + dx, y + dy
            pos[i] = (x, y)
            state = int(rng.integers(0, 4))
            rx, ry = x, y
            u = rng.random()
            if u < off:  # the record only: the walk goes on from the cell
                rx, ry = blocked[rng.integers(0, len(blocked))] if rng.random() < 0.5 else ((w + int(rng.integers(0, 3)), y) if rng.random() < 0.5 else (x, h + int(rng.integers(0, 3))))
            elif u < off + bad:
                state = int(rng.integers(4, 256))
            rec[i, t] = pack(rx, ry, state)
    return rec


def swap_walks(rows, n, T, seed):
    """Records dense in exchanges: agents 2j and 2j + 1 stand on neighbouring free cells and trade places in
    every transition (pairs may share cells with other pairs). (n, T) uint64."""
    h, w = len(rows), len(rows[0])
    rng = np.random.default_rng(seed)
    pairs = [((x, y), (x + 1, y)) for y in range(h) for x in range(w - 1) if rows[y][x] != "@" and rows[y][x + 1] != "@"]
    pairs += [((x, y), (x, y + 1)) for y in range(h - 1) for x in range(w) if rows[y][x] != "@" and rows[y + 1][x] != "@"]
    rec = np.zeros((n, T), dtype=np.uint64)
    ends = None
    for i in range(n):
        if i % 2 == 0:
            ends = pairs[int(rng.integers(0, len(pairs)))]
        for t in range(T):
            rec[i, t] = pack(*ends[(i + t) % 2], int(rng.integers(0, 4)))
    return rec


def edge_rows(w, h):
    """An open w x h grid with blocked cells beside its last corner and in its first row."""
    rows = [bytearray(b"." * w) for _ in range(h)]
    for x, y in ((w - 3, h - 1), (w - 1, h - 3), (1, 0), (w // 2, h // 2)):
        rows[y][x] = ord("@")
    return [r.decode() for r in rows]


def edge_records(w, h, n, T, seed):
    """Records for a large grid without listing its cells: agents start in the last row, the last column,
    the last corner and anywhere, walk by unit steps clipped to the grid (blocked cells are walked over: they
    are off_map, still on the grid), are now and then pulled onto another agent's cell, and agents 0 and 1
    trade the last two cells of the last row in every transition. (n, T) uint64."""
    rng = np.random.default_rng(seed)
    pos = []
    for i in range(n):
        k = i % 4
        pos.append((int(rng.integers(0, w)), h - 1) if k == 0 else (w - 1, int(rng.integers(0, h))) if k == 1
                   else (w - 1, h - 1) if k == 2 else (int(rng.integers(0, w)), int(rng.integers(0, h))))
    steps = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))
    rec = np.zeros((n, T), dtype=np.uint64)
    for t in range(T):
        for i in range(n):
            x, y = pos[i]
            if rng.random() < 0.05:
                x, y = pos[int(rng.integers(0, n))]
            else:
                dx, dy = steps[rng.integers(0, 5)]
                x, y = min(max(x + dx, 0), w - 1), min(max(y + dy, 0), h - 1)
            if i < 2 <= n:
                x, y = w - 1 - (i + t) % 2, h - 1
            pos[i] = (x, y)
            rec[i, t] = pack(x, y, int(rng.integers(0, 4)))
    return rec


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """(rows, rec, model) of the n = 300, T = 70 random records on a 20 x 16 map with obstacles (do not modify)."""
    from p2p_distributed_tswap_amd import maps

    rows = maps.random_map(20, 16, 0.2, 5)
    rec = random_records(rows, 300, 70, seed)
    return rows, rec, audit_model(rows, rec)
