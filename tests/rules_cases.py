"""Built states for k_plan's rules phase (SEC_RULES, csrc/tsw_plan_kernel.h + tsw_plan_rules.h) and a counting
restatement of the sequential phase. Shared by test_rules_cases.py (CPU: every case is what it claims) and
test_gpu_rules.py (GPU: Planner.step against OracleGraph.step, and the kernel's counters against the restatement's).
No test in here.

A case is a map, positions v and goals g (cell ids, one agent per cell) for Planner.step / OracleGraph.step, built
deterministically from its name. Families (case(name).__doc__ of each builder says what the oracle does with it):

  ring-<L>-d<d>-<numbering>   one closed corridor of L cells, an agent per cell, goals d cells ahead: d rule-4
                              rotations of the L-cycle in one phase
  rings2                      two disjoint rings on 34x34, one inside the other
  convoy-<K>                  one rule-3 swap whose s gets a successor chain of K moving agents (the batched walk's cap)
  cascade-<K>-<inc|dec>       a 1 x (K + 1) corridor: a far goal handed down the line by K rule-3 swaps (inc), or by
                              one swap per step (dec); cascade-<K>-chain is dec called K times
  pairs-<P>-<adj|split>       P head-on pairs in 1-wide rows: P rotations of 2-cycles
  mixed                       pairs, a 4-cycle and a cascade of 5 in one 64-agent chunk
  close-<k>                   seeded dense states in which a rule-3 swap closes a new cycle
  close-ring                  two swaps of one chunk that close a ring together (the batch's cut by walk marks)
  field-cascade-<K>, field-pairs
                              the cascade and the pairs inside an open field: next hops with two candidates
"""
from __future__ import annotations

import dataclasses
import functools
import random

import numpy as np

from oracle import OracleGraph
from p2p_distributed_tswap_amd import maps

CHUNK = 64        # agents per ballot of the wave rules rounds
LIST_CAP = 1024   # entries of the changed list (tsw_plan_dev.h)
WALK_CAP = 16     # Tunables::walk_cap: hops of a batched firing's successor walk


# ---- the sequential phase, counted -----------------------------------------------------------------------------
class NextHop:
    """OracleGraph.get_path_next, memoised per (cell, goal): the next cell, or None when the path has no step."""

    def __init__(self, og):
        self.og, self.memo = og, {}

    def __call__(self, v, g):
        key = (v, g)
        if key not in self.memo:
            nxt, ln, _ = self.og.get_path_next(v, g)
            self.memo[key] = nxt if ln >= 2 else None
        return self.memo[key]


@dataclasses.dataclass
class Counters:
    firings: list = dataclasses.field(default_factory=list)    # (agent, kind 3 | 4, cycle length; 0 for a swap) in order
    partners: list = dataclasses.field(default_factory=list)   # s of each firing (the successor of the firing agent)
    closes: int = 0                                            # rule-3 swaps that close a new cycle through s
    walk_hops: list = dataclasses.field(default_factory=list)  # per rule-3 swap: agents on s's new successor chain
    rot_per_cycle: dict = dataclasses.field(default_factory=dict)  # frozenset(members) -> rotations

    @property
    def n(self):
        return len(self.firings)

    @property
    def swaps(self):
        return sum(1 for f in self.firings if f[1] == 3)

    @property
    def rotations(self):
        return sum(1 for f in self.firings if f[1] == 4)

    @property
    def rotations2(self):
        return sum(1 for f in self.firings if f[1] == 4 and f[2] == 2)

    @property
    def longest_cascade(self):
        """Longest chain of rule-3 firings in which each firing's s is the agent of the chain's next firing (other
        agents may fire in between)."""
        depth, best = {}, 0
        for (a, kind, _), s in zip(self.firings, self.partners):
            if kind == 3:
                d = depth.pop(a, 0) + 1
                depth[s] = d
                best = max(best, d)
        return best

    @property
    def per_chunk(self):
        d = {}
        for a, _, _ in self.firings:
            d[a // CHUNK] = d.get(a // CHUNK, 0) + 1
        return d

    @property
    def r4_after_r3_in_chunk(self):
        """Chunks in which a rule-4 firing follows a rule-3 firing."""
        seen3, out = set(), set()
        for a, kind, _ in self.firings:
            if kind == 3:
                seen3.add(a // CHUNK)
            elif a // CHUNK in seen3:
                out.add(a // CHUNK)
        return out

    def add(self, other):
        self.firings += other.firings
        self.partners += other.partners
        self.closes += other.closes
        self.walk_hops += other.walk_hops
        for k, c in other.rot_per_cycle.items():
            self.rot_per_cycle[k] = self.rot_per_cycle.get(k, 0) + c


def restate(nh, v, g):
    """tswap.rs:180-252: one pass in agent order; rule 3 when the successor rests on its goal, rule 4 when the chase
    returns to the firing agent. nh: NextHop. Returns (goals after the phase, Counters)."""
    v = [int(x) for x in v]
    g = [int(x) for x in g]
    n = len(v)
    pos = {}
    for k in range(n - 1, -1, -1):  # position(): the lowest index on a cell
        pos[v[k]] = k
    C = Counters()

    def succ(k):
        if v[k] == g[k]:
            return None
        u = nh(v[k], g[k])
        return None if u is None else pos.get(u)

    for i in range(n):
        if v[i] == g[i]:
            continue
        u = nh(v[i], g[i])
        if u is None:
            continue
        j = pos.get(u)
        if j is None or j == i:
            continue
        if v[j] == g[j]:  # rule 3 (:198-202)
            g[i], g[j] = g[j], g[i]
            C.firings.append((i, 3, 0))
            C.partners.append(j)
            # j was terminal: a cycle through j now is a new one
            x, steps = succ(j), 0
            while x is not None and x != j and steps <= n:
                x, steps = succ(x), steps + 1  # steps: agents passed
            if x == j:
                C.closes += 1
            C.walk_hops.append(steps + (x is not None))
            continue
        ap, b, found = [i], j, False  # rule 4 (:204-249)
        while True:
            if v[b] == g[b]:
                break
            w = nh(v[b], g[b])
            if w is None:
                break
            c = pos.get(w)
            if c is None:
                break
            if b in ap:
                ap = []
                break
            ap.append(b)
            b = c
            if b == i:
                found = True
                break
        if found and len(ap) > 1:
            last = g[ap[-1]]
            for k in range(len(ap) - 1, 0, -1):
                g[ap[k]] = g[ap[k - 1]]
            g[ap[0]] = last
            C.firings.append((i, 4, len(ap)))
            C.partners.append(j)
            key = frozenset(ap)
            C.rot_per_cycle[key] = C.rot_per_cycle.get(key, 0) + 1
    return np.array(g, dtype=np.uint32), C


# ---- cases -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    rows: tuple          # the map
    v: np.ndarray        # positions (cell ids)
    g: np.ndarray        # goals
    calls: int = 1       # step calls, each fed the result of the one before (the chained cascade)
    moved: object = None  # agents that change cell over the calls, as the builder's docstring says (None: not stated)
    doc: str = ""

    @property
    def n(self):
        return int(self.v.size)

    @property
    def map_key(self):
        return self.rows


def _blocked(w, h):
    return np.ones((h, w), dtype=bool)


def ring_loop(w, h, x0=0, y0=0):
    """(x, y) of the border of the w x h box at (x0, y0), in loop order: top row left to right, right column down,
    bottom row right to left, left column up. 2 (w + h) - 4 cells."""
    top = [(x0 + i, y0) for i in range(w)]
    right = [(x0 + w - 1, y0 + j) for j in range(1, h)]
    bottom = [(x0 + i, y0 + h - 1) for i in range(w - 2, -1, -1)]
    left = [(x0, y0 + j) for j in range(h - 2, 0, -1)]
    return top + right + bottom + left


RING_BOX = {4: (2, 2), 10: (4, 3), 62: (17, 16), 64: (17, 17), 66: (18, 17), 128: (33, 33)}
SPREAD_CHUNKS = 16  # the spread numbering: members in chunks 1 .. 16, chunk 0 holds resting agents only


def spread_index(p):
    """Loop position p -> agent index: consecutive positions 64 apart, chunk 0 left to the fillers."""
    return CHUNK * (1 + p % SPREAD_CHUNKS) + p // SPREAD_CHUNKS


def ring(L, d, numbering):
    """A w x h box whose border is one closed corridor of L cells, an agent on every cell, each goal d cells ahead
    along the loop. The oracle rotates the L-cycle d times in the one phase (the d lowest-numbered members fire one
    after another), all L goals change, every agent ends on its goal and nobody moves. `spread` puts consecutive
    loop positions 64 indices apart on a 64-wide map and fills the other indices (n = 1,088) with agents resting on
    their goals in a strip below the ring: no firing member lies in chunk 0."""
    w, h = RING_BOX[L]
    loop = ring_loop(w, h)
    assert len(loop) == L and 2 * d < L
    if numbering == "spread":
        W, H = CHUNK, h + 2 + SPREAD_CHUNKS + 1
        n = CHUNK * (SPREAD_CHUNKS + 1)
        idx = [spread_index(p) for p in range(L)]
    else:
        W, H, n = w, h, L
        idx = {"id": list(range(L)), "rev": list(range(L - 1, -1, -1)),
               "perm": random.Random(1000 + L).sample(range(L), L)}[numbering]
    blk = _blocked(W, H)
    for x, y in loop:
        blk[y, x] = False
    v = np.zeros(n, dtype=np.uint32)
    g = np.zeros(n, dtype=np.uint32)
    for p, (x, y) in enumerate(loop):
        gx, gy = loop[(p + d) % L]
        v[idx[p]], g[idx[p]] = y * W + x, gy * W + gx
    if numbering == "spread":
        blk[h + 2:, :] = False
        strip = [(h + 2) * W + c for c in range(n)]
        used = set(idx)
        rest = [k for k in range(n) if k not in used]
        for k, c in zip(rest, strip):
            v[k] = g[k] = c
    return Case(f"ring-{L}-d{d}-{numbering}", tuple(maps.to_rows(blk)), v, g, moved=0, doc=ring.__doc__)


def rings2():
    """34x34: the border ring (L = 132, goals 1 ahead) and, inside a blocked ring, the border of the 30x30 box at
    (2, 2) (L = 116, goals 3 ahead). Outer members take the even indices while they last, inner ones the odd. The
    oracle rotates the outer cycle once and the inner one three times; nobody moves."""
    outer, inner = ring_loop(34, 34), ring_loop(30, 30, 2, 2)
    blk = _blocked(34, 34)
    for x, y in outer + inner:
        blk[y, x] = False
    order = []
    for p in range(len(outer)):
        order.append((outer, p, 1))
        if p < len(inner):
            order.append((inner, p, 3))
    v = np.array([lp[p][1] * 34 + lp[p][0] for lp, p, _ in order], dtype=np.uint32)
    g = np.array([lp[(p + d) % len(lp)][1] * 34 + lp[(p + d) % len(lp)][0] for lp, p, d in order], dtype=np.uint32)
    return Case("rings2", tuple(maps.to_rows(blk)), v, g, moved=0, doc=rings2.__doc__)


def cascade(K, order):
    """A 1 x (K + 1) corridor, an agent on every cell and on its own goal, except the agent on cell 0 whose goal is
    cell K. `inc` (indices increase along the corridor): the oracle hands the far goal down the line in the one phase,
    K rule-3 swaps, each firing's s the next firing agent, K goals change. `dec` (indices decrease): exactly one swap
    per step; `chain` is dec stepped K times, each call fed the result of the one before (K swaps in all). Nobody
    moves."""
    W = K + 1
    cells = list(range(W))
    idx = cells if order == "inc" else cells[::-1]
    v = np.zeros(W, dtype=np.uint32)
    g = np.zeros(W, dtype=np.uint32)
    for c in cells:
        v[idx[c]] = c
        g[idx[c]] = K if c == 0 else c
    return Case(f"cascade-{K}-{order}", tuple(maps.open_map(W, 1)), v, g, calls=K if order == "chain" else 1, moved=0,
                doc=cascade.__doc__)


def convoy(K):
    """A 1 x (K + 4) corridor. Agent 0 on cell 0 heads for cell K + 3; agent 1 rests on its goal, cell 1; agents
    2 .. K + 1 on cells 2 .. K + 1 each head for the next cell (the last one for the free cell K + 2): a convoy whose
    successor chain has K agents and ends at a free cell. The oracle makes one rule-3 swap (0, 1): agent 1 takes the
    far goal, and its new successor chain is the whole convoy — the walk a batched firing must make before it may
    join a batch, K agents long (walk_cap = 16: K = 15 fits, 16 and 17 do not). Only the convoy's last agent
    moves."""
    W = K + 4
    v = np.arange(K + 2, dtype=np.uint32)
    g = v + 1
    g[0], g[1] = K + 3, 1
    return Case(f"convoy-{K}", tuple(maps.open_map(W, 1)), v, g, moved=1, doc=convoy.__doc__)


def _pair_rows(P, W=CHUNK):
    per_row = W // 4
    nrows = (P + per_row - 1) // per_row
    blk = _blocked(W, 2 * nrows - 1)
    blk[0::2, :] = False
    return blk, per_row


def pairs(P, numbering):
    """A 64-wide map whose even rows are free and odd rows blocked; 16 pairs a row, four cells c .. c + 3 a pair:
    agents on c + 1 and c + 2 with goals c + 3 and c + 0. The oracle rotates every 2-cycle (one rule-4 firing a pair,
    by its lower-numbered member), both goals of every pair change and everybody moves. `adj`: members 2p and 2p + 1;
    `split`: p and P + p."""
    blk, per_row = _pair_rows(P)
    W = blk.shape[1]
    v = np.zeros(2 * P, dtype=np.uint32)
    g = np.zeros(2 * P, dtype=np.uint32)
    for p in range(P):
        c = 2 * (p // per_row) * W + 4 * (p % per_row)
        a, b = (2 * p, 2 * p + 1) if numbering == "adj" else (p, P + p)
        v[a], g[a] = c + 1, c + 3
        v[b], g[b] = c + 2, c + 0
    return Case(f"pairs-{P}-{numbering}", tuple(maps.to_rows(blk)), v, g, moved=2 * P, doc=pairs.__doc__)


MIXED_PAIRS, MIXED_K = 6, 5


def mixed():
    """One chunk (22 agents) on a 64x6 map: six head-on pairs in row 0, a 2x2 ring with goals 1 ahead in rows 2-3,
    a cascade of 5 in row 5 (indices increasing along it). Numbering: pair 0, cascade 0, pair 1, cascade 1, pair 2,
    cascade 2, the ring's four, then pair 3, cascade 3, ... — the cascade's agents between the pairs'. The oracle
    makes 6 rotations of 2-cycles, one of the 4-cycle and 5 swaps; the 12 pair agents move, nobody else."""
    W = CHUNK
    blk = _blocked(W, 6)
    blk[0, :] = False
    blk[2:4, 0:2] = False
    blk[5, 0:MIXED_K + 1] = False
    ringc = ring_loop(2, 2, 0, 2)
    vs, gs = [], []

    def put(cv, cg):
        vs.append(cv)
        gs.append(cg)

    def casc(c):
        put(5 * W + c, 5 * W + (MIXED_K if c == 0 else c))

    for p in range(MIXED_PAIRS):
        c = 4 * p
        put(c + 1, c + 3)
        put(c + 2, c + 0)
        casc(p)
        if p == 2:
            for q, (x, y) in enumerate(ringc):
                gx, gy = ringc[(q + 1) % 4]
                put(y * W + x, gy * W + gx)
    assert MIXED_PAIRS == MIXED_K + 1  # one cascade agent after every pair
    return Case("mixed", tuple(maps.to_rows(blk)), np.array(vs, dtype=np.uint32), np.array(gs, dtype=np.uint32),
                moved=2 * MIXED_PAIRS, doc=mixed.__doc__)


# seeds of dense_state() whose phase holds a rule-3 swap that closes a new cycle (found by search_closing())
CLOSE_W, CLOSE_H, CLOSE_BLOCK, CLOSE_FILL = 14, 10, 0.25, 0.6
CLOSE_SEEDS = (20, 32, 83)


def dense_state(seed):
    """A seeded dense corridor state: random_map(14, 10, 0.25), agents on 60 % of the largest component's cells, goals
    a seeded draw of distinct cells of it."""
    rows = maps.random_map(CLOSE_W, CLOSE_H, CLOSE_BLOCK, seed)
    comp = [y * CLOSE_W + x for x, y in maps.largest_component(rows)]
    rng = random.Random(seed)
    n = min(int(len(comp) * CLOSE_FILL), 128)
    return rows, np.array(rng.sample(comp, n), dtype=np.uint32), np.array(rng.sample(comp, n), dtype=np.uint32)


def search_closing(seeds, want=3):
    """Seeds of dense_state whose restated phase counts a closing swap (how CLOSE_SEEDS was found)."""
    out = []
    for s in seeds:
        rows, v, g = dense_state(s)
        _, C = restate(NextHop(OracleGraph(maps.rows_to_array(list(rows)))), v, g)
        if C.closes > 0:
            out.append(s)
            if len(out) == want:
                break
    return out


def close_ring():
    """Two rule-3 swaps that close a cycle together, on the 10-cell ring of the 4x3 box. Along the loop stand agents
    0, 3, 4, 5, 1, 2, 6, 7, 8, 9: agents 3 and 2 rest on their goals, the other eight head 2 or 3 cells ahead, all
    goals distinct. Agent 0 swaps with 3, agent 1 with 2. After the first swap the successor chain of 3 ends at the
    resting 2; only the second swap, whose s (agent 2) gets the chain 6, 7, 8, 9, 0, 3, 4, 5, 1 back to itself, closes
    the ring. In a batch, lane 1's walk passes agents 0 and 3, which lane 0 marked, while its own agent, successor
    and new successor carry no earlier mark, and no lane between the two carries one either: only the marks met on
    the walk (`cw`) cut the batch at lane 1. The oracle then rotates the 10-cycle from agent 2; nobody moves."""
    loop = ring_loop(4, 3)
    index = [0, 3, 4, 5, 1, 2, 6, 7, 8, 9]
    ahead = [3, 0, 2, 3, 3, 0, 2, 2, 2, 3]
    blk = _blocked(4, 3)
    for x, y in loop:
        blk[y, x] = False
    v = np.zeros(10, dtype=np.uint32)
    g = np.zeros(10, dtype=np.uint32)
    for p, (x, y) in enumerate(loop):
        gx, gy = loop[(p + ahead[p]) % 10]
        v[index[p]], g[index[p]] = y * 4 + x, gy * 4 + gx
    assert len(set(g.tolist())) == 10
    return Case("close-ring", tuple(maps.to_rows(blk)), v, g, moved=0, doc=close_ring.__doc__)


def close(k):
    """dense_state(CLOSE_SEEDS[k]): at least one rule-3 swap of the phase gives s a successor whose chain leads back
    to s (FO_RESCAN in fire(), the batch's closing cut, the fast path's labelling loop). Positions: the oracle's."""
    rows, v, g = dense_state(CLOSE_SEEDS[k])
    return Case(f"close-{k}", tuple(rows), v, g, doc=close.__doc__)


FIELD_H = 24
ORIENTS = [(dx, dy) for dx in (1, -1) for dy in (1, -1)]


def _field_cascade(K, dx, dy):
    W = 40 if K <= 30 else K + 10
    x0 = 4 if dx > 0 else W - 5
    y0 = FIELD_H // 2
    v = np.array([y0 * W + x0 + dx * i for i in range(K + 1)], dtype=np.uint32)
    g = v.copy()
    g[0] = (y0 + 4 * dy) * W + x0 + dx * (K + 4)  # diagonal from the line, past its end
    return Case(f"field-cascade-{K}", tuple(maps.open_map(W, FIELD_H)), v, g, moved=1)


def _field_pairs(axis, dx, dy, P=8):
    W = 40
    y0 = FIELD_H // 2
    vs, gs = [], []
    for p in range(P):
        if axis == "h":  # members side by side, goals diagonal past the partner
            xa = 6 + 4 * p if dx > 0 else W - 7 - 4 * p
            vs += [y0 * W + xa, y0 * W + xa + dx]
            gs += [(y0 + 5 * dy) * W + xa + 6 * dx, (y0 - 5 * dy) * W + xa - 5 * dx]
        else:  # one above the other
            xa = 8 + 3 * p
            vs += [y0 * W + xa, (y0 + 1) * W + xa]
            gs += [(y0 + 6) * W + xa + 5 * dx, (y0 - 5) * W + xa + 5 * dy]
    return Case("field-pairs", tuple(maps.open_map(W, FIELD_H)), np.array(vs, dtype=np.uint32),
                np.array(gs, dtype=np.uint32))


def _first_orientation(build, enough, orients=ORIENTS):
    for o in orients:
        c = build(*o)
        _, C = restate(NextHop(OracleGraph(maps.rows_to_array(list(c.rows)))), c.v, c.g)
        if enough(C):
            return c
    raise AssertionError("no orientation of the field case fires as wanted")


def field_cascade(K):
    """The cascade line (K + 1 agents in a row, each on its goal) inside an open 24-high field, the head's goal
    diagonal from the line past its end: from every cell of the line the far goal's next hop has two candidates, so
    under lazy next hops a firing's new code is unknown until a worker or a K3 pass answers. Of the four orientations
    (line east / west, goal below / above) the first one for which the oracle's tie-break walks the goal down the
    whole line: K swaps; then the last agent alone moves."""
    c = _first_orientation(lambda dx, dy: _field_cascade(K, dx, dy), lambda C: C.swaps >= K)
    return dataclasses.replace(c, doc=field_cascade.__doc__)


def field_pairs():
    """Eight head-on pairs in an open 40x24 field, goals diagonal past the partner: the first orientation (members
    side by side or one above the other, goals left / right) in which the oracle's tie-break sends both members at
    each other and it fires once per pair. Positions: the oracle's."""
    c = _first_orientation(_field_pairs, lambda C: C.rotations2 == 8 and C.n == 8,
                           [(a, dx, dy) for a in "hv" for dx, dy in ORIENTS])
    return dataclasses.replace(c, doc=field_pairs.__doc__)


RING_CASES = [(4, 1, "id"), (10, 1, "id"), (10, 3, "rev"), (62, 1, "perm"), (62, 3, "id"), (64, 1, "id"), (64, 3, "id"),
              (64, 3, "rev"), (64, 3, "perm"), (64, 3, "spread"), (66, 1, "id"), (66, 3, "perm"), (66, 3, "spread"),
              (128, 1, "rev"), (128, 3, "id"), (10, 3, "spread")]
CASCADE_K = [15, 16, 17, 63, 64, 65, 130]
CHAIN_K = [17, 65]
CONVOY_K = [15, 16, 17]
PAIR_P = [1, 31, 32, 33, 512, 513]
FIELD_K = [20, 70]

RING_NAMES = [f"ring-{L}-d{d}-{o}" for L, d, o in RING_CASES] + ["rings2"]
CASCADE_NAMES = [f"cascade-{K}-{o}" for K in CASCADE_K for o in ("inc", "dec")] + [f"cascade-{K}-chain" for K in CHAIN_K]
PAIR_NAMES = [f"pairs-{P}-{o}" for P in PAIR_P for o in ("adj", "split")]
CLOSE_NAMES = [f"close-{k}" for k in range(len(CLOSE_SEEDS))] + ["close-ring"]
FIELD_NAMES = [f"field-cascade-{K}" for K in FIELD_K] + ["field-pairs"]
CONVOY_NAMES = [f"convoy-{K}" for K in CONVOY_K]
NAMES = RING_NAMES + CASCADE_NAMES + CONVOY_NAMES + PAIR_NAMES + ["mixed"] + CLOSE_NAMES + FIELD_NAMES


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    """The named case, built once; its arrays are read-only."""
    c = _build(name)
    c.v.setflags(write=False)
    c.g.setflags(write=False)
    return c


def _build(name) -> Case:
    parts = name.split("-")
    if name == "rings2":
        return rings2()
    if name == "mixed":
        return mixed()
    if name == "field-pairs":
        return field_pairs()
    if name == "close-ring":
        return close_ring()
    if parts[0] == "ring":
        return ring(int(parts[1]), int(parts[2][1:]), parts[3])
    if parts[0] == "cascade":
        return dataclasses.replace(cascade(int(parts[1]), parts[2]), name=name)
    if parts[0] == "convoy":
        return convoy(int(parts[1]))
    if parts[0] == "pairs":
        return pairs(int(parts[1]), parts[2])
    if parts[0] == "close":
        return close(int(parts[1]))
    if parts[0] == "field":
        return field_cascade(int(parts[2]))
    raise KeyError(name)


# The `pg` placement's grid: one 208x208 map, blocked except for these cases' maps, each at its origin (x0, y0) with at
# least one blocked row / column between two of them. The regions are not connected, so a case's agents see only
# their own; cases on the same box share a region.
PG_SIDE = 208
PG_ORIGIN = {"ring-64": (0, 0), "ring-66": (19, 0), "ring-62": (39, 0), "ring-10": (58, 0), "ring-4": (64, 0),
             "mixed": (0, 19), "pairs-33": (0, 27), "cascade-65": (0, 34)}
PG_MEMBER = {"ring-64": "ring-64-d1-id", "ring-66": "ring-66-d1-id", "ring-62": "ring-62-d3-id", "ring-10": "ring-10-d1-id",
             "ring-4": "ring-4-d1-id", "mixed": "mixed", "pairs-33": "pairs-33-adj", "cascade-65": "cascade-65-inc"}


# the cases test_gpu_rules.py runs in the pg placement: the rings around the 64-member edge, pairs, mixed, a cascade
PG_CASES = ["ring-4-d1-id", "ring-10-d3-rev", "ring-62-d3-id", "ring-64-d1-id", "ring-64-d3-perm", "ring-66-d3-perm",
            "pairs-33-adj", "pairs-33-split", "mixed", "cascade-65-inc"]


def pg_region(name):
    key = name if name in PG_ORIGIN else "-".join(name.split("-")[:2])
    assert key in PG_ORIGIN and not name.endswith("spread"), name
    return key


@functools.lru_cache(maxsize=None)
def pg_rows():
    blk = _blocked(PG_SIDE, PG_SIDE)
    for key, (x0, y0) in PG_ORIGIN.items():
        b = maps.rows_to_blocked(list(case(PG_MEMBER[key]).rows))
        h, w = b.shape
        assert blk[max(y0 - 1, 0):y0 + h + 1, max(x0 - 1, 0):x0 + w + 1].all(), f"{key} touches another region"
        blk[y0:y0 + h, x0:x0 + w] = b
    return tuple(maps.to_rows(blk))


@functools.lru_cache(maxsize=None)
def embedded(name) -> Case:
    """The case inside pg_rows(): the same state, its cells moved to its region."""
    c = case(name)
    x0, y0 = PG_ORIGIN[pg_region(name)]
    assert c.rows == case(PG_MEMBER[pg_region(name)]).rows
    w = len(c.rows[0])
    re = lambda a: ((a // w + y0) * PG_SIDE + a % w + x0).astype(np.uint32)
    e = dataclasses.replace(c, name=name + "@208", rows=pg_rows(), v=re(c.v), g=re(c.g))
    e.v.setflags(write=False)
    e.g.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _oracle(rows):
    return OracleGraph(maps.rows_to_array(list(rows)))


@functools.lru_cache(maxsize=None)
def _expected(rows, name, embedded_case):
    c = embedded(name) if embedded_case else case(name)
    assert c.rows == rows
    og = _oracle(rows)
    nh = NextHop(og)
    v, g = c.v.copy(), c.g.copy()
    total, per_call, ok = Counters(), [], True
    for _ in range(c.calls):
        rg, C = restate(nh, v, g)
        nv, ng = og.step(v, g)
        ok = ok and np.array_equal(rg, ng)
        per_call.append(C)
        total.add(C)
        v, g = nv, ng
    v.setflags(write=False)
    g.setflags(write=False)
    return dict(v=v, g=g, counters=total, per_call=per_call, restated_ok=ok, moved=int(np.count_nonzero(v != c.v)))


def expected(c: Case):
    """OracleGraph.step applied c.calls times and the restatement beside it: v, g (read-only), counters (summed over
    the calls), per_call, restated_ok (the restatement's goals equalled the oracle's after every call), moved.
    Computed once per case and shared."""
    return _expected(c.rows, c.name.split("@")[0], c.name.endswith("@208"))
