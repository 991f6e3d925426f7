"""The lock-step model of the decentralized run (include/tswap.h, above tsw_fleet_apply) in plain
Python / numpy, shared by test_fleet_run_host.py (CPU) and test_gpu_fleet_run.py (GPU), and the hand-made
apply cases as named inputs. No test in here."""
import functools

import numpy as np

from p2p_distributed_tswap_amd import maps

import fleet_cases as fc

MOVE, SWAP, ROTATION, WAIT = 0, 1, 2, 3
NONE = 0xFFFFFFFF

# (fleet, radius, ticks) of every run comparison
RUN_CASES = [("dense12", 2, 40), ("rand20", 15, 40), ("warehouse", 15, 25)]


def apply_model(v, g, act, cell, partner, part_off, part):
    """The sequential definition: agents take their turns in ascending index; a Move reads the
    tick-start positions, a goal swap exchanges the CURRENT goals of requester and partner, a rotation
    gives participant m the TICK-START goal of participant m + 1. Returns new (v, g)."""
    v0 = np.asarray(v, dtype=np.uint32)
    g0 = np.asarray(g, dtype=np.uint32)
    v1, G = v0.copy(), g0.copy()
    for i in range(v0.size):
        a = int(act[i])
        if a == MOVE:
            v1[i] = cell[i]
        elif a == SWAP:
            j = int(partner[i])
            G[i], G[j] = G[j], G[i]
        elif a == ROTATION:
            P = [int(x) for x in part[int(part_off[i]):int(part_off[i + 1])]]
            for m, a_m in enumerate(P):
                G[a_m] = g0[P[(m + 1) % len(P)]]
    return v1, G


def touched(i, act, partner, part_off, part):
    """The agents whose goal the op of initiator i reads or writes ([] for a Move or a Wait)."""
    if act[i] == SWAP:
        return [i, int(partner[i])]
    if act[i] == ROTATION:
        return [int(x) for x in part[int(part_off[i]):int(part_off[i + 1])]]
    return []


def goal_op_rounds(act, partner, part_off, part):
    """Rounds the claim scheme of tsw_fleet.hip takes for one tick's goal ops: the longest chain of ops
    that share an agent with a smaller-index op (0 without ops)."""
    last = {}  # agent -> round in which the latest op touching it fired
    rounds = 0
    for i in np.flatnonzero((np.asarray(act) == SWAP) | (np.asarray(act) == ROTATION)):
        t = touched(int(i), act, partner, part_off, part)
        r = 1 + max([last.get(a, 0) for a in t], default=0)
        for a in t:
            last[a] = r
        rounds = max(rounds, r)
    return rounds


def goal_op_pending(act, partner, part_off, part):
    """The claim scheme of tsw_fleet.hip round by round: the pending ops (initiators, ascending) at the
    start of every round. An op fires when it is the smallest pending op on every agent it touches; the
    others stay pending, in order. len(result) == goal_op_rounds(...)."""
    act = np.asarray(act)
    cur = [int(i) for i in np.flatnonzero((act == SWAP) | (act == ROTATION))]
    rounds = []
    while cur:
        rounds.append(cur)
        owner = {}
        for i in cur:
            for a in touched(i, act, partner, part_off, part):
                owner[a] = min(owner.get(a, i), i)
        cur = [i for i in cur if any(owner[a] != i for a in touched(i, act, partner, part_off, part))]
    return rounds


def kept_carry_rounds(act, partner, part_off, part, chunk=256):
    """Rounds in which k_fleet_goals' compaction (chunks of `chunk` pending ops, `kept += total` between
    them) places a kept op of a later chunk behind kept ops of an earlier one: kept > 0 at k0 > 0."""
    pend = goal_op_pending(act, partner, part_off, part)
    count = 0
    for cur, nxt in zip(pend, pend[1:]):
        keep = np.isin(cur, nxt)
        count += bool(keep[:chunk].any() and keep[chunk:].any())
    return count


def run_model(og, rows, v, g, radius, ticks):
    """`ticks` ticks of brute_nearby + oracle_fleet + apply_model with the fixed-point stop (a tick that
    changes nothing ends the run and is not counted). Returns (v, g, v_rec, g_rec, ticks_done, decisions):
    records of shape (n, ticks_done + 1), decisions[t] the five arrays tick t applied."""
    W = len(rows[0])
    v = np.asarray(v, dtype=np.uint32).copy()
    g = np.asarray(g, dtype=np.uint32).copy()
    vr, gr, dec = [v.copy()], [g.copy()], []
    for _ in range(ticks):
        off, idx = fc.brute_nearby(v, W, radius)
        d = fc.oracle_fleet(og, v, g, off, idx)
        v1, g1 = apply_model(v, g, *d)
        if np.array_equal(v1, v) and np.array_equal(g1, g):
            break
        v, g = v1, g1
        dec.append(d)
        vr.append(v.copy())
        gr.append(g.copy())
    return v, g, np.stack(vr, axis=1), np.stack(gr, axis=1), len(dec), dec


@functools.lru_cache(maxsize=None)
def long_run_case(ticks=3):
    """The model run of fc.long_rules123() at r = 80 (lists of 1,099 entries), cut where the library must
    stop: the first tick in which an agent's decision goes past Rule 3 (Rotation or Wait) reaches Rule 4
    with a list over the 1,024-entry limit, so that tick fails with TSW_EOVERFLOW and is not applied.
    Returns (v, g, v_rec, g_rec, ticks_done, overflow): the state and the records after ticks_done ticks,
    overflow True when tick number ticks_done is the failing one. Computed once and shared (do not modify)."""
    from oracle import OracleGraph

    rows, v, g, _ = fc.long_rules123()
    og = OracleGraph(maps.rows_to_array(rows))
    v, g = v.copy(), g.copy()
    vr, gr = [v.copy()], [g.copy()]
    overflow = False
    for _ in range(ticks):
        off, idx = fc.brute_nearby(v, len(rows[0]), 80)
        d = fc.oracle_fleet(og, v, g, off, idx)
        if (d[0] >= ROTATION).any():
            overflow = True
            break
        v1, g1 = apply_model(v, g, *d)
        if np.array_equal(v1, v) and np.array_equal(g1, g):
            break
        v, g = v1, g1
        vr.append(v.copy())
        gr.append(g.copy())
    return v, g, np.stack(vr, axis=1), np.stack(gr, axis=1), len(vr) - 1, overflow


@functools.lru_cache(maxsize=None)
def run_case(name):
    """run_model of a RUN_CASES fleet, computed once and shared (do not modify)."""
    from oracle import OracleGraph

    r, ticks = {n: (r, t) for n, r, t in RUN_CASES}[name]
    rows, v, g = fc.fleet_case(name)
    return run_model(OracleGraph(maps.rows_to_array(rows)), rows, v, g, r, ticks)


# ---- hand-made apply cases --------------------------------------------------------------------------

def _case(rows, v, g, ops, moves=()):
    """ops: (initiator, SWAP, partner) or (initiator, ROTATION, [participants]); moves: (agent, cell).
    Everybody else waits. Returns (rows, v, g, act, cell, partner, part_off, part)."""
    v = np.asarray(v, dtype=np.uint32)
    g = np.asarray(g, dtype=np.uint32)
    n = v.size
    act = np.full(n, WAIT, dtype=np.uint32)
    cell = v.copy()
    partner = np.full(n, NONE, dtype=np.uint32)
    lists = [[] for _ in range(n)]
    for i, kind, arg in ops:
        act[i] = kind
        if kind == SWAP:
            partner[i] = arg
        else:
            lists[i] = list(arg)
    for i, c in moves:
        act[i] = MOVE
        cell[i] = c
    part_off = np.zeros(n + 1, dtype=np.uint32)
    part_off[1:] = np.cumsum([len(x) for x in lists])
    part = np.array([a for x in lists for a in x], dtype=np.uint32)
    return rows, v, g, act, cell, partner, part_off, part


@functools.lru_cache(maxsize=None)
def apply_case(name):
    """Named hand-made inputs of fleet_apply. Goals are 100 + index-like distinct cells where it helps
    reading; every cell is on the case's open map."""
    o8 = maps.open_map(8, 8)
    if name == "two_requesters":  # 1 and 2 both swap with 0
        return _case(o8, [0, 1, 2], [10, 11, 12], [(1, SWAP, 0), (2, SWAP, 0)])
    if name == "rotation_3cycle":  # each agent rotates the other two
        return _case(o8, [0, 1, 2], [10, 11, 12],
                     [(0, ROTATION, [1, 2]), (1, ROTATION, [2, 0]), (2, ROTATION, [0, 1])])
    if name == "rotation_then_swap":  # rotation by 0 over {2, 3}, then 1 swaps with 2
        return _case(o8, [0, 1, 2, 3], [10, 11, 12, 13], [(0, ROTATION, [2, 3]), (1, SWAP, 2)])
    if name == "swap_then_rotation":  # the same pair in the other index order
        return _case(o8, [0, 1, 2, 3], [10, 11, 12, 13], [(0, SWAP, 2), (1, ROTATION, [2, 3])])
    if name == "two_moves_one_cell":
        return _case(o8, [0, 2, 20], [7, 7, 20], [], moves=[(0, 1), (1, 1)])
    if name == "chain200":  # 200 agents all swap with agent 0: a dependency chain of 200
        o16 = maps.open_map(16, 16)
        n = 201
        return _case(o16, np.arange(n), np.arange(n)[::-1] + 20, [(i, SWAP, 0) for i in range(1, n)])
    if name == "disjoint1500":  # 1,500 disjoint swaps: more ops than a workgroup has threads
        o64 = maps.open_map(64, 64)
        n = 3000
        return _case(o64, np.arange(n), (np.arange(n) * 7 + 3) % 4096, [(2 * k, SWAP, 2 * k + 1) for k in range(1500)])
    if name == "rotation70":  # more participants than a wave has lanes; initiator 0 outside its list
        o16 = maps.open_map(16, 16)
        n = 80
        order = [int(x) for x in np.random.RandomState(70).permutation(np.arange(1, n))[:70]]
        return _case(o16, np.arange(n), np.arange(n) + 100, [(0, ROTATION, order), (5, SWAP, 6)])
    # more than 256 pending ops that do NOT fire: the compaction of the kept ops crosses its chunks of 256
    if name == "chain300":  # as chain200: round 1 keeps 299 ops, every round all but one
        o32 = maps.open_map(32, 32)
        n = 301
        return _case(o32, np.arange(n), np.arange(n)[::-1] + 20, [(i, SWAP, 0) for i in range(1, n)])
    if name == "pairs800":  # 400 partners with two requesters each: round 1 fires every even op of 800, keeps the odd
        o64 = maps.open_map(64, 64)
        n = 1200
        ops = [(3 * k + d, SWAP, 3 * k + 2) for k in range(400) for d in (0, 1)]
        return _case(o64, np.arange(n), (np.arange(n) * 7 + 3) % 4096, ops)  # 7 is odd: the goals are distinct
    if name == "rotations_kept300":  # 300 rotations {0, 300 + i} by initiator i, all through agent 0; 4 far swaps
        o32 = maps.open_map(32, 32)
        n = 620
        ops = [(i, ROTATION, [0, 300 + i]) for i in range(1, 301)]
        ops += [(604 + 4 * k, SWAP, 606 + 4 * k) for k in range(4)]
        return _case(o32, np.arange(n), (np.arange(n) * 5 + 1) % 1024, ops)
    raise KeyError(name)


APPLY_CASES = ["two_requesters", "rotation_3cycle", "rotation_then_swap", "swap_then_rotation", "two_moves_one_cell",
               "chain200", "disjoint1500", "rotation70", "chain300", "pairs800", "rotations_kept300"]
# the cases above whose kept ops fill more than one chunk of the compaction
KEPT_CASES = ["chain300", "pairs800", "rotations_kept300"]


def single_agent():
    """(rows, v, g): one agent on open_map(6, 6) from cell 0 to cell 35, 10 steps away."""
    return maps.open_map(6, 6), np.array([0], dtype=np.uint32), np.array([35], dtype=np.uint32)
