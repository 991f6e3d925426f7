"""The decentralized MAPD run (include/tswap.h, above tsw_fleet_mapd) in plain Python / numpy, shared by
test_fleet_mapd_host.py (CPU) and test_gpu_fleet_mapd.py (GPU): the task phase as the sequential loop of
the header, its scan form (what the kernels compute), the run built from fleet_cases.brute_nearby,
fleet_cases.oracle_fleet and fleet_run_model.apply_model, and the named cases. No test in here."""
import functools
from collections import namedtuple

import numpy as np

from p2p_distributed_tswap_amd import maps

import fleet_cases as fc
import fleet_run_model as fm

IDLE, TO_PICKUP, TO_DELIVERY = 0, 1, 2
NONE = 0xFFFFFFFF
# AgentState discriminants (include/tswap.h TSW_PICKING .. TSW_IDLE)
PICKING, CARRYING, DELIVERED, REC_IDLE = 0, 1, 2, 3

Run = namedtuple("Run", "rec goals tasks T stalled next delivered colocated")


def task_phase(v, g, st, tk, nxt, pick, dlv):
    """Stage 1 as the header states it: agents in ascending index, arrival transition first, then the
    dispatch of the next task of the stream. g, st, tk are updated in place. Returns (next, changed,
    delivered): changed = a transition was made, delivered = TO_DELIVERY -> IDLE transitions."""
    m = len(pick)
    changed, delivered = False, 0
    for i in range(len(v)):
        if v[i] == g[i]:
            if st[i] == TO_PICKUP:
                st[i] = TO_DELIVERY
                g[i] = dlv[tk[i]]
                changed = True
            elif st[i] == TO_DELIVERY:
                st[i] = IDLE
                tk[i] = NONE
                changed = True
                delivered += 1
        if st[i] == IDLE and nxt < m:
            tk[i] = nxt
            st[i] = TO_PICKUP
            g[i] = pick[nxt]
            nxt += 1
            changed = True
    return nxt, changed, delivered


def task_phase_scan(v, g, st, tk, nxt, pick, dlv):
    """The same stage in the form the kernels compute it: the arrival transitions of all agents, an
    exclusive prefix count of the agents idle after them, and task next + rank for every idle agent with
    next + rank < m. In place; returns (next, changed)."""
    m = len(pick)
    at = v == g
    to_dlv = at & (st == TO_PICKUP)
    to_idle = at & (st == TO_DELIVERY)
    g[to_dlv] = dlv[tk[to_dlv]]
    st[to_dlv] = TO_DELIVERY
    st[to_idle] = IDLE
    tk[to_idle] = NONE
    idle = st == IDLE
    rank = np.cumsum(idle) - idle  # exclusive
    take = idle & (nxt + rank < m)
    k = (nxt + rank[take]).astype(np.uint32)
    tk[take] = k
    st[take] = TO_PICKUP
    g[take] = pick[k]
    changed = bool(to_dlv.any() or to_idle.any() or take.any())
    return min(m, nxt + int(idle.sum())), changed


def pack(v, g, st, W):
    """Column of records: x | y << 16 | state << 32 (plan_mapd_arrays' packing of tsw_rec)."""
    state = np.where(st == IDLE, REC_IDLE, np.where(st == TO_PICKUP, PICKING, np.where(v == g, DELIVERED, CARRYING)))
    v = v.astype(np.uint64)
    return (v % np.uint64(W)) | ((v // np.uint64(W)) << np.uint64(16)) | (state.astype(np.uint64) << np.uint64(32))


def cells_of(xy, W):
    xy = np.asarray(xy, dtype=np.uint32).reshape(-1, 2)
    return (xy[:, 1] * np.uint32(W) + xy[:, 0]).astype(np.uint32)


def run_model(og, rows, starts_xy, tasks_xyxy, radius, max_t):
    """The run of the header, stage by stage. Returns a Run: rec (n, T) uint64, goals / tasks (n, T)
    uint32, T, stalled, and for the reports next (tasks handed out), delivered, colocated (agents beyond
    the first on a cell, summed over the recorded columns)."""
    W = len(rows[0])
    tasks_xyxy = np.asarray(tasks_xyxy, dtype=np.uint32).reshape(-1, 4)
    pick, dlv = cells_of(tasks_xyxy[:, :2], W), cells_of(tasks_xyxy[:, 2:], W)
    v = cells_of(starts_xy, W)
    g = v.copy()
    n, m = v.size, pick.size
    if n == 0:  # the entry point's own rule: nothing to run
        e = np.zeros((0, 0), dtype=np.uint32)
        return Run(e.astype(np.uint64), e, e, 0, False, 0, 0, 0)
    st = np.zeros(n, dtype=np.uint32)
    tk = np.full(n, NONE, dtype=np.uint32)
    nxt = delivered = colocated = 0
    rec, goals, tks = [], [], []
    stalled = False
    while True:
        nxt, tchanged, d = task_phase(v, g, st, tk, nxt, pick, dlv)
        delivered += d
        off, idx = fc.brute_nearby(v, W, radius)
        v1, g1 = fm.apply_model(v, g, *fc.oracle_fleet(og, v, g, off, idx))
        unchanged = not tchanged and np.array_equal(v1, v) and np.array_equal(g1, g)
        v, g = v1, g1
        done = nxt == m and bool(np.all(st == IDLE))
        if not done and unchanged:
            stalled = True
            break
        rec.append(pack(v, g, st, W))
        goals.append(g.copy())
        tks.append(tk.copy())
        colocated += n - np.unique(v).size
        if done or len(rec) > max_t:
            break
    def stack(cols, dt):
        return np.stack(cols, axis=1) if cols else np.zeros((n, 0), dtype=dt)

    return Run(stack(rec, np.uint64), stack(goals, np.uint32), stack(tks, np.uint32), len(rec), stalled, nxt,
               delivered, int(colocated))


# ---- named cases ------------------------------------------------------------------------------------

# name -> (instance, radius, max_t, ending); ending: "normal" (every task delivered), "stalled", "horizon"
def _open8():
    rows = maps.open_map(8, 8)
    return (rows, *maps.make_instance(rows, 6, 12, 1))


def _tasks(*t):
    return np.array(t, dtype=np.uint32).reshape(-1, 4)


def _starts(*s):
    return np.array(s, dtype=np.uint32).reshape(-1, 2)


_INSTANCES = {
    "single": lambda: (maps.open_map(6, 6), *maps.make_instance(maps.open_map(6, 6), 1, 3, 2)),
    "open8": _open8,
    "open8-r2": _open8,
    "open8-wf": lambda: (maps.open_map(8, 8), *maps.make_wf_instance(maps.open_map(8, 8), 6, 12, 1)),
    "rand20": lambda: (lambda rows: (rows, *maps.make_instance(rows, 40, 120, 3)))(maps.random_map(20, 16, 0.2, 5)),
    "dense12": lambda: (lambda rows: (rows, *maps.make_wf_instance(rows, 50, 100, 4)))(maps.random_map(12, 12, 0.15, 9)),
    "warehouse": lambda: (lambda rows: (rows, *maps.make_wf_instance(rows, 300, 600, 5)))(
        maps.warehouse_map(170, 84, 0x170084)),
    "dispatch3000": lambda: (maps.open_map(64, 64), *maps.make_instance(maps.open_map(64, 64), 3000, 2000, 7)),
    # hand-made endings, all on open_map(6, 6)
    "no-tasks": lambda: (maps.open_map(6, 6), _starts((0, 0), (3, 2)), _tasks()),
    "max_t-0": lambda: (maps.open_map(6, 6), _starts((0, 0), (3, 2)), _tasks((5, 5, 0, 5), (1, 1, 4, 4))),
    "pickup-is-delivery": lambda: (maps.open_map(6, 6), _starts((0, 0)), _tasks((2, 1, 2, 1), (4, 4, 0, 3))),
    "pickup-on-start": lambda: (maps.open_map(6, 6), _starts((1, 1), (4, 0)), _tasks((1, 1, 3, 3), (5, 5, 4, 0))),
    "fewer-tasks": lambda: (maps.open_map(6, 6), _starts((0, 0), (5, 0), (0, 5), (5, 5)), _tasks((2, 2, 3, 3), (3, 2, 1, 4))),
}

CASES = {
    "single": (15, 100, "normal"),
    "open8": (15, 200, "normal"),
    "open8-r2": (2, 200, "normal"),
    "open8-wf": (15, 200, "normal"),
    "rand20": (15, 300, "stalled"),
    "dense12": (2, 200, "stalled"),
    "warehouse": (15, 60, "horizon"),
    "dispatch3000": (1, 2, "horizon"),
}
HAND_CASES = {
    "no-tasks": (15, 50, "normal"),
    "max_t-0": (15, 0, "horizon"),
    "pickup-is-delivery": (15, 50, "normal"),
    "pickup-on-start": (15, 50, "normal"),
    "fewer-tasks": (15, 50, "normal"),
}


@functools.lru_cache(maxsize=None)
def instance(name):
    """(rows, starts (n,2), tasks (m,4), radius, max_t, ending) of a named case (do not modify)."""
    rows, starts, tasks = _INSTANCES[name]()
    return (rows, starts, tasks, *{**CASES, **HAND_CASES}[name])


@functools.lru_cache(maxsize=None)
def run_case(name):
    """run_model of a named case, computed once per process and shared (do not modify)."""
    from oracle import OracleGraph

    rows, starts, tasks, r, max_t, _ = instance(name)
    return run_model(OracleGraph(maps.rows_to_array(rows)), rows, starts, tasks, r, max_t)


def ending(run, max_t):
    """How a run ended, in the words of the CASES table."""
    if run.stalled:
        return "stalled"
    return "horizon" if run.T == max_t + 1 and not _all_idle_last(run) else "normal"


def _all_idle_last(run):
    return run.T > 0 and bool(np.all((run.rec[:, -1] >> np.uint64(32)) == REC_IDLE)) and bool(np.all(run.tasks[:, -1] == NONE))
