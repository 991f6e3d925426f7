"""CPU model of tsw_plan_mapd_online (include/tswap.h): the reference's tswap_mapd loop (tswap.rs:39-172) with a
release time per task, in Python. tswap_step is the oracle's (OracleGraph.step); the assignment is a plain
first-minimum scan over the visible unused tasks. Test infrastructure only.

online_mapd returns (rec (n, T) uint64 = x | y << 16 | state << 32, goals (n, T) uint32, T, counters) with

  counters["segments"]        1 + the distinct release times in (0, max_t]: the stretches of the run between
                              two releases, what the library runs as one k_plan segment each
  counters["held"]            columns produced with no visible unused task and every agent idle on its goal
                              (nothing can move: the column repeats the one before)
  counters["idle_walking"]    columns produced with no visible unused task and every agent idle, but some agent
                              off its goal (a goal swap sent a resting agent elsewhere): the fleet still moves
  counters["never_released"]  tasks with release > max_t

A task cell that the reference would look up (pos2id[..], :112 / :136) and that is off the grid or blocked raises
ValueError there, as the reference panics.
"""
from __future__ import annotations

import numpy as np

from oracle import OracleGraph

IDLE, TO_PICKUP, TO_DELIVERY = 0, 1, 2
PICKING, CARRYING, DELIVERED, ST_IDLE = 0, 1, 2, 3  # AgentState (src/map/agent.rs:9-15)


def online_mapd(cells: np.ndarray, starts_xy, tasks_xyxy, release, max_t: int = 2000, graph: OracleGraph = None):
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    h, w = cells.shape
    graph = graph or OracleGraph(cells)
    starts = np.asarray(starts_xy, dtype=np.int64).reshape(-1, 2)
    tasks = np.asarray(tasks_xyxy, dtype=np.int64).reshape(-1, 4)
    n, m = len(starts), len(tasks)
    rel = np.zeros(m, dtype=np.int64) if release is None else np.asarray(release, dtype=np.int64).reshape(-1)
    assert rel.size == m

    def cell_of(x, y):
        if not (0 <= x < w and 0 <= y < h) or cells[y, x] == ord("@"):
            raise ValueError(f"task cell ({x}, {y}) off-grid or blocked (reference would panic)")
        return int(y * w + x)

    v = np.array([cell_of(int(x), int(y)) for x, y in starts], dtype=np.uint32)
    g = v.copy()
    state = [IDLE] * n
    task = [-1] * n
    used = np.zeros(m, dtype=bool)
    rec = np.zeros((max(n, 1), max_t + 1), dtype=np.uint64)
    goals = np.zeros((max(n, 1), max_t + 1), dtype=np.uint32)
    held = walking = 0
    t = 0
    while True:
        visible = (~used) & (rel <= t)  # updated as tasks are taken below
        if t >= 1 and not visible.any() and all(s == IDLE for s in state):
            if np.array_equal(v, g):
                held += 1
            else:
                walking += 1
        for i in range(n):
            if v[i] == g[i]:
                if state[i] == TO_PICKUP:
                    state[i] = TO_DELIVERY
                    if task[i] >= 0:
                        g[i] = cell_of(int(tasks[task[i], 2]), int(tasks[task[i], 3]))
                elif state[i] == TO_DELIVERY:
                    state[i] = IDLE
                    task[i] = -1
            if state[i] == IDLE and visible.any():
                x, y = int(v[i]) % w, int(v[i]) // w
                ks = np.nonzero(visible)[0]
                d = np.abs(tasks[ks, 0] - x) + np.abs(tasks[ks, 1] - y)
                k = int(ks[int(np.argmin(d))])  # first minimum: the lowest task index on ties
                used[k] = True
                visible[k] = False
                task[i] = k
                state[i] = TO_PICKUP
                g[i] = cell_of(int(tasks[k, 0]), int(tasks[k, 1]))
        if n:
            v, g = graph.step(v, g)
        for i in range(n):
            s = ST_IDLE if state[i] == IDLE else PICKING if state[i] == TO_PICKUP else (DELIVERED if v[i] == g[i] else CARRYING)
            rec[i, t] = int(v[i]) % w | (int(v[i]) // w) << 16 | s << 32
            goals[i, t] = g[i]
        t += 1
        if (used.all() and all(s == IDLE for s in state)) or t > max_t:
            break
    counters = {
        "segments": 1 + len({int(r) for r in rel if 0 < r <= max_t}),
        "held": held,
        "idle_walking": walking,
        "never_released": int(np.count_nonzero(rel > max_t)),
    }
    return rec[:n, :t], goals[:n, :t], t, counters
