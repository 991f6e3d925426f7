#!/usr/bin/env python3
"""What tsw_plan_mapd_online costs on C3 (170x84 warehouse, 1,000 agents, the 32,000-task stream, max_t 2000).

Four legs in one process on one context, alternating, RUNS times each (median and interquartile range):

  a  plan_mapd_arrays                              the whole stream at t = 0 (the parent's path)
  b  plan_mapd_online, release = 0                 the same plan through the segment runner: one segment
  c  plan_mapd_online, 16 tasks released per step  ~2,000 segments
  d  the per-tick loop that c replaces             Planner.step per tick, the task phase in numpy on the host

c and d must give the same records. Reported per leg: ms per call and per step, walker_launches and the section
breakdown of tsw_get_stats; for c the cost of a segment boundary, (c - b) / (segments - 1), which is an upper bound
(the paced plan is also a different plan: fewer tasks to scan per step, other traffic).

  python scripts/online_plan.py [--runs 5] [--out profiles/r18/online.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_distributed_tswap_amd import Planner, build_id, maps  # noqa: E402

MAX_T = 2000
PER_STEP = 16


def tick_loop(p, w, starts, tasks, rel, max_t):
    """tsw_plan_mapd_online's model with Planner.step for tswap_step: what a caller had to write before."""
    n, m = len(starts), len(tasks)
    v = (starts[:, 1].astype(np.int64) * w + starts[:, 0]).astype(np.uint32)
    g = v.copy()
    pick = (tasks[:, 1].astype(np.int64) * w + tasks[:, 0]).astype(np.uint32)
    dlv = (tasks[:, 3].astype(np.int64) * w + tasks[:, 2]).astype(np.uint32)
    px, py = tasks[:, 0].astype(np.int64), tasks[:, 1].astype(np.int64)
    order = np.argsort(rel, kind="stable")
    state = np.zeros(n, dtype=np.int8)  # 0 idle, 1 to pickup, 2 to delivery
    task = np.full(n, -1, dtype=np.int64)
    used = np.zeros(m, dtype=bool)
    rec = np.zeros((n, max_t + 1), dtype=np.uint64)
    nrel = 0
    vis = np.zeros(m, dtype=bool)  # released and unused
    t = 0
    while True:
        while nrel < m and rel[order[nrel]] <= t:
            vis[order[nrel]] = True
            nrel += 1
        at = v == g
        tp = at & (state == 1)
        td = at & (state == 2)
        state[tp] = 2
        g[tp] = dlv[task[tp]]
        state[td] = 0
        task[td] = -1
        for i in np.nonzero(state == 0)[0]:  # index order: an agent's choice removes the task for the next
            ks = np.nonzero(vis)[0]
            if ks.size == 0:
                break
            x, y = int(v[i]) % w, int(v[i]) // w
            k = int(ks[int(np.argmin(np.abs(px[ks] - x) + np.abs(py[ks] - y)))])
            vis[k] = False
            used[k] = True
            task[i] = k
            state[i] = 1
            g[i] = pick[k]
        v, g = p.step(v, g)
        s = np.where(state == 0, 3, np.where(state == 1, 0, np.where(v == g, 2, 1))).astype(np.uint64)
        rec[:, t] = (v % w).astype(np.uint64) | ((v // w).astype(np.uint64) << np.uint64(16)) | (s << np.uint64(32))
        t += 1
        if (used.all() and (state == 0).all()) or t > max_t:
            break
    return rec[:, :t]


def summary(xs):
    q1, med, q3 = (float(x) for x in np.percentile(xs, [25, 50, 75]))
    return {"median_ms": med, "iqr_ms": [q1, q3], "runs_ms": [float(x) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "online.json"))
    ap.add_argument("--skip-d", action="store_true", help="leave the per-tick loop out (it takes the longest)")
    a = ap.parse_args()
    rows, starts, tasks = maps.config_instance("c3_warehouse_170x84")
    w = len(rows[0])
    m = len(tasks)
    rel0 = np.zeros(m, dtype=np.uint32)
    relp = (np.arange(m) // PER_STEP).astype(np.uint32)
    segments = 1 + len({int(r) for r in relp if 0 < r <= MAX_T})
    legs = {
        "a": lambda p: p.plan_mapd_arrays(starts, tasks, MAX_T)[0],
        "b": lambda p: p.plan_mapd_online(starts, tasks, rel0, MAX_T)[0],
        "c": lambda p: p.plan_mapd_online(starts, tasks, relp, MAX_T)[0],
        "d": lambda p: tick_loop(p, w, starts, tasks, relp, MAX_T),
    }
    if a.skip_d:
        del legs["d"]
    times = {k: [] for k in legs}
    stats, recs = {}, {}
    with Planner(rows) as p:
        for k, f in legs.items():  # warm: tables and next hops of every leg's goals
            recs[k] = f(p)
        for _ in range(a.runs):
            for k, f in legs.items():
                p.reset_stats()
                t0 = time.perf_counter()
                r = f(p)
                times[k].append((time.perf_counter() - t0) * 1e3)
                st = p.stats()
                stats[k] = {q: st[q] for q in ("walker_launches", "astar_launches", "plan_section_ms", "plan_exits",
                                               "coop_waits", "coop_wait_ms", "rule_rounds", "move_rounds", "steps")}
                assert np.array_equal(r, recs[k]), f"leg {k}: a repeated call gave another plan"
    out = {"config": "c3_warehouse_170x84", "agents": len(starts), "tasks": m, "max_t": MAX_T, "runs": a.runs,
           "released_per_step": PER_STEP, "build_id": build_id(), "legs": {}}
    for k in legs:
        T = int(recs[k].shape[1])
        s = summary(times[k])
        out["legs"][k] = {**s, "columns": T, "ms_per_step": s["median_ms"] / T, **stats[k]}
    out["a_equals_b"] = bool(np.array_equal(recs["a"], recs["b"]))
    if "d" in legs:
        out["c_equals_d"] = bool(np.array_equal(recs["c"], recs["d"]))
    out["c_segments"] = segments
    out["c_launches_per_segment"] = out["legs"]["c"]["walker_launches"] / segments
    out["c_boundary_ms_upper_bound"] = (out["legs"]["c"]["median_ms"] - out["legs"]["b"]["median_ms"]) / (segments - 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if k != "legs" else {q: {x: l[x] for x in ("median_ms", "iqr_ms", "columns", "ms_per_step",
                                                                       "walker_launches")} for q, l in v.items()})
                      for k, v in out.items()}, indent=1))
    assert out["a_equals_b"], "release = 0 must give plan_mapd_arrays' plan"
    if "d" in legs:
        assert out["c_equals_d"], "the paced online plan must equal the per-tick loop's"


if __name__ == "__main__":
    main()
