"""Time per step of a decentralized MAPD run, two ways, alternating in one process on warm tables:

  (a) the yardstick — what a caller did before tsw_fleet_mapd, from entry points the library already had:
      per step the task phase in numpy on the host and Planner.fleet_run(ticks=1), the state going
      through the host every step;
  (b) one Planner.fleet_mapd call: state, task phase, tick and records resident on the device, divided by
      the columns it recorded.

Both legs run the same instance from its start. Before timing, (b)'s records, goals and tasks are checked
against (a)'s (that pass also packs (a)'s records; the timed (a) does not, which favours (a)). Every timed
call ends in a stream synchronise inside the library; the clock is the host's. Needs a GPU.

Reported per instance besides the times: tasks handed out, deliveries, whether the run stalled, and
co-locations (agents beyond the first on a cell, summed over the recorded columns).

The share of a step spent in the task and record kernels comes from a kernel trace of leg (b) alone, taken
in a run of its own (the profiler slows the host side, so it is never on while timing):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<instance> -o run -- \\
        python scripts/fleet_mapd.py --run-only --instances <instance>
    python scripts/fleet_mapd.py --kernel-stats DIR     # times, then merges each DIR/<instance>'s per-kernel figures

usage: python scripts/fleet_mapd.py [--max-t 200] [--reps 7] [--radius 15] [--out profiles/r11/fleet_mapd.json]
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_distributed_tswap_amd import Planner, build_id, maps  # noqa: E402

INSTANCES = {  # name: (map, agents, tasks, seed): well-formed streams that outlast the horizon
    "warehouse_170x84_1k": (lambda: maps.warehouse_map(170, 84, 0x170084), 1000, 2000, 0x170084),
    "wh10k_510x220_10k": (lambda: maps.warehouse_map(510, 220, 0x510220), 10000, 20000, 0x510220),
}
MAPD_KERNELS = ("k_mapd_arrive", "k_mapd_assign", "k_mapd_record")
IDLE, TO_PICKUP, TO_DELIVERY, NONE = 0, 1, 2, 0xFFFFFFFF


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda f: float(np.quantile(a, f))  # noqa: E731
    return {"median_ms": round(q(0.5), 4), "p25_ms": round(q(0.25), 4), "p75_ms": round(q(0.75), 4),
            "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "samples": int(a.size)}


def instance(name):
    make, n, m, seed = INSTANCES[name]
    rows = make()
    starts, tasks = maps.make_wf_instance(rows, n, m, seed)
    return rows, starts, tasks


def cells(xy, W):
    return (xy[:, 1] * np.uint32(W) + xy[:, 0]).astype(np.uint32)


def task_phase(v, g, st, tk, nxt, pick, dlv):
    """Stage 1 of the model (include/tswap.h, above tsw_fleet_mapd) in numpy, in place: the arrival
    transitions, then task next + rank for the idle agent of that rank while next + rank < m.
    Returns (next, changed, deliveries)."""
    at = v == g
    to_dlv = at & (st == TO_PICKUP)
    to_idle = at & (st == TO_DELIVERY)
    g[to_dlv] = dlv[tk[to_dlv]]
    st[to_dlv] = TO_DELIVERY
    st[to_idle] = IDLE
    tk[to_idle] = NONE
    idle = st == IDLE
    rank = np.cumsum(idle) - idle
    take = idle & (nxt + rank < pick.size)
    k = (nxt + rank[take]).astype(np.uint32)
    tk[take] = k
    st[take] = TO_PICKUP
    g[take] = pick[k]
    return (min(pick.size, nxt + int(idle.sum())), bool(to_dlv.any() or to_idle.any() or take.any()),
            int(to_idle.sum()))


def pack(v, g, st, W):
    state = np.where(st == IDLE, 3, np.where(st == TO_PICKUP, 0, np.where(v == g, 2, 1))).astype(np.uint64)
    v = v.astype(np.uint64)
    return (v % np.uint64(W)) | ((v // np.uint64(W)) << np.uint64(16)) | (state << np.uint64(32))


def leg_a(p, W, starts, pick, dlv, radius, max_t, keep=None):
    """The run through the host. Returns (columns, stalled, next, deliveries)."""
    v = cells(starts, W)
    g = v.copy()
    st, tk = np.zeros(v.size, dtype=np.uint32), np.full(v.size, NONE, dtype=np.uint32)
    nxt = cols = delivered = 0
    while True:
        nxt, tchanged, d = task_phase(v, g, st, tk, nxt, pick, dlv)
        delivered += d
        v, g, ticked = p.fleet_run(v, g, 1, radius)
        done = nxt == pick.size and not st.any()
        if not done and not tchanged and not ticked:
            return cols, True, nxt, delivered
        if keep is not None:
            keep.append((pack(v, g, st, W), g.copy(), tk.copy()))
        cols += 1
        if done or cols > max_t:
            return cols, False, nxt, delivered


def run_instance(name, max_t, reps, radius):
    rows, starts, tasks = instance(name)
    W = len(rows[0])
    pick, dlv = cells(tasks[:, :2], W), cells(tasks[:, 2:], W)
    res = {"map": [W, len(rows)], "agents": int(starts.shape[0]), "tasks": int(tasks.shape[0]), "radius": radius,
           "max_t": max_t}
    with Planner(rows) as p:
        # warm tables and buffers ((b) first: it builds every table of the run), and (b) == (a)
        rec, goals, tks, stalled = p.fleet_mapd(starts, tasks, max_t, radius, trace=True)
        keep = []
        cols, a_stalled, nxt, delivered = leg_a(p, W, starts, pick, dlv, radius, max_t, keep)
        assert cols == rec.shape[1] and a_stalled == stalled, "fleet_mapd ends differently from the host loop"
        for k, got in enumerate((rec, goals, tks)):
            assert np.array_equal(got, np.stack([c[k] for c in keep], axis=1)), "fleet_mapd differs from the host loop"
        assert nxt < tasks.shape[0] or stalled, "the task stream did not outlast the horizon"
        cell = rec & np.uint64(0xFFFFFFFF)
        res.update(columns=int(cols), stalled=bool(stalled), tasks_handed_out=int(nxt), deliveries=int(delivered),
                   colocations=int(sum(cell.shape[0] - np.unique(cell[:, t]).size for t in range(cell.shape[1]))))
        t_a, t_b = [], []
        for _ in range(reps):  # alternate (a) and (b)
            t0 = time.perf_counter()
            ca = leg_a(p, W, starts, pick, dlv, radius, max_t)[0]
            t_a.append(1e3 * (time.perf_counter() - t0) / max(ca, 1))
            t0 = time.perf_counter()
            rb, _ = p.fleet_mapd(starts, tasks, max_t, radius)
            t_b.append(1e3 * (time.perf_counter() - t0) / max(rb.shape[1], 1))
    res["a_host_loop_per_step"] = summary(t_a)   # per repetition: (numpy task phase + fleet_run(ticks=1)) per column
    res["b_fleet_mapd_per_step"] = summary(t_b)  # per repetition: fleet_mapd / columns
    y = res["a_host_loop_per_step"]
    res["yardstick_spread_ms"] = round(y["p75_ms"] - y["p25_ms"], 4)  # interquartile: the margin
    res["mapd_not_slower_than_host_loop"] = bool(
        res["b_fleet_mapd_per_step"]["median_ms"] <= y["median_ms"] + res["yardstick_spread_ms"])
    res["speedup_vs_a"] = round(y["median_ms"] / res["b_fleet_mapd_per_step"]["median_ms"], 2)
    return res


def run_only(names, max_t, reps, radius):
    """Leg (b) alone, for a kernel trace: one warming run, then `reps` runs per instance."""
    for name in names:
        rows, starts, tasks = instance(name)
        with Planner(rows) as p:
            for _ in range(reps + 1):
                rec, stalled = p.fleet_mapd(starts, tasks, max_t, radius)
        print(json.dumps({"instance": name, "fleet_mapd_calls": reps + 1, "columns": int(rec.shape[1])}), flush=True)


def kernel_stats(path):
    """Per-kernel totals of a rocprofv3 --kernel-trace --stats run (its *kernel_stats.csv, found under path)."""
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {path}")
    rows = []
    with open(files[0], newline="") as fh:
        for r in csv.DictReader(fh):
            m = re.match(r"(?:void )?([\w:]+)", r["Name"].replace("(anonymous namespace)::", ""))
            rows.append({"kernel": m.group(1).split("::")[-1] if m else r["Name"], "calls": int(r["Calls"]),
                         "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1), "mean_us": round(float(r["AverageNs"]) / 1e3, 2)})
    rows.sort(key=lambda r: -r["total_us"])
    found = [r for r in rows if r["kernel"] in MAPD_KERNELS]
    return {"source": "rocprofv3 --kernel-trace --stats over `fleet_mapd.py --run-only --instances <this one>`, a run of "
            "its own (its first fleet_mapd also builds the tables: compare per call, not totals)",
            "mapd_kernels_us_per_step": round(sum(r["mean_us"] for r in found), 2),  # one call of each per step
            "mapd_kernels_found": [r["kernel"] for r in found],
            "note": "the task phase also takes one of the five exclusive scans of a step (k_scan_*), not separable by name",
            "mapd_kernels": found, "kernels": rows[:16]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-t", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=int, default=15)
    ap.add_argument("--instances", nargs="*", default=list(INSTANCES))
    ap.add_argument("--run-only", action="store_true", help="leg (b) alone, nothing written: the kernel-trace run")
    ap.add_argument("--kernel-stats", help="directory holding one kernel-trace output directory per instance, to merge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "fleet_mapd.json"))
    a = ap.parse_args()
    if a.run_only:
        return run_only(a.instances, a.max_t, min(a.reps, 3), a.radius)
    out = {"build_id": build_id(), "method": "host clock around calls that end in a stream synchronise; legs (a) and (b) "
           "alternate repetition by repetition in one process on warm tables, each from the instance's start; "
           "per step = a repetition's time / its recorded columns; spread = interquartile range", "instances": {}}
    for name in a.instances:
        out["instances"][name] = run_instance(name, a.max_t, a.reps, a.radius)
        print(name, json.dumps(out["instances"][name]), flush=True)
        if a.kernel_stats:  # DIR/<instance>/: that instance's kernel trace
            kt = kernel_stats(os.path.join(a.kernel_stats, name))
            kt["mapd_kernels_share_of_step"] = round(
                kt["mapd_kernels_us_per_step"] / (1e3 * out["instances"][name]["b_fleet_mapd_per_step"]["median_ms"]), 4)
            out["instances"][name]["kernel_trace"] = kt
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"fleet_mapd": a.out, "build_id": out["build_id"]}), flush=True)


if __name__ == "__main__":
    main()
