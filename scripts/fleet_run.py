"""Time per tick of a lock-step decentralized run, two ways, alternating in one process on warm tables:

  (a) what a caller did before tsw_fleet_run, plus the new apply: T ticks of Planner.decide_fleet +
      Planner.fleet_apply, the state going through the host every tick. The decide_fleet calls alone are
      the yardstick (b_decide_fleet of scripts/fleet_tick.py: the parent's per-tick cost with no apply at all);
  (b) one Planner.fleet_run(ticks=T): v | g resident on the device, divided by ticks_done.

Both legs start every repetition from the same (v, g). Before timing, (b)'s final state is checked against
(a)'s. The goal-op rounds per tick (the longest chain of goal ops sharing an agent, what the one-workgroup
claim loop of tsw_fleet.hip iterates) are computed from leg (a)'s decisions. Every timed call ends in a stream
synchronise inside the library; the clock is the host's. Needs a GPU (Planner raises without one).

The share of a tick spent in the apply kernels comes from a kernel trace of leg (b) alone, taken in a run of
its own (the profiler slows the host side, so it is never on while timing):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<instance> -o run -- \\
        python scripts/fleet_run.py --run-only --instances <instance>
    python scripts/fleet_run.py --kernel-stats DIR      # times, then merges each DIR/<instance>'s per-kernel figures

usage: python scripts/fleet_run.py [--ticks 50] [--reps 7] [--radius 15] [--out profiles/r8/fleet_run.json]
"""
import argparse
import csv
import glob
import json
import os
import random
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_distributed_tswap_amd import Planner, build_id, maps  # noqa: E402

INSTANCES = {  # name: (map, agents, seed) — the two instances of scripts/fleet_tick.py
    "warehouse_170x84_1k": (lambda: maps.warehouse_map(170, 84, 0x170084), 1000, 0x170084),
    "wh10k_510x220_10k": (lambda: maps.warehouse_map(510, 220, 0x510220), 10000, 0x510220),
}
APPLY_KERNELS = ("k_fleet_moves", "k_fleet_goals", "k_fleet_record")


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda f: float(np.quantile(a, f))  # noqa: E731
    return {"median_ms": round(q(0.5), 4), "p25_ms": round(q(0.25), 4), "p75_ms": round(q(0.75), 4),
            "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "samples": int(a.size)}


def goal_op_rounds(act, partner, part_off, part):
    """(rounds, ops) of one tick: an op fires one round after the last smaller-index op sharing an agent."""
    last, rounds, ops = {}, 0, 0
    for i in np.flatnonzero((act == 1) | (act == 2)).tolist():
        t = [i, int(partner[i])] if act[i] == 1 else part[part_off[i]:part_off[i + 1]].tolist()
        r = 1 + max((last.get(a, 0) for a in t), default=0)
        for a in t:
            last[a] = r
        rounds, ops = max(rounds, r), ops + 1
    return rounds, ops


def instance(name):
    make, n, seed = INSTANCES[name]
    rows = make()
    W = len(rows[0])
    comp = maps.largest_component(rows)
    rng = random.Random(seed)
    v = np.array([y * W + x for x, y in rng.sample(comp, n)], dtype=np.uint32)
    g = np.array([y * W + x for x, y in (rng.choice(comp) for _ in range(n))], dtype=np.uint32)
    return rows, v, g


def leg_a(p, v, g, ticks, radius, keep=None):
    """T ticks through the host. Returns (v, g, ticks that changed something, decide ms, apply ms per tick)."""
    t_dec, t_app, done = [], [], 0
    for _ in range(ticks):
        t0 = time.perf_counter()
        dec = p.decide_fleet(v, g, radius)
        t1 = time.perf_counter()
        v1, g1 = p.fleet_apply(v, g, *dec)
        t2 = time.perf_counter()
        t_dec.append(1e3 * (t1 - t0))
        t_app.append(1e3 * (t2 - t1))
        if np.array_equal(v1, v) and np.array_equal(g1, g):
            break
        v, g, done = v1, g1, done + 1
        if keep is not None:
            keep.append(dec)
    return v, g, done, t_dec, t_app


def run_instance(name, ticks, reps, radius):
    rows, v, g = instance(name)
    res = {"map": [len(rows[0]), len(rows)], "agents": int(v.size), "radius": radius, "ticks": ticks}
    with Planner(rows) as p:
        # warm tables and buffers, and (b) == (a)
        decs = []
        av, ag, adone, _, _ = leg_a(p, v, g, ticks, radius, decs)
        bv, bg, bdone = p.fleet_run(v, g, ticks, radius)
        assert bdone == adone and np.array_equal(av, bv) and np.array_equal(ag, bg), "fleet_run differs from decide_fleet + fleet_apply"
        res["ticks_done"] = int(bdone)
        ro = [goal_op_rounds(*(d[k] for k in (0, 2, 3, 4))) for d in decs]
        res["goal_op_rounds_per_tick"] = {"max": max(r for r, _ in ro), "mean": round(float(np.mean([r for r, _ in ro])), 3)}
        res["goal_ops_per_tick"] = {"max": max(o for _, o in ro), "mean": round(float(np.mean([o for _, o in ro])), 2)}
        t_dec, t_app, t_a, t_b = [], [], [], []
        for _ in range(reps):  # alternate (a) and (b)
            t0 = time.perf_counter()
            _, _, da, td, ta = leg_a(p, v, g, ticks, radius)
            t_a.append(1e3 * (time.perf_counter() - t0) / max(da, 1))
            t_dec += td
            t_app += ta
            t0 = time.perf_counter()
            _, _, db = p.fleet_run(v, g, ticks, radius)
            t_b.append(1e3 * (time.perf_counter() - t0) / max(db, 1))
    res["a_decide_fleet"] = summary(t_dec)       # per tick: the parent's cost, no apply (the yardstick)
    res["a_fleet_apply"] = summary(t_app)        # per tick: the apply through the host
    res["a_per_tick"] = summary(t_a)             # per repetition: (decide_fleet + fleet_apply + the Python loop) / ticks
    res["b_fleet_run_per_tick"] = summary(t_b)   # per repetition: fleet_run / ticks_done
    y = res["a_decide_fleet"]
    res["yardstick_spread_ms"] = round(y["p75_ms"] - y["p25_ms"], 4)  # interquartile: the margin
    res["run_not_slower_than_decide_fleet_alone"] = bool(
        res["b_fleet_run_per_tick"]["median_ms"] <= y["median_ms"] + res["yardstick_spread_ms"])
    res["speedup_vs_a_per_tick"] = round(res["a_per_tick"]["median_ms"] / res["b_fleet_run_per_tick"]["median_ms"], 2)
    return res


def run_only(names, ticks, reps, radius):
    """Leg (b) alone, for a kernel trace: one warming run, then `reps` runs per instance."""
    for name in names:
        rows, v, g = instance(name)
        with Planner(rows) as p:
            for _ in range(reps + 1):
                done = p.fleet_run(v, g, ticks, radius)[2]
        print(json.dumps({"instance": name, "fleet_run_calls": reps + 1, "ticks_done": int(done)}), flush=True)


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
    per_tick = sum(r["mean_us"] for r in rows if r["kernel"] in APPLY_KERNELS[:2])  # one call of each per tick
    return {"source": "rocprofv3 --kernel-trace --stats over `fleet_run.py --run-only --instances <this one>`, a run of "
            "its own (its first fleet_run also builds the tables: compare per call, not totals)",
            "apply_kernels_us_per_tick": round(per_tick, 2),
            "note": "the apply also takes one of the four exclusive scans of a tick (k_scan_*), not separable by name",
            "kernels": sorted(rows, key=lambda r: -r["total_us"])[:16]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=int, default=15)
    ap.add_argument("--instances", nargs="*", default=list(INSTANCES))
    ap.add_argument("--run-only", action="store_true", help="leg (b) alone, nothing written: the kernel-trace run")
    ap.add_argument("--kernel-stats", help="directory holding one kernel-trace output directory per instance, to merge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "fleet_run.json"))
    a = ap.parse_args()
    if a.run_only:
        return run_only(a.instances, a.ticks, min(a.reps, 3), a.radius)
    out = {"build_id": build_id(), "method": "host clock around calls that end in a stream synchronise; legs (a) and (b) "
           "alternate repetition by repetition in one process on warm tables, each from the same (v, g); "
           "spread = interquartile range", "instances": {}}
    for name in a.instances:
        out["instances"][name] = run_instance(name, a.ticks, a.reps, a.radius)
        print(name, json.dumps(out["instances"][name]), flush=True)
        if a.kernel_stats:  # DIR/<instance>/: that instance's kernel trace
            kt = kernel_stats(os.path.join(a.kernel_stats, name))
            kt["apply_share_of_tick"] = round(kt["apply_kernels_us_per_tick"] / (1e3 * out["instances"][name]["b_fleet_run_per_tick"]["median_ms"]), 4)
            out["instances"][name]["kernel_trace"] = kt
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"fleet_run": a.out, "build_id": out["build_id"]}), flush=True)


if __name__ == "__main__":
    main()
