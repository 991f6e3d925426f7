#!/usr/bin/env python3
"""What tsw_astar_reserved costs, against its host twin on the same inputs.

Workload: the 170x84 warehouse (C3's map), K queries between random free cells (K = 1,000 and 10,000, start_time
0), reservations taken from a real plan of C3: every record of plan_mapd_arrays is a reserved vertex (cell, t) and
every move a reserved edge ((from, to), t); max_time = 2 * (w + h), max_nodes the default 65,536.

Legs, alternating in one process after a warm-up of both (median and interquartile range over RUNS):

  device  Planner.astar_reserved, wall ms of the whole call, and from tsw_probe_st_astar the reservation set's
          build and upload, the search kernel (HIP events) and the path packing
  host    host_astar_reserved on one core, wall ms (at most HOST_RUNS times: it is the slow leg)

The two must return the same paths, status and pops. Clocks per pop: the search kernel's time times the waves that
ran at once times the device clock, over the pops of the call — what one wave spends per pop while the others hide
its latency — next to the throughput figure (kernel ns per pop over all waves).

  python scripts/st_astar.py [--runs 5] [--out profiles/r21/st_astar.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_distributed_tswap_amd import (TSW_SP_CAPACITY, TSW_SP_FOUND, TSW_SP_NONE, Planner, build_id,  # noqa: E402
                                       host_astar_reserved, maps)

MAX_T = 2000
HOST_RUNS = 3
CLOCK_MHZ = 2400.0  # MI355X peak engine clock: the per-pop clocks below are an upper bound at lower clocks


def summary(xs):
    q1, med, q3 = (float(x) for x in np.percentile(xs, [25, 50, 75]))
    return {"median_ms": med, "iqr_ms": [q1, q3], "runs_ms": [float(x) for x in xs]}


def timed(f):
    t0 = time.perf_counter()
    r = f()  # every call returns after its device work
    return r, (time.perf_counter() - t0) * 1e3


def reservations(rec, w):
    """Every record a reserved vertex, every move a reserved edge, at the record's column."""
    x = (rec & np.uint64(0xFFFF)).astype(np.uint32)
    y = ((rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint32)
    cell = y * np.uint32(w) + x
    t = np.broadcast_to(np.arange(rec.shape[1], dtype=np.uint32), cell.shape)
    node = np.stack([cell.reshape(-1), t.reshape(-1)], axis=1)
    moved = cell[:, 1:] != cell[:, :-1]
    edge = np.stack([cell[:, :-1][moved], cell[:, 1:][moved], t[:, 1:][moved]], axis=1)
    return np.ascontiguousarray(node), np.ascontiguousarray(edge)


def measure(p, rows, k, node, edge, max_time, runs, seed):
    free = np.nonzero(maps.rows_to_array(rows).reshape(-1) != ord("@"))[0].astype(np.uint32)
    rng = np.random.default_rng(seed)
    st, gl = free[rng.integers(0, free.size, k)], free[rng.integers(0, free.size, k)]
    t0 = np.zeros(k, dtype=np.uint32)
    dev = lambda: p.astar_reserved(st, gl, t0, node, edge, max_time)  # noqa: E731
    host = lambda: host_astar_reserved(rows, st, gl, t0, node, edge, max_time)  # noqa: E731
    ref = dev()  # warm-up of both legs, and the comparison
    href = host()
    same = all(np.array_equal(a, b) for a, b in zip(ref, href))
    assert same, "the device and the host twin differ"
    t_dev, t_host, probes = [], [], []
    for r in range(runs):
        got, ms = timed(dev)
        assert np.array_equal(got[1], ref[1])
        t_dev.append(ms)
        probes.append(p.st_astar_probe())
        if r < HOST_RUNS:
            t_host.append(timed(host)[1])
    off, path, status, pops = ref
    npops = int(pops.sum())
    waves = probes[-1]["waves"]
    out = {"queries": k, "found": int((status == TSW_SP_FOUND).sum()), "none": int((status == TSW_SP_NONE).sum()),
           "capacity": int((status == TSW_SP_CAPACITY).sum()), "pops": npops, "pops_max": int(pops.max()),
           "path_entries": int(path.size), "waves": waves, "batches": probes[-1]["batches"],
           "equals_host_twin": bool(same), "device_call": summary(t_dev), "host_twin": summary(t_host),
           "split_ms": {key: summary([q[key] for q in probes]) for key in ("reservations_ms", "search_ms", "pack_ms")}}
    search = out["split_ms"]["search_ms"]["median_ms"]
    out["device_us_per_query"] = 1e3 * out["device_call"]["median_ms"] / k
    out["host_us_per_query"] = 1e3 * out["host_twin"]["median_ms"] / k
    out["search_ns_per_pop_all_waves"] = 1e6 * search / max(npops, 1)
    out["wave_clocks_per_pop"] = search * 1e-3 * CLOCK_MHZ * 1e6 * min(waves, k) / max(npops, 1)
    # with one query per wave the kernel lasts as long as its longest search: that search's time per pop
    out["longest_query_us_per_pop"] = 1e3 * search / max(int(pops.max()), 1) if k <= waves else None
    out["host_ns_per_pop"] = 1e6 * out["host_twin"]["median_ms"] / max(npops, 1)
    out["host_over_device_call"] = out["host_twin"]["median_ms"] / out["device_call"]["median_ms"]
    out["host_over_search_kernel"] = out["host_twin"]["median_ms"] / max(search, 1e-9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "st_astar.json"))
    a = ap.parse_args()
    rows, starts, tasks = maps.config_instance("c3_warehouse_170x84")
    w, h = len(rows[0]), len(rows)
    max_time = 2 * (w + h)
    out = {"map": "c3_warehouse_170x84", "max_time": max_time, "max_nodes": 65536, "runs": a.runs, "host_runs": HOST_RUNS,
           "clock_mhz_assumed": CLOCK_MHZ, "build_id": build_id(), "legs": {}}
    with Planner(rows) as p:
        rec = p.plan_mapd_arrays(starts, tasks, MAX_T)[0]
        node, edge = reservations(rec, w)
        out["plan_columns"] = int(rec.shape[1])
        out["vertex_reservations"], out["edge_reservations"] = int(node.shape[0]), int(edge.shape[0])
        out["vertex_reservations_in_horizon"] = int((node[:, 1] <= max_time + 1).sum())
        for k in a.queries:
            out["legs"][str(k)] = measure(p, rows, k, node, edge, max_time, a.runs, 20 + k)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for k, r in out["legs"].items():
        print(k, json.dumps({"device_ms": r["device_call"]["median_ms"], "host_ms": r["host_twin"]["median_ms"],
                             "split_ms": {key: v["median_ms"] for key, v in r["split_ms"].items()},
                             "pops": r["pops"], "wave_clocks_per_pop": r["wave_clocks_per_pop"],
                             "host_ns_per_pop": r["host_ns_per_pop"], "found": r["found"], "none": r["none"],
                             "capacity": r["capacity"]}))


if __name__ == "__main__":
    main()
