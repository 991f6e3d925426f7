"""The two planning modes on the same instances, audited on the device (first open item):
tsw_plan_mapd (centralized TSWAP) and tsw_fleet_mapd (the lock-step decentralized run) from the same starts
and tasks, each plan's records through tsw_audit_records, side by side: columns, ending, deliveries, moving
columns, colocations, swaps, jumps.

Per instance the parent starts ONE child process (one context) under `timeout`; the parent never opens the
device. The child also times the audit: Planner.audit (host records: upload + both passes + read-back) and
Planner.audit_device (records resident on the device), against the same counts in numpy in the same
process, and reports the byte floor (records read once / the measured time) and where pass B's table lived.
Every timed call ends in a stream synchronise inside the library; the clock is the host's.

The split between the passes comes from a kernel trace of the audit alone, in a run of its own per instance
(the profiler slows the host side, so it is never on while timing):
    python scripts/mode_compare.py --trace            # also runs each traced instance under rocprofv3

usage: python scripts/mode_compare.py [--instances NAME ...] [--reps 5] [--trace] [--out profiles/r15/mode_compare.json]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # fleet_mapd_model: the named small cases

BIG = {  # name: (instance, radius, plan max_t, fleet max_t)
    "c3_warehouse_170x84_1k": (lambda maps: maps.config_instance("c3_warehouse_170x84"), 15, 2000, 2000),
    "wh10k_510x220_10k": (lambda maps: maps.wh10k_instance(), 15, 2000, 200),  # scripts/fleet_mapd.py's horizon
}
TIMEOUT_S = {"c3_warehouse_170x84_1k": 300, "wh10k_510x220_10k": 600}
AUDIT_KERNELS = ("k_audit_rows", "k_audit_columns")
LDS_TABLE_BYTES_PER_CELL = 8  # csrc/tsw_audit.hip: one 64-bit entry per cell


def small_cases():
    import fleet_mapd_model as mm

    return list(mm.CASES)


def instance(name):
    from p2p_distributed_tswap_amd import maps

    if name in BIG:
        make, radius, plan_t, fleet_t = BIG[name]
        rows, starts, tasks = make(maps)
        return rows, starts, tasks, radius, plan_t, fleet_t
    import fleet_mapd_model as mm

    rows, starts, tasks, radius, max_t, _ = mm.instance(name)
    return rows, starts, tasks, radius, max_t, max_t


def numpy_counts(rec, w, h):
    """The audit's summary counts the way a caller had to get them before: numpy on the host."""
    x = (rec & np.uint64(0xFFFF)).astype(np.int64)
    y = ((rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
    st = (rec >> np.uint64(32)) & np.uint64(0xFF)
    on = (x < w) & (y < h)
    cell = y * w + x
    out = {"colocations": 0, "swaps": 0}
    for t in range(rec.shape[1]):
        c = cell[on[:, t], t]
        out["colocations"] += int(c.size - np.unique(c).size)
    dist = np.abs(x[:, 1:] - x[:, :-1]) + np.abs(y[:, 1:] - y[:, :-1])
    out["moves"] = int(np.count_nonzero(dist))
    out["jumps"] = int(np.count_nonzero(dist > 1))
    out["moving_columns"] = int(np.count_nonzero((dist != 0).any(axis=0)))
    dl = st == 2
    out["deliveries"] = int(np.count_nonzero(dl[:, 0])) + int(np.count_nonzero(dl[:, 1:] & ~dl[:, :-1]))
    unit = (dist == 1) & on[:, 1:] & on[:, :-1]
    ncell = w * h
    for t in range(dist.shape[1]):
        u = unit[:, t]
        fwd = cell[u, t] * ncell + cell[u, t + 1]
        back = cell[u, t + 1] * ncell + cell[u, t]
        out["swaps"] += int(np.count_nonzero(np.isin(fwd, back)))
    return out


def median_ms(call, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


class DeviceCopy:
    """The records in device memory, from the HIP runtime the library links."""

    def __init__(self, rec):
        import ctypes

        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(rec.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, rec.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rec.nbytes), 1) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def close(self):
        self.hip.hipFree(self.ptr)


def side(p, rec, w, h, reps, ending):
    """One mode's column of the comparison, with the audit's timings on its records."""
    keys = ("deliveries", "moving_columns", "colocations", "swaps", "jumps", "off_map", "bad_state", "moves")
    a = p.audit(rec)
    out = {"columns": int(rec.shape[1]), "ending": ending, **{k: int(a[k]) for k in keys},
           "first_t": a["first_t"], "first_agent": a["first_agent"]}
    t0 = time.perf_counter()
    ref = numpy_counts(rec, w, h)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    for k, v in ref.items():
        assert out[k] == v, f"audit and numpy disagree on {k}: {out[k]} vs {v}"
    dev = DeviceCopy(rec)
    try:
        n, T = rec.shape
        p.audit_device(dev.ptr.value, n, T, T)  # warm: the scratch is allocated
        host_ms, host_min = median_ms(lambda: p.audit(rec), reps)
        full_ms, _ = median_ms(lambda: p.audit(rec, col=True, agents=True), reps)
        dev_ms, dev_min = median_ms(lambda: p.audit_device(dev.ptr.value, n, T, T), reps)
    finally:
        dev.close()
    out["audit"] = {
        "records_bytes": int(rec.nbytes), "reps": reps,
        "host_records_median_ms": host_ms, "host_records_min_ms": host_min,
        "host_records_col_agents_median_ms": full_ms,
        "device_records_median_ms": dev_ms, "device_records_min_ms": dev_min,
        "numpy_same_counts_ms": round(numpy_ms, 3),
        "device_records_GBps": round(rec.nbytes / (dev_ms * 1e-3) / 1e9, 2),  # records read once / time
        "host_records_GBps": round(rec.nbytes / (host_ms * 1e-3) / 1e9, 2),
    }
    return out


def run_one(name, reps, audit_only):
    from p2p_distributed_tswap_amd import Planner, build_id

    rows, starts, tasks, radius, plan_t, fleet_t = instance(name)
    w, h = len(rows[0]), len(rows)
    res = {"map": [w, h], "cells": w * h, "agents": int(starts.shape[0]), "tasks": int(tasks.shape[0]), "radius": radius,
           "plan_max_t": plan_t, "fleet_max_t": fleet_t, "build_id": build_id(),
           "audit_table": "lds" if w * h * LDS_TABLE_BYTES_PER_CELL + 64 <= 160 * 1024 else "global"}
    with Planner(rows) as p:
        t0 = time.perf_counter()
        prec, _ = p.plan_mapd_arrays(starts, tasks, plan_t)
        res["plan_mapd_s"] = round(time.perf_counter() - t0, 3)
        if audit_only:  # the kernel-trace run: the audit alone, a few times
            for _ in range(3):
                p.audit(prec)
            return {"instance": name, "audits": 3}
        t0 = time.perf_counter()
        frec, stalled = p.fleet_mapd(starts, tasks, fleet_t, radius)
        res["fleet_mapd_s"] = round(time.perf_counter() - t0, 3)
        res["plan_mapd"] = side(p, prec, w, h, reps, "horizon" if prec.shape[1] == plan_t + 1 else "done")
        last_idle = frec.shape[1] > 0 and bool(np.all((frec[:, -1] >> np.uint64(32)) == 3))
        ending = "stalled" if stalled else "horizon" if frec.shape[1] == fleet_t + 1 and not last_idle else "done"
        res["fleet_mapd"] = side(p, frec, w, h, reps, ending)
    return res


def kernel_split(path):
    """Per-kernel totals of the audit from a rocprofv3 --kernel-trace --stats run (its *kernel_stats.csv)."""
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {"error": f"no *kernel_stats.csv under {path}"}
    found = {}
    with open(files[0], newline="") as fh:
        for r in csv.DictReader(fh):
            m = re.match(r"(?:void )?([\w:]+)", r["Name"].replace("(anonymous namespace)::", ""))
            k = m.group(1).split("::")[-1] if m else r["Name"]
            if k in AUDIT_KERNELS:  # the full name keeps k_audit_columns' template argument: <true> = the table in LDS
                found[k] = {"name": r["Name"], "calls": int(r["Calls"]), "mean_us": round(float(r["AverageNs"]) / 1e3, 2)}
    tot = sum(v["mean_us"] for v in found.values())
    return {"source": "rocprofv3 --kernel-trace --stats over `mode_compare.py --one <instance> --audit-only`, a run of its own",
            "kernels": found,
            "pass_b_share_of_kernel_time": round(found["k_audit_columns"]["mean_us"] / tot, 4) if len(found) == 2 and tot else None}


def child(args, name, extra=(), wrap=()):
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S.get(name, 120)), *wrap, sys.executable, os.path.abspath(__file__), "--one", name,
           "--reps", str(args.reps), *extra]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{name}: child exited with {r.returncode}; stopping (nothing more is started on the device)")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", nargs="*")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", help="(child) run this instance in this process and print its JSON")
    ap.add_argument("--audit-only", action="store_true", help="(child) plan once, then the audit alone: the kernel-trace run")
    ap.add_argument("--trace", action="store_true", help="also trace the audit of the large instances under rocprofv3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "mode_compare.json"))
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run_one(a.one, a.reps, a.audit_only)), flush=True)
        return
    names = a.instances or small_cases() + list(BIG)
    out = {"method": "one process and one context per instance; both modes from the same starts and tasks; audit timings: host "
           "clock around calls that end in a stream synchronise, median of reps; numpy: the same counts on the host, once",
           "instances": {}}
    for name in names:
        res = child(a, name)
        out.setdefault("build_id", res["build_id"])
        assert res["build_id"] == out["build_id"]
        if a.trace and name in BIG:
            with tempfile.TemporaryDirectory() as d:
                child(a, name, ("--audit-only",), ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
                                                   "-o", "run", "--"))
                res["kernel_trace"] = kernel_split(d)
        out["instances"][name] = res
        print(name, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"mode_compare": a.out, "build_id": out["build_id"]}), flush=True)


if __name__ == "__main__":
    main()
