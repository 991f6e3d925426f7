#!/usr/bin/env python3
"""What tsw_task_timeline costs on the records of a plan, and what it replaces.

Per instance (C3: 170x84 warehouse, 1,000 agents, the 32,000-task stream, max_t 2000; optionally wh10k) and per
release schedule (every task at 0; 16 tasks released per step, as scripts/online_plan.py paces them), in one
process on one context:

  plan      plan_mapd_online, wall ms                                   the plan the timeline describes
  timeline  task_timeline_device on the records resident on the device, wall ms and, from tsw_probe_timeline, the
            HIP-event time of each pass (A events, B replay, C attach), the takes and the candidates the takes scanned
  host      task_timeline on the same records in host memory (adds the upload)
  model     tests/timeline_model.replay, the Python loop over the records that the call replaces (once)

The plan and timeline legs alternate, RUNS times each after a warm-up of both (median and interquartile range).
The device's table must equal the model's.

  python scripts/task_timeline.py [--runs 5] [--instance c3|wh10k] [--out profiles/r19/task_timeline.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from p2p_distributed_tswap_amd import Planner, build_id, maps  # noqa: E402

MAX_T = 2000
PER_STEP = 16
SUMMARY = ("wait_sum", "service_sum", "carry_sum", "assigned", "carried", "delivered", "unreleased", "service_min",
           "service_max", "makespan", "consistent")


class DevBuf:
    """Device memory from the HIP runtime the library links (a second runtime in the process cannot open the device)."""

    def __init__(self, arr):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(arr.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(arr.nbytes), 1) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def summary(xs):
    q1, med, q3 = (float(x) for x in np.percentile(xs, [25, 50, 75]))
    return {"median_ms": med, "iqr_ms": [q1, q3], "runs_ms": [float(x) for x in xs]}


def timed(f):
    t0 = time.perf_counter()
    r = f()  # every Planner call returns after its device work
    return r, (time.perf_counter() - t0) * 1e3


def measure(p, starts, tasks, rel, runs, with_model):
    plan = lambda: p.plan_mapd_online(starts, tasks, rel, MAX_T)[0]  # noqa: E731
    rec = np.ascontiguousarray(plan())
    n, T = rec.shape
    dev = DevBuf(rec)
    tl = lambda: p.task_timeline_device(dev.ptr.value, n, T, T, starts, tasks, rel)  # noqa: E731
    ref = tl()
    host = p.task_timeline(rec, starts, tasks, rel)
    assert all(np.array_equal(ref[k], host[k]) for k in ref), "the host and the device form differ"
    t_plan, t_tl, t_host, passes = [], [], [], []
    for _ in range(runs):
        r, ms = timed(plan)
        assert np.array_equal(r, rec), "a repeated call gave another plan"
        t_plan.append(ms)
        got, ms = timed(tl)
        assert np.array_equal(got["task"], ref["task"])
        t_tl.append(ms)
        passes.append(p.timeline_probe())
        t_host.append(timed(lambda: p.task_timeline(rec, starts, tasks, rel))[1])
    dev.free()
    out = {"columns": T, "plan": summary(t_plan), "timeline_device": summary(t_tl), "timeline_host": summary(t_host),
           "passes_ms": {k: summary([q[k] for q in passes]) for k in ("events_ms", "replay_ms", "attach_ms")},
           "takes": passes[-1]["takes"], "candidates_scanned": passes[-1]["candidates_scanned"],
           "compactions": 0,  # the candidate array never holds a dead entry: a take overwrites its entry with the last
           "summary": {k: int(ref[k]) for k in SUMMARY}}
    out["candidates_per_take"] = out["candidates_scanned"] / max(out["takes"], 1)
    out["replay_us_per_take"] = 1e3 * out["passes_ms"]["replay_ms"]["median_ms"] / max(out["takes"], 1)
    out["timeline_over_plan"] = out["timeline_device"]["median_ms"] / out["plan"]["median_ms"]
    if with_model:
        import timeline_model as tm

        model, ms = timed(lambda: tm.replay(rec, starts, tasks, rel))
        out["python_model_ms"] = ms
        out["equals_python_model"] = bool(np.array_equal(model["task"], ref["task"])
                                          and all(int(model[k]) == int(ref[k]) for k in SUMMARY))
        assert out["equals_python_model"], "the device's timeline differs from the Python model's"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--instance", choices=("c3", "wh10k"), default="c3",
                    help="wh10k: the 10,000-agent warehouse (releases at 0 only, no Python model)")
    ap.add_argument("--skip-model", action="store_true", help="leave the Python model out (it takes the longest)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "task_timeline.json"))
    a = ap.parse_args()
    out = {"max_t": MAX_T, "runs": a.runs, "released_per_step": PER_STEP, "build_id": build_id(), "instances": {}}
    for name in ("c3_warehouse_170x84" if a.instance == "c3" else "wh10k",):
        rows, starts, tasks = maps.config_instance(name) if name != "wh10k" else maps.wh10k_instance()
        m = len(tasks)
        legs = {"release_0": np.zeros(m, dtype=np.uint32)}
        if name != "wh10k":
            legs[f"release_{PER_STEP}_per_step"] = (np.arange(m) // PER_STEP).astype(np.uint32)
        inst = {"agents": len(starts), "tasks": m, "legs": {}}
        with Planner(rows) as p:
            for leg, rel in legs.items():
                inst["legs"][leg] = measure(p, starts, tasks, rel, a.runs, name != "wh10k" and not a.skip_model)
        out["instances"][name] = inst
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for name, inst in out["instances"].items():
        for leg, r in inst["legs"].items():
            print(name, leg, json.dumps({"plan_ms": r["plan"]["median_ms"], "timeline_ms": r["timeline_device"]["median_ms"],
                                         "passes_ms": {k: v["median_ms"] for k, v in r["passes_ms"].items()},
                                         "takes": r["takes"], "candidates_per_take": r["candidates_per_take"],
                                         "python_model_ms": r.get("python_model_ms")}))


if __name__ == "__main__":
    main()
