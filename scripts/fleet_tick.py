"""Time per decentralized tick of a whole fleet, two ways, alternating in one process on warm tables:

  (a) what tsw_decide alone offers: every agent's nearby list built on the host (numpy, all pairs) and
      handed to the batched decision — reported as list-build ms, the tsw_decide call on the flattened
      lists alone (decide-call ms: the least any caller of (a) pays), and Planner.decide (which also
      flattens the lists in Python) over a few ticks;
  (b) Planner.decide_fleet: lists and decisions on the device (tsw_decide_fleet).

Before timing, (b)'s decisions are checked against (a)'s on the same inputs. Every timed call ends in a
stream synchronise inside the library; the clock is the host's. Needs a GPU (Planner raises without one).

usage: python scripts/fleet_tick.py [--ticks 20] [--warmup 3] [--radius 15] [--out profiles/r7/fleet_tick.json]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from p2p_distributed_tswap_amd import Planner, build_id, maps  # noqa: E402

INSTANCES = {  # name: (map, agents, seed)
    "warehouse_170x84_1k": (lambda: maps.warehouse_map(170, 84, 0x170084), 1000, 0x170084),
    "wh10k_510x220_10k": (lambda: maps.warehouse_map(510, 220, 0x510220), 10000, 0x510220),
}


def _u32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def host_lists(v, W, r, chunk=512):
    """(nb_off, nb_idx) on the host: all pairs, |dx| + |dy| <= r, self excluded, ascending index."""
    n = v.size
    x, y = (v % W).astype(np.int32), (v // W).astype(np.int32)
    counts = np.zeros(n, dtype=np.int64)
    cols = []
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        m = (np.abs(x[i0:i1, None] - x[None, :]) + np.abs(y[i0:i1, None] - y[None, :])) <= r
        m[np.arange(i1 - i0), np.arange(i0, i1)] = False
        counts[i0:i1] = m.sum(axis=1)
        cols.append(np.nonzero(m)[1])
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(counts)
    return off, np.concatenate(cols).astype(np.uint32)


class RawDecide:
    """tsw_decide on flattened lists with preallocated outputs: the call itself, nothing around it."""

    def __init__(self, p, n, tot):
        self.p = p
        self.act, self.cell, self.partner, self.npart = (np.zeros(n, dtype=np.uint32) for _ in range(4))
        self.part = np.zeros(tot + n + 1, dtype=np.uint32)

    def __call__(self, v, g, off, nv, ng):
        p = self.p
        p._check(p._lib.tsw_decide(p._ctx, _u32p(v), _u32p(g), v.size, _u32p(off), _u32p(nv), _u32p(ng),
                                   _u32p(self.act), _u32p(self.cell), _u32p(self.partner), _u32p(self.npart),
                                   _u32p(self.part)))


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda f: float(np.quantile(a, f))  # noqa: E731
    return {"median_ms": round(q(0.5), 4), "p25_ms": round(q(0.25), 4), "p75_ms": round(q(0.75), 4),
            "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "ticks": int(a.size)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def run_instance(name, ticks, warmup, radius, wrapper_ticks):
    make, n, seed = INSTANCES[name]
    rows = make()
    W, H = len(rows[0]), len(rows)
    comp = maps.largest_component(rows)
    rng = random.Random(seed)
    v = np.array([y * W + x for x, y in rng.sample(comp, n)], dtype=np.uint32)
    g = np.array([y * W + x for x, y in (rng.choice(comp) for _ in range(n))], dtype=np.uint32)
    res = {"map": [W, H], "agents": n, "radius": radius}
    with Planner(rows) as p:
        off, idx = host_lists(v, W, radius)
        nv, ng = v[idx], g[idx]
        raw = RawDecide(p, n, int(off[-1]))
        for _ in range(warmup):  # warm tables: every next hop the tick needs is resolved after these
            raw(v, g, off, nv, ng)
            fleet = p.decide_fleet(v, g, radius)
        # (b) == (a) on the same inputs, list indices mapped to agent indices
        noff, nidx = p.nearby(v, radius)
        assert np.array_equal(noff, off) and np.array_equal(nidx, idx), "device lists differ from the host's"
        act, cell, partner, part_off, part = fleet
        assert np.array_equal(act, raw.act) and np.array_equal(cell, raw.cell)
        has = raw.partner != 0xFFFFFFFF
        assert np.array_equal(partner[~has], raw.partner[~has])
        assert np.array_equal(partner[has], idx[off[:-1][has].astype(np.int64) + raw.partner[has]])
        assert np.array_equal(np.diff(part_off.astype(np.int64)), raw.npart)
        for i in np.flatnonzero(raw.npart):
            b = int(off[i]) + int(i)
            assert np.array_equal(part[part_off[i]:part_off[i + 1]], idx[int(off[i]) + raw.part[b:b + raw.npart[i]]])
        res["lists_total"] = int(off[-1])
        res["longest_list"] = int(np.diff(off.astype(np.int64)).max())
        res["actions_move_swap_rotation_wait"] = [int((act == k).sum()) for k in range(4)]
        t_build, t_call, t_fleet, t_wrap = [], [], [], []
        for k in range(ticks):  # alternate (a) and (b)
            ms, (off, idx) = timed(lambda: host_lists(v, W, radius))
            nv, ng = v[idx], g[idx]
            t_build.append(ms)
            t_call.append(timed(lambda: raw(v, g, off, nv, ng))[0])
            t_fleet.append(timed(lambda: p.decide_fleet(v, g, radius))[0])
            if k < wrapper_ticks:
                lists = [list(zip(nv[off[i]:off[i + 1]].tolist(), ng[off[i]:off[i + 1]].tolist())) for i in range(n)]
                t_wrap.append(timed(lambda: p.decide(v, g, lists))[0])
    res["a_list_build"] = summary(t_build)
    res["a_decide_call"] = summary(t_call)
    res["a_planner_decide"] = summary(t_wrap)
    res["b_decide_fleet"] = summary(t_fleet)
    a, b = res["a_decide_call"], res["b_decide_fleet"]
    res["a_decide_call_spread_ms"] = round(a["p75_ms"] - a["p25_ms"], 4)  # interquartile: the margin
    res["b_not_slower_than_a_decide_call"] = bool(b["median_ms"] <= a["median_ms"] + res["a_decide_call_spread_ms"])
    res["speedup_vs_a_total"] = round((res["a_list_build"]["median_ms"] + a["median_ms"]) / b["median_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=int, default=15)
    ap.add_argument("--wrapper-ticks", type=int, default=3, help="ticks that also time Planner.decide (Python flattening)")
    ap.add_argument("--instances", nargs="*", default=list(INSTANCES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "fleet_tick.json"))
    a = ap.parse_args()
    out = {"build_id": build_id(), "method": "host clock around calls that end in a stream synchronise; (a) and (b) "
           "alternate tick by tick in one process on warm tables; spread = interquartile range",
           "instances": {}}
    for name in a.instances:
        out["instances"][name] = run_instance(name, a.ticks, a.warmup, a.radius, a.wrapper_ticks)
        print(name, json.dumps(out["instances"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"fleet_tick": a.out, "build_id": out["build_id"]}), flush=True)


if __name__ == "__main__":
    main()
