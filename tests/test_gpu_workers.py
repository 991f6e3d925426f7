"""GPU: the K3 workers inside the plan dispatch (tsw_worker.h: resolve_exact, stage_detour, the tier chain,
over astar_wave_par of tsw_astar.h) at their tier and DAG-exit boundaries, in every layout worker_config()
can give them.

Every context runs with the host A* service off, so only workers answer. The instances come from
tests/worker_cases.py (premises checked on the CPU by tests/test_worker_cases.py): agents standing on
multi-candidate cells of every detour class around the byte g-scores' overflow and the detour bytes'
saturation, on maps whose heaps outgrow the register heap. After each call EVERY resolved code the context's
table store holds for the instance's goals is compared with the oracle — also the speculative and task-chain
answers that no step of the call consumed.
"""
import re

import numpy as np
import pytest

import worker_cases as wc
from p2p_distributed_tswap_amd import Planner, TSW_HOST_ASTAR_OFF, maps
from table_io_cases import check_store  # the store audit, shared with the table entry-point tests
from worker_cases import NH_STAY, MapRef

pytestmark = pytest.mark.gpu


def check_own_cells(tabs, goals, v, g, what: str):
    """Every agent's own (v, g) code is resolved (0..4)."""
    slot = {int(goal): k for k, goal in enumerate(goals)}
    codes = np.array([tabs[slot[int(b)]][int(a)] for a, b in zip(v, g)], dtype=np.uint8)
    bad = np.flatnonzero(codes > NH_STAY)
    assert bad.size == 0, f"{what}: {bad.size} agents' own codes unresolved, first agent {bad[0]}: 0x{codes[bad[0]]:02x}"


# The two stderr lines of worker_args and coop_debug_report (tsw_plan_host.hip) under TSW_PLAN_DEBUG that _diag() depends on:
#   fprintf(stderr, "[k_plan] workers: %u waves (%u per workgroup), g-scores %u, heap %u entries, DAG exit %u, %u B LDS each\n", ...)
#   fprintf(stderr, "[k_plan] worker A* ms (queries, pops): ... | tier-2 hand-offs %llu tier-3 %llu | detour staging %.1f ms (%u)\n", ...)
_RE_WORKERS = re.compile(r"\[k_plan\] workers: (\d+) waves \((\d+) per workgroup\), g-scores (\d+), heap (\d+) entries, "
                         r"DAG exit (\d+), (\d+) B LDS each")
_RE_TIERS = re.compile(r"tier-2 hand-offs (\d+) tier-3 (\d+) \| detour staging [0-9.]+ ms \((\d+)\)")


def _diag(err: str):
    """(layout, tier2, tier3, staged) of a diagnostic call's stderr: layout = (g-scores, heap, DAG exit, LDS bytes
    per worker) of every dispatch (they must agree), the counts summed over the call's dispatches."""
    lay = {tuple(int(x) for x in m.groups()[2:]) for m in _RE_WORKERS.finditer(err)}
    assert len(lay) == 1, f"worker layout lines: {sorted(lay)}"
    tiers = [tuple(int(x) for x in m.groups()) for m in _RE_TIERS.finditer(err)]
    assert tiers, "no worker A* line in the diagnostic output"
    return lay.pop(), sum(t[0] for t in tiers), sum(t[1] for t in tiers), sum(t[2] for t in tiers)


def _r16(x):
    return (x + 15) // 16 * 16


def check_layout(lay, ref: MapRef, env):
    """The layout worker_config() chose is the one the knobs ask for (a silent fall-back would turn the matrix
    into one case), and a worker's LDS slice holds what coop_worker carves from it: heap, g-scores, the
    bitmap padded to 16 bytes, the detour bytes."""
    gs, heap, dag, lds = lay
    ncell, fbb = ref.W * ref.H, _r16(ref.H * ((ref.W + 31) // 32) * 4)
    want_gs = env.get("TSW_WORKER_GS")
    if want_gs is not None:
        assert gs == int(want_gs), lay
    assert dag == (0 if env.get("TSW_DAG_EXIT") == "0" else 1 if gs != 0 else 2), lay
    if "TSW_ASTAR_WAVE_HCAP" in env:
        assert heap == int(env["TSW_ASTAR_WAVE_HCAP"]), lay
    else:
        assert heap > 64, lay
    fb = not (gs == 0 and env.get("TSW_WORKER_FB") == "0")
    gsb = ncell * 4 if gs == 1 else _r16(ncell) if gs == 2 else 0
    carve = heap * 8 + gsb + (fbb if fb else 0) + (ncell if dag == 1 else 0)
    assert lds >= carve, f"{lay}: a worker's slice is {carve - lds} bytes short of its carve"
    if gs == 0 and "TSW_WORKER_FB" in env:
        assert lds == _r16(carve), f"{lay}: TSW_WORKER_FB={env['TSW_WORKER_FB']} not honoured"


def check_stats(st, what):
    assert st["coop_workers"] > 0, what
    assert sum(st["plan_exits"]) == 0, (what, st["plan_exits"])
    assert st["watchdog_fires"] == 0, what
    assert st["host_astar_queries"] == 0, what
    assert st["coop_worker_queries"][0] > 0, what


# ---- 3b: tsw_step on the class-selected instances ----------------------------------------------------------

_step_cache = {}


def _step_case(size, kind):
    """(ref, v0, g0, [(v1, g1), (v2, g2)]) of serpentine(*size): two oracle steps, computed once. Both kinds of
    instance of a map share its MapRef (they use the same goals)."""
    if (size, kind) not in _step_cache:
        ref = next((c[0] for (sz, _), c in _step_cache.items() if sz == size), None) or MapRef(wc.serpentine(*size))
        v, g = (wc.saturation_instance if kind == "saturated" else wc.step_instance)(ref.rows)
        s1 = ref.og.step(v, g)
        s2 = ref.og.step(*s1)
        for a in (v, g, *s1, *s2):
            a.setflags(write=False)
        _step_cache[(size, kind)] = (ref, v, g, [s1, s2])
    return _step_cache[(size, kind)]


S, L = (120, 100), (200, 130)
STEP_RUNS = [
    ("prod-120x100", False, S, {}),
    ("prod-200x130", False, L, {}),
    ("gs2", True, S, {"TSW_WORKER_GS": "2"}),
    ("gs1", True, S, {"TSW_WORKER_GS": "1"}),
    ("gs0-fb1", True, S, {"TSW_WORKER_GS": "0", "TSW_WORKER_FB": "1"}),
    ("gs0-fb0", True, S, {"TSW_WORKER_GS": "0", "TSW_WORKER_FB": "0"}),
    ("gs2-noexit", True, S, {"TSW_WORKER_GS": "2", "TSW_DAG_EXIT": "0"}),
    ("gs2-mask1", True, S, {"TSW_WORKER_GS": "2", "TSW_DAG_MASK": "1"}),
    ("gs2-hcap64", True, S, {"TSW_WORKER_GS": "2", "TSW_ASTAR_WAVE_HCAP": "64"}),
    ("gs1-hcap64-lds-heap", True, S, {"TSW_WORKER_GS": "1", "TSW_ASTAR_WAVE_HCAP": "64", "TSW_ASTAR_REGHEAP": "0"}),
    ("gs2-regheap41", True, S, {"TSW_WORKER_GS": "2", "TSW_ASTAR_REGHEAP": "41"}),
    ("gs0-200x130", True, L, {"TSW_WORKER_GS": "0"}),
    # the layout worker_config() picks by itself on 200x130 (H * Ww = 910 words of bitmap, not a multiple of
    # 16 bytes, an odd heap size): its slice must hold the padded carve (check_layout)
    ("default-200x130", True, L, {}),
    # every multi-candidate cell with detour byte 254 / 255 / 256 (worker_cases.saturation_instance), global
    # g-scores (the bytes are read from the store: astar_wave_par itself switches the exit off at a saturated
    # start), the exit tested after every 2nd pop
    ("gs0-mask1-saturated", True, S, {"TSW_WORKER_GS": "0", "TSW_DAG_MASK": "1"}),
]


def _set_knobs(monkeypatch, capfd, diag, env):
    if diag:
        monkeypatch.setenv("TSW_PLAN_DEBUG", "1")
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        capfd.readouterr()


def _check_diag(capfd, ref, env, what, need_tier2=False, need_tier3=False):
    err = capfd.readouterr().err
    lay, t2, t3, staged = _diag(err)
    print(f"{what}: g-scores {lay[0]} heap {lay[1]} DAG exit {lay[2]} LDS {lay[3]} B | tier-2 hand-offs {t2} "
          f"tier-3 {t3} detour stagings {staged}")
    check_layout(lay, ref, env)
    if need_tier2:
        assert t2 > 0, what
    if need_tier3:
        assert t3 > 0 and (lay[0] == 0 or t2 >= t3), what
    if lay[2] == 1:
        assert staged > 0, what
    else:
        assert staged == 0, what


@pytest.mark.parametrize("name,diag,size,env", STEP_RUNS, ids=[r[0] for r in STEP_RUNS])
def test_step_class_instances(name, diag, size, env, monkeypatch, capfd):
    """Two consecutive tsw_step calls == OracleGraph.step (v and g), every agent's own code resolved after
    each, then the whole store against the oracle."""
    ref, v0, g0, steps = _step_case(size, "saturated" if name.endswith("saturated") else "classes")
    _set_knobs(monkeypatch, capfd, diag, env)
    with Planner(ref.rows, diag=diag, host_astar=TSW_HOST_ASTAR_OFF) as p:
        v, g = v0, g0
        for k, (rv, rg) in enumerate(steps):
            hv, hg = p.step(v, g)
            dv, dg = np.flatnonzero(hv != rv), np.flatnonzero(hg != rg)
            assert dv.size == 0 and dg.size == 0, f"{name} step {k}: v differs at agents {dv[:8]}, g at {dg[:8]}"
            tabs = p.next_hop_tables(np.unique(g0))
            # the rules phase read (v, g) of every agent, the movement phase (v, g after the goal swaps)
            check_own_cells(tabs, np.unique(g0), v, g, f"{name} step {k} (v, g)")
            check_own_cells(tabs, np.unique(g0), v, rg, f"{name} step {k} (v, g')")
            v, g = rv, rg
        st = p.stats()
        _, _, n = check_store(p, ref, g0, name)
    print(f"{name}: {n} A*-decided codes in the store checked; worker queries needed/spec/chain "
          f"{st['coop_worker_queries']}; oracle so far {ref.oracle_calls} calls {ref.oracle_s:.1f} s")
    check_stats(st, name)
    assert n >= v0.size
    if diag:
        hc = env.get("TSW_ASTAR_WAVE_HCAP") == "64"
        # delta >= 32 overflows the byte g-scores; without the early exit such a query always reaches that node
        _check_diag(capfd, ref, env, name, need_tier2=name == "gs2-noexit" or (hc and env["TSW_WORKER_GS"] != "0"),
                    need_tier3=hc)


# ---- 3c / 3d: tsw_plan_mapd_trace, task chains and the DAG prefetch ---------------------------------------------

_plan_cache = {}


def _plan_case(which):
    if which not in _plan_cache:
        rows, starts, tasks, max_t = (wc.plan_serpentine if which == "serpentine" else wc.plan_cave)()
        ref = MapRef(rows)
        rec, goal = ref.og.mapd(starts, tasks, max_t, trace_goals=True)
        assert maps.moving_timesteps(rec) == max_t
        rec.setflags(write=False)
        goal.setflags(write=False)
        W = ref.W
        goals = np.unique(np.concatenate([starts[:, 1] * W + starts[:, 0], tasks[:, 1] * W + tasks[:, 0],
                                          tasks[:, 3] * W + tasks[:, 2]]).astype(np.uint32))
        _plan_cache[which] = (ref, starts, tasks, max_t, rec, goal, goals)
    return _plan_cache[which]


PLAN_RUNS = [
    ("serpentine-prod", "serpentine", False, {}),
    ("serpentine-gs0", "serpentine", True, {"TSW_WORKER_GS": "0"}),
    ("serpentine-gs2-hcap64", "serpentine", True, {"TSW_WORKER_GS": "2", "TSW_ASTAR_WAVE_HCAP": "64"}),
    ("cave-prod", "cave", False, {}),
    ("cave-gs1-hcap64", "cave", True, {"TSW_WORKER_GS": "1", "TSW_ASTAR_WAVE_HCAP": "64"}),
    ("cave-gs2-lds-heap", "cave", True, {"TSW_WORKER_GS": "2", "TSW_ASTAR_REGHEAP": "0"}),
]


@pytest.mark.parametrize("name,which,diag,env", PLAN_RUNS, ids=[r[0] for r in PLAN_RUNS])
def test_plan_high_detour_and_large_heaps(name, which, diag, env, monkeypatch, capfd):
    """A coop-mode plan (task chains, DAG prefetch) on serpentine(200, 130) (detours in the hundreds) and on
    cave_map(128, 97, 9) (large heaps, small detours): records and goals == the oracle's, then the whole store
    over the plan's goal set (starts, pickups, deliveries)."""
    ref, starts, tasks, max_t, rrec, rgoal, goals = _plan_case(which)
    _set_knobs(monkeypatch, capfd, diag, env)
    with Planner(ref.rows, diag=diag, host_astar=TSW_HOST_ASTAR_OFF) as p:
        rec, goal = p.plan_mapd_arrays(starts, tasks, max_t, trace_goals=True)
        st = p.stats()
        assert rec.shape == rrec.shape
        if not np.array_equal(goal, rgoal):
            t = int(np.argmax((goal != rgoal).any(axis=0)))
            i = int(np.argmax(goal[:, t] != rgoal[:, t]))
            pytest.fail(f"{name}: goals diverge first at t={t}, agent {i}: {goal[i, t]} != {rgoal[i, t]}")
        if not np.array_equal(rec, rrec):
            t = int(np.argmax((rec != rrec).any(axis=0)))
            i = int(np.argmax(rec[:, t] != rrec[:, t]))
            pytest.fail(f"{name}: records diverge first at t={t}, agent {i}: {rec[i, t]:#x} != {rrec[i, t]:#x}")
        _, _, n = check_store(p, ref, goals, name)
    print(f"{name}: {n} A*-decided codes in the store checked over {goals.size} goals; worker queries needed/spec/chain "
          f"{st['coop_worker_queries']}; oracle so far {ref.oracle_calls} calls {ref.oracle_s:.1f} s")
    check_stats(st, name)
    assert n > 0
    if diag:
        _check_diag(capfd, ref, env, name, need_tier3=name == "cave-gs1-hcap64")
