"""GPU: K1 and K3 at the limits of their packed fields, bit-exact against the oracle. Coordinates of 1024 and more
(the 11th bit of x and y: 2048-wide and 2048-tall grids), table distances at both sides of 0x8000 and at the end
of the u16 range (a farthest cell at exactly 65,534 steps has a table, one at 65,535 has none), the wave A*
cores' hand-off at g = 2^15 with a wide frontier in the heap, k_astar_lds with all ten g bits set, and 2^20-cell
grids that are not square.

The maps and instances come from tests/limit_cases.py; tests/test_limit_cases.py checks on the CPU that they have
the properties these tests rely on. Oracle results are computed once per module and shared."""
import numpy as np
import pytest

import fleet_cases as fc
import limit_cases as lc
from p2p_distributed_tswap_amd import (TSW_EINVAL, TSW_EOVERFLOW, TSW_F_EAGER_NEXTHOP, TSW_F_EXIT_MODE,
                                       TSW_HOST_ASTAR_OFF, Planner, TswapError)

pytestmark = pytest.mark.gpu

INF = lc.INF
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- K1 ---------------------------------------------------------------------------------------------------------

K1_KERNELS = ["default", "mg", "blk", "blk-pair", "wave", "block", "big"]
K1_MAPS = ["wide", "tall", "exact", "over", *sorted(lc.STRIPS)]

# The forced kernels that fit each map on an MI355X (160 KiB of LDS per workgroup), from a run of this file on one;
# `default` (the production chain) and `block` run everywhere. Both directions are asserted: a listed kernel runs
# and is exact, an unlisted one is refused with TSW_EINVAL "does not fit". Why the unlisted ones do not fit:
_ALL = set(K1_KERNELS)
_FITS_BY_MAP = {
    # mg: bfs_mg_lds_bytes' V term, mg_vbytes = (W + 2) * (H + 2) * 2 = 143,500 of 169,412 bytes > 163,840
    "wide": _ALL - {"mg"},
    # mg: the same V term, 143,500 of 165,808 bytes > 163,840
    "tall": _ALL - {"mg"},
    # mg: the V term alone, (2048 + 2) * (63 + 2) * 2 = 266,500 bytes > 163,840
    "exact": _ALL - {"mg"},
    # mg: 65,536 free cells, mg_selected() needs nfree <= 0xFFFF (its levels are bounded by the cell count); the V
    # term does not fit either
    "over": _ALL - {"mg"},
    "strip2048x16": _ALL,
    "strip16x2048": _ALL,
    "strip2047x17": _ALL,
    "strip17x2047": _ALL,
}
FITS = {(m, k) for m, ks in _FITS_BY_MAP.items() for k in ks}


def _force(monkeypatch, kernel):
    """Kernel selection is read when a context of the diagnostic build is created. Returns Planner's diag."""
    if kernel == "default":
        return False
    monkeypatch.setenv("TSW_BFS_KERNEL", "blk" if kernel == "blk-pair" else kernel)
    if kernel == "blk-pair":
        monkeypatch.setenv("TSW_BFS_PAIR", "1")
    return True


def _tables_equal(c, p, goals, what):
    got = p.dist_tables(goals)
    for k, g in enumerate(goals):
        ref = c.bfs(g)
        bad = np.flatnonzero(got[k] != ref)
        assert bad.size == 0, (f"{what}: goal {g}: {bad.size} cells differ, first cell {bad[0]} "
                               f"got {got[k][bad[0]]} want {ref[bad[0]]}")
    return got


def _refused(p, goals):
    with pytest.raises(TswapError) as ei:
        p.dist_tables(goals)
    assert ei.value.code == TSW_EINVAL and "does not fit" in str(ei.value)


def _overflows(p, goals):
    with pytest.raises(TswapError) as ei:
        p.dist_tables(np.asarray(goals, dtype=np.uint32))
    assert ei.value.code == TSW_EOVERFLOW, ei.value


def _k1_goals(c):
    if c.name in ("wide", "tall"):
        return lc.snake_goals(c)
    if c.name == "exact":
        return c.order[[0, -1]].astype(np.uint32)
    return lc.strip_goals(c)


@pytest.mark.parametrize("kernel", K1_KERNELS)
@pytest.mark.parametrize("name", [m for m in K1_MAPS if m != "over"])
def test_k1_tables(name, kernel, monkeypatch):
    """wide / tall: both ends of the path, the middle and 5 seeded cells; the table of order[0] holds the oracle's
    2,064 distances of 0x8000 and more (a signed 16-bit slip would fail the equality too: this names it).
    exact: both ends, 65,534 steps apart: a table whose maximum is 0xFFFE, not an overflow.
    Strips: 40 goals, half of them with a coordinate of 1024 or more; two strips have ragged widths."""
    c = lc.case(name)
    goals = _k1_goals(c)
    diag = _force(monkeypatch, kernel)
    with Planner(c.rows, diag=diag) as p:
        if (name, kernel) not in FITS:
            return _refused(p, goals)
        got = _tables_equal(c, p, goals, f"{name} {kernel}")
        assert p.stats()["tables"] == goals.size
    if name in ("wide", "tall"):
        assert np.count_nonzero((got[0] != INF) & (got[0] >= 0x8000)) == 2064
        assert np.count_nonzero(got[0].astype(np.int16) < 0) == 2064 + np.count_nonzero(~c.free)
    if name == "exact":
        assert got[0][c.free].max() == 0xFFFE and got[1][c.free].max() == 0xFFFE


@pytest.mark.parametrize("kernel", K1_KERNELS)
def test_k1_over_the_u16_range(kernel, monkeypatch):
    """`over`: order[0] and order[-1] are 65,535 steps apart, one more than a table holds: TSW_EOVERFLOW, and no
    goal of the failed call stays registered (a level stop that fires one level late would write 0xFFFF as a
    distance and return a wrong table with no error). order[1] is 65,534 from the far end: a table. Then two
    agents step toward the table-less goal."""
    c = lc.case("over")
    o = c.order
    mid = o[o.size // 2]
    diag = _force(monkeypatch, kernel)
    with Planner(c.rows, diag=diag) as p:
        if ("over", kernel) not in FITS:
            return _refused(p, o[:1])
        _overflows(p, [o[0]])
        _overflows(p, [o[-1]])
        _overflows(p, [o[1], o[0]])
        assert p.stats()["tables"] == 0
        got = _tables_equal(c, p, np.array([o[1], mid], dtype=np.uint32), f"over {kernel}")
        assert got[0][c.free].max() == 0xFFFE and got[1][c.free].max() == 32768
        assert p.stats()["tables"] == 2
        v = np.array([o[-1], o[10]], dtype=np.uint32)
        g = np.array([o[0], o[0]], dtype=np.uint32)
        rv, rg = _once(("over-step",), lambda: c.og.step(v, g))
        hv, hg = p.step(v, g)
        assert np.array_equal(hv, rv) and np.array_equal(hg, rg)
        assert rv[0] == o[-2] and rv[1] == o[9]
        assert p.stats()["tableless_goals"] >= 1


@pytest.mark.parametrize("name", sorted(lc.FULL))
def test_k1_full_size(name):
    """2^20 cells, not square: the first and the last free cell (id 1,048,574) and 2 seeded goals, default chain."""
    c = lc.case(name)
    with Planner(c.rows) as p:
        _tables_equal(c, p, lc.full_goals(c), name)


# ---- K3 through tsw_get_path_next -------------------------------------------------------------------------------

K3_MODES = {
    "product": None,
    "serial": {"TSW_ASTAR_SERIAL": "1"},
    "no-tier2": {"TSW_ASTAR_NO_TIER2": "1"},
    "global-gs": {"TSW_ASTAR_GLOBAL_GS": "1"},
    "lds-gs": {"TSW_ASTAR_GLOBAL_GS": "0"},
    "hcap16": {"TSW_ASTAR_WAVE_HCAP": "16"},
}


def _mode(monkeypatch, mode):
    for k, v in (K3_MODES[mode] or {}).items():
        monkeypatch.setenv(k, v)
    return K3_MODES[mode] is not None


def _path_ref(c, key, s, g):
    def make():
        r = [c.og.get_path_next(int(a), int(b))[:2] for a, b in zip(s, g)]
        return np.array([x[0] for x in r], dtype=np.uint32), np.array([x[1] for x in r], dtype=np.int32)

    return _once((c.name, key), make)


def _paths_equal(c, p, s, g, ref, what):
    nxt, ln = p.get_path_next(s, g)
    bad = np.flatnonzero((nxt != ref[0]) | (ln != ref[1]))
    assert bad.size == 0, (f"{what}: {bad.size} of {s.size} queries differ; first {s[bad[0]]} -> {g[bad[0]]}: next "
                           f"{nxt[bad[0]]} len {ln[bad[0]]}, oracle next {ref[0][bad[0]]} len {ref[1][bad[0]]}")


@pytest.mark.parametrize("mode", list(K3_MODES))
@pytest.mark.parametrize("name", ["snake_room", "snake_room_t"])
def test_k3_hand_off_at_g15(name, mode, monkeypatch):
    """64 queries from the head of the snake to room cells: the search reaches the room with g near 2^15 and
    crosses it (or, for at least an eighth of them, stays below it) with the room's frontier in the heap; `len`
    itself is 32,769 or more. Plus the exact boundary along the snake: lengths 32,768 (g = 32,767, the last the
    15-bit field holds) and 32,769, in both directions."""
    c = lc.case(name)
    s, g = lc.room_queries(c)
    bs, bg, bl = lc.boundary_pairs(c)
    s, g = np.concatenate([s, bs]), np.concatenate([g, bg])
    ref = _path_ref(c, "room", s, g)
    assert ref[1][-4:].tolist() == bl.tolist()
    diag = _mode(monkeypatch, mode)
    with Planner(c.rows, diag=diag) as p:
        _paths_equal(c, p, s, g, ref, f"{name} {mode}")


@pytest.mark.parametrize("mode", ["product", "serial"])
@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_k3_strip_pairs(name, mode, monkeypatch):
    """300 pairs whose start has a coordinate of 1024 or more, the goal within Manhattan 150; the last 8 goals lie
    in another component (the fallback's coordinate comparisons)."""
    c = lc.case(name)
    s, g = lc.strip_pairs(c)
    ref = _path_ref(c, "pairs", s, g)
    diag = _mode(monkeypatch, mode)
    with Planner(c.rows, diag=diag) as p:
        _paths_equal(c, p, s, g, ref, f"{name} {mode}")


@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_k3_strip_eager_tables(name):
    """TSW_F_EAGER_NEXTHOP tables of 2 goals, at 400 sampled free cells with a coordinate of 1024 or more, against
    get_path (per pair: the oracle's whole-table call takes a quarter of a minute per goal on these maps)."""
    c = lc.case(name)
    goals, at = lc.eager_goals(c), lc.high_cells(c)
    want = _once((name, "eager"), lambda: np.array([[c.code(a, goal) for a in at] for goal in goals], dtype=np.uint8))
    with Planner(c.rows, flags=TSW_F_EAGER_NEXTHOP) as p:
        tabs = p.next_hop_tables(goals)
    for k, goal in enumerate(goals):
        bad = np.flatnonzero(tabs[k][at] != want[k])
        assert bad.size == 0, (f"{name}: goal {goal}: {bad.size} of {at.size} codes differ, first cell {at[bad[0]]} "
                               f"got {tabs[k][at[bad[0]]]} want {want[k][bad[0]]}")
        assert (tabs[k][~c.free] == 0xFF).all()


@pytest.mark.parametrize("name", sorted(lc.FULL))
def test_k3_full_size_last_cells(name):
    """32 pairs within Manhattan 150 of the last free cell: cell ids next to 2^20."""
    c = lc.case(name)
    s, g = lc.full_pairs(c)
    ref = _path_ref(c, "pairs", s, g)
    with Planner(c.rows) as p:
        _paths_equal(c, p, s, g, ref, name)


@pytest.mark.parametrize("name", sorted(lc.LINES))
def test_k3_lds_heap_fields(name):
    """k_astar_lds (1024 cells, entry f:11 | g:10 | cell:11). Open line: every pair among cells 0, 1, 511, 512, 1022,
    1023: lengths up to 1,024, so g = 1023. Walled line: 1021 -> 1023 runs to cell 0 (f = 2044) and stays; 0 -> 1023
    takes the fallback."""
    c = lc.case(name)
    s, g = lc.walled_line_pairs() if name.startswith("w") else lc.line_pairs()
    ref = _path_ref(c, "line", s, g)
    if name.startswith("w"):
        assert ref[0].tolist() == [1021, c.W if c.vertical else 1]
    else:
        assert ref[1].max() == 1024
    with Planner(c.rows) as p:
        _paths_equal(c, p, s, g, ref, name)


# ---- planning at high coordinates -------------------------------------------------------------------------------

def _plan_equal(p, starts, tasks, max_t, ref, what):
    rrec, rgoal = ref
    rec, goal = p.plan_mapd_arrays(starts, tasks, max_t, trace_goals=True)
    assert rec.shape == rrec.shape, what
    if not np.array_equal(goal, rgoal):
        t = int(np.argmax((goal != rgoal).any(axis=0)))
        i = int(np.argmax(goal[:, t] != rgoal[:, t]))
        pytest.fail(f"{what}: goals diverge first at t={t}, agent {i}: {goal[i, t]} != {rgoal[i, t]}")
    if not np.array_equal(rec, rrec):
        t = int(np.argmax((rec != rrec).any(axis=0)))
        i = int(np.argmax(rec[:, t] != rrec[:, t]))
        pytest.fail(f"{what}: records diverge first at t={t}, agent {i}: {rec[i, t]:#x} != {rrec[i, t]:#x}")


@pytest.mark.parametrize("flags", [0, TSW_F_EXIT_MODE], ids=["coop", "exit"])
@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_plan_strip_window(name, flags):
    """48 agents and 96 tasks in the part of the strip past coordinate 1100, 80 steps (all of them move agents):
    records (tsw_rec's x and y out of k_plan) and goals == the oracle's."""
    c = lc.case(name)
    starts, tasks, max_t = lc.strip_plan_instance(c)
    ref = _once((name, "plan"), lambda: c.og.mapd(starts, tasks, max_t, trace_goals=True))
    assert lc.rec_xy(ref[0])[1 if c.vertical else 0].max() >= 1980
    with Planner(c.rows, flags=flags) as p:
        _plan_equal(p, starts, tasks, max_t, ref, f"{name} flags {flags}")
        assert p.stats()["watchdog_fires"] == 0


@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_step_strip_window(name):
    """Five chained tsw_step calls on the same starts with seeded goals == OracleGraph.step."""
    c = lc.case(name)
    v, g = lc.strip_step_instance(c)
    with Planner(c.rows) as p:
        for k in range(5):
            rv, rg = _once((name, "step", k), lambda: c.og.step(v, g))
            hv, hg = p.step(v, g)
            dv, dg = np.flatnonzero(hv != rv), np.flatnonzero(hg != rg)
            assert dv.size == 0 and dg.size == 0, f"{name} step {k}: v differs at agents {dv[:8]}, g at {dg[:8]}"
            v, g = rv, rg


ROOM_PLANS = [
    ("coop", False, {}, {}),
    ("host-off", False, {"host_astar": TSW_HOST_ASTAR_OFF}, {}),
    ("exit", False, {"flags": TSW_F_EXIT_MODE}, {}),
    ("worker-gs0", True, {}, {"TSW_WORKER_GS": "0"}),
]


@pytest.mark.parametrize("what,diag,kw,env", ROOM_PLANS, ids=[r[0] for r in ROOM_PLANS])
def test_plan_snake_room(what, diag, kw, env, monkeypatch):
    """12 agents in the room heading for pickups at the far end of the snake, 32,783 steps and more away: next hops
    decided among several candidates at distances of 2^15 and more, by the K3 workers inside the dispatch (with
    the host service, without it, with global g-scores) and by the exit mode's host-launched passes."""
    c = lc.case("snake_room")
    starts, tasks, max_t = lc.room_plan_instance()
    ref = _once(("snake_room", "plan"), lambda: c.og.mapd(starts, tasks, max_t, trace_goals=True))
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    with Planner(c.rows, diag=diag, **kw) as p:
        _plan_equal(p, starts, tasks, max_t, ref, f"snake_room {what}")
        st = p.stats()
    assert st["watchdog_fires"] == 0
    if what == "host-off":
        assert st["host_astar_queries"] == 0


@pytest.mark.parametrize("name", ["strip2048x16", "strip16x2048"])
def test_fleet_at_high_coordinates(name):
    """tsw_nearby == the brute-force lists and tsw_decide_fleet == the oracle's decisions (as test_gpu_fleet.py
    checks them) for a recipe fleet standing on the half of the strip with coordinates of 1024 and more."""
    c = lc.case(name)
    v, g, _ = lc.high_fleet(c)
    boff, bidx = fc.brute_nearby(v, c.W, 15)
    ref = _once((name, "fleet"), lambda: fc.oracle_fleet(c.og, v, g, boff, bidx))
    with Planner(c.rows) as p:
        off, idx = p.nearby(v, 15)
        assert off.dtype == np.uint32 and idx.dtype == np.uint32
        assert np.array_equal(off, boff) and np.array_equal(idx, bidx)
        got = p.decide_fleet(v, g, 15)
    for what, a, b in zip(("act", "cell", "partner", "part_off", "part"), got, ref):
        assert a.dtype == np.uint32 and a.shape == b.shape and np.array_equal(a, b), \
            f"{name} {what}: first difference at {int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else 'shape'}"
    assert ref[3][-1] > 0  # rotations: the participant translation runs
