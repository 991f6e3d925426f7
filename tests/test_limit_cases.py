"""CPU: the premises tests/test_gpu_limits.py rests on, from the oracle alone, so that none of its cases can pass
vacuously: the maps of tests/limit_cases.py put distances at both sides of 0x8000 and of the u16 range, their
queries cross g = 2^15 inside a wide frontier, and their plans move agents at coordinates of 1024 and more. Also
the checks of this area that need no GPU: the host A* on these maps, and tsw_create's refusal of grids past
2048 per side or 2^20 cells."""
import os

import numpy as np
import pytest

import limit_cases as lc
import p2p_distributed_tswap_amd as pkg
from p2p_distributed_tswap_amd import Planner, TswapError, maps

INF = lc.INF


def _lib_or_skip():
    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("libtswap_hip.so not built (run __graft_entry__.build())")


# ---- 1: the table of maps -------------------------------------------------------------------------------------

def test_snake_layout_small():
    """The recipe itself on 5 x 5: gaps alternate east / west, order walks every free cell once by unit steps, keep
    blocks the tail, and the transposed map is the same map with x and y exchanged."""
    rows, order = lc.snake(5, 5)
    assert rows == [".....", "@@@@.", ".....", ".@@@@", "....."]
    assert order.tolist() == [0, 1, 2, 3, 4, 9, 14, 13, 12, 11, 10, 15, 20, 21, 22, 23, 24]
    rows, order = lc.snake(5, 5, keep=13)
    assert rows == [".....", "@@@@.", ".....", ".@@@@", ".@@@@"] and order.size == 13 and order[-1] == 20
    trows, torder = lc.snake(5, 5, keep=13, transpose=True)
    assert trows == ["".join(r[x] for r in rows) for x in range(5)]
    assert [(c // 5, c % 5) for c in torder.tolist()] == [(c % 5, c // 5) for c in order.tolist()]


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_wide_and_tall_cross_0x8000(name):
    c = lc.case(name)
    assert (c.W, c.H) == ((2048, 33) if name == "wide" else (33, 2048))
    o = c.order
    assert np.count_nonzero(c.free) == o.size == 34832 and np.unique(o).size == o.size
    D = c.bfs(o[0])
    assert D[o[-1]] == 34831 and np.array_equal(D[o], np.arange(o.size))
    assert np.count_nonzero((D != INF) & (D >= 0x8000)) == 2064
    goals = lc.snake_goals(c)
    assert np.unique(goals).size == 8 and c.free[goals].all()
    assert c.long_coord(o).max() == 2047


def test_exact_and_over_straddle_the_u16_range():
    """`exact`: the farthest cell is 65,534 = 0xFFFE steps away, the largest distance a table holds. `over`: one cell
    more, 65,535 steps = the INF sentinel itself: the oracle's u16 BFS returns 0xFFFF there and is no reference
    for that goal; from order[1] the farthest cell is at 65,534 again."""
    e, o = lc.case("exact"), lc.case("over")
    assert (e.W, e.H) == (o.W, o.H) == (2048, 63)
    assert np.count_nonzero(e.free) == e.order.size == 65535
    assert np.count_nonzero(o.free) == o.order.size == 65536
    assert e.bfs(e.order[0])[e.order[-1]] == 65534 == 0xFFFE == e.bfs(e.order[-1])[e.order[0]]
    for k in (0, -1):
        assert e.bfs(e.order[k])[e.free].max() == 0xFFFE
        # the cell 65,535 steps away comes back as the sentinel, every other one exact
        D = o.bfs(o.order[k])
        far = o.order[-1 - k] if k == 0 else o.order[0]
        assert D[far] == INF and np.count_nonzero(D[o.free] == INF) == 1
        path = o.order if k == 0 else o.order[::-1]
        assert np.array_equal(D[path[:-1]], np.arange(65535))
    D1 = o.bfs(o.order[1])
    assert D1[o.free].max() == 0xFFFE and D1[o.order[-1]] == 0xFFFE and D1[o.order[0]] == 1
    mid = o.order[o.order.size // 2]
    assert o.bfs(mid)[o.free].max() == 32768


@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_strips(name):
    c = lc.case(name)
    w, h = lc.STRIPS[name]
    assert c.rows == maps.random_map(w, h, 0.2, lc.SEED)  # the numpy splitmix64 stream is maps.random_map's
    assert (w % 8 == 0) == (name in ("strip2048x16", "strip16x2048"))  # the ragged ones: no 16-byte store path
    goals = lc.strip_goals(c)
    assert np.unique(goals).size == 40 and c.free[goals].all()
    assert np.count_nonzero(c.long_coord(goals) >= lc.HALF) == 20
    s, g = lc.strip_pairs(c)
    assert c.free[s].all() and c.free[g].all() and (c.long_coord(s) >= lc.HALF).all()
    man = np.abs(s.astype(np.int64) % c.W - g % c.W) + np.abs(s.astype(np.int64) // c.W - g // c.W)
    assert man.max() <= 150 and man.min() >= 1
    cross = sum(1 for a, b in zip(s[-8:], g[-8:]) if c.bfs(b)[a] == INF)
    assert cross >= 4  # pairs across components: the fallback's coordinate comparisons
    hi = lc.high_cells(c)
    assert np.unique(hi).size == 400 and (c.long_coord(hi) >= lc.HALF).all()
    assert (c.long_coord(lc.eager_goals(c)) >= lc.HALF).all()


@pytest.mark.parametrize("name", sorted(lc.FULL))
def test_full_size(name):
    c = lc.case(name)
    assert c.W * c.H == 1 << 20 and c.W != c.H
    assert c.free_ids[-1] == 1048574
    goals = lc.full_goals(c)
    assert goals[0] == c.free_ids[0] and goals[1] == 1048574 and np.unique(goals).size == 4
    s, g = lc.full_pairs(c)
    assert c.free[s].all() and c.free[g].all() and min(s.min(), g.min()) > (1 << 20) - 151 * max(c.W, 151)
    w, h = lc.FULL[name]
    assert lc.random_map(w // 64, h // 64, 0.1, lc.SEED) == maps.random_map(w // 64, h // 64, 0.1, lc.SEED)


def test_lines_reach_the_lds_fields():
    """k_astar_lds packs f:11 | g:10 | cell:11: on the open 1024-cell line the longest path has 1,024 cells
    (g = 1023, all ten bits); on the walled one the search from 1021 for 1023 runs to cell 0, where
    f = g + h = 1021 + 1023 = 2044."""
    for name in ("line1024x1", "line1x1024"):
        c = lc.case(name)
        assert c.W * c.H == 1024 and c.free.all()
        s, g = lc.line_pairs()
        ln = [c.og.get_path_next(int(a), int(b))[1] for a, b in zip(s, g)]
        assert max(ln) == 1024 and s.size == 36
    for name in ("wline1024x1", "wline1x1024"):
        c = lc.case(name)
        assert np.flatnonzero(~c.free).tolist() == [1022]
        s, g = lc.walled_line_pairs()
        step = c.W if c.vertical else 1
        assert c.og.get_path_next(1021, 1023)[0] == 1021   # no neighbour is closer: stay
        assert c.og.get_path_next(0, 1023)[0] == step      # fallback toward the goal
        assert c.bfs(0)[1021] + abs(1023 - 0) == 2044


# ---- 2: the query mix of snake_room -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["snake_room", "snake_room_t"])
def test_room_queries_straddle_g15(name):
    c = lc.case(name)
    assert (c.W, c.H) == ((2048, 48) if name == "snake_room" else (48, 2048))
    assert c.order.size == 32783
    s, g = lc.room_queries(c)
    assert s.size == 64
    ln = np.array([c.og.get_path_next(int(a), int(b))[1] for a, b in zip(s, g)])
    over, under = int(np.count_nonzero(ln >= lc.G15 + 1)), int(np.count_nonzero(ln < lc.G15 + 1))
    print(f"{name}: {over} of 64 queries cross g = 2^15, {under} do not (lengths {ln.min()}..{ln.max()})")
    assert over >= 16 and under >= 8 and ln.min() > 0
    # g crosses 2^15 inside the room: the goals are room cells and the snake alone is 32,783 - k cells long
    room = lc.room_cells(c)
    assert np.isin(g, room).all() and room.size > 20000
    # the exact boundary, along the snake
    bs, bg, bl = lc.boundary_pairs(c)
    assert [c.og.get_path_next(int(a), int(b))[1] for a, b in zip(bs, bg)] == bl.tolist() == [32768, 32769, 32768, 32769]


# ---- 3: the plan instances ------------------------------------------------------------------------------------

def test_room_plan_instance():
    """The snake_room plan: every agent starts 300..1200 steps from the door, and at least 16 (agent, step) next
    hops are decided among several candidates at a distance of 32,768 or more from the goal."""
    c = lc.case("snake_room")
    starts, tasks, max_t = lc.room_plan_instance()
    assert starts.shape == (12, 2) and tasks.shape == (24, 4) and max_t == 8
    st = starts[:, 1] * c.W + starts[:, 0]
    d = c.bfs(int(c.order[-1]) + c.W)[st]
    assert np.unique(st).size == 12 and d.min() >= 300 and d.max() <= 1200
    assert np.array_equal(tasks[:, 1] * c.W + tasks[:, 0], c.order[:24])
    assert np.isin(tasks[:, 3] * c.W + tasks[:, 2], lc.room_cells(c)).all()
    rec, goal = c.og.mapd(starts, tasks, max_t, trace_goals=True)
    assert rec.shape == (12, max_t + 1) and maps.moving_timesteps(rec) == max_t
    x, y = lc.rec_xy(rec)
    pos = y * c.W + x
    hits = sum(1 for i in range(12) for t in range(max_t)
               if pos[i, t] != goal[i, t] and c.bfs(goal[i, t])[pos[i, t]] >= lc.G15
               and lc.multi_candidate(c, int(pos[i, t]), int(goal[i, t])))
    print(f"snake_room plan: {hits} of {12 * max_t} next hops are multi-candidate at distance >= 32768")
    assert hits >= 16


@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_strip_plan_instance_moves_at_high_coordinates(name):
    c = lc.case(name)
    starts, tasks, max_t = lc.strip_plan_instance(c)
    assert starts.shape == (48, 2) and tasks.shape == (96, 4)
    k = 1 if c.vertical else 0
    assert starts[:, k].min() >= 1100 and tasks[:, [k, k + 2]].min() >= 1100
    rec, _ = c.og.mapd(starts, tasks, max_t)
    assert rec.shape[1] == max_t + 1 and maps.moving_timesteps(rec) == max_t
    far = lc.rec_xy(rec)[k]
    print(f"{name}: largest coordinate in the records {far.max()}")
    assert far.min() >= 1024 and far.max() >= 1980
    v, g = lc.strip_step_instance(c)
    assert np.unique(v).size == 48 and c.free[g].all() and (c.long_coord(g) >= 1100).all()
    moved = 0
    for _ in range(5):
        v2, g = c.og.step(v, g)
        moved += int(np.count_nonzero(v2 != v))
        v = v2
    assert moved >= 48


@pytest.mark.parametrize("name", ["strip2048x16", "strip16x2048"])
def test_high_fleet(name):
    """The fleet of the nearby / decide tests stands at coordinates >= 1024, its lists are not empty, and its
    decisions include moves, waits and the rotations of the recipe's loops (90 agents on 16,000 cells are too
    sparse for a goal swap: the small maps of test_gpu_fleet.py have those)."""
    import fleet_cases as fc

    c = lc.case(name)
    v, g, rings = lc.high_fleet(c)
    assert rings == 6 and c.free[v].all() and c.free[g].all()
    assert (c.long_coord(v) >= lc.HALF).all() and (c.long_coord(g) >= lc.HALF).all()
    off, idx = fc.brute_nearby(v, c.W, 15)
    assert off[-1] >= 2 * v.size
    act, _, _, part_off, _ = fc.oracle_fleet(c.og, v, g, off, idx)
    assert {0, 2, 3} <= set(np.unique(act).tolist()) and part_off[-1] > 0


# ---- 4: the host A* -------------------------------------------------------------------------------------------

def _host_vs_oracle(c, s, g):
    got = pkg.host_next_hop_codes(c.rows, s, g)
    want = np.array([c.code(a, b) for a, b in zip(s, g)], dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{c.name}: {bad.size} of {s.size} differ; first: start {s[bad[0]]} goal {g[bad[0]]} "
                           f"host {got[bad[0]]} oracle {want[bad[0]]}")


@pytest.mark.parametrize("name", ["snake_room", "snake_room_t"])
def test_host_astar_room_queries(name):
    _lib_or_skip()
    c = lc.case(name)
    s, g = lc.room_queries(c)
    bs, bg, _ = lc.boundary_pairs(c)
    _host_vs_oracle(c, np.concatenate([s, bs]), np.concatenate([g, bg]))


@pytest.mark.parametrize("name", sorted(lc.STRIPS))
def test_host_astar_strip_pairs(name):
    _lib_or_skip()
    c = lc.case(name)
    _host_vs_oracle(c, *lc.strip_pairs(c))


# ---- 5: tsw_create's limits -----------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(2049, 1), (1, 2049), (1025, 1024)])
def test_create_refuses_grids_past_the_limits(w, h):
    """include/tswap.h: at most 2048 per side and 2^20 cells. The check precedes the device lookup, so the refusal
    names the limit (not a missing device) on any machine."""
    _lib_or_skip()
    with pytest.raises(TswapError) as ei:
        Planner(np.full((h, w), ord("."), dtype=np.uint8))
    assert "2048" in str(ei.value) and "2^20" in str(ei.value)
