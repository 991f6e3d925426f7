"""CPU: the premises tests/test_gpu_workers.py rests on, so that none of its cases can pass vacuously — the
class-selected step instances hold every detour class, their A* heaps outgrow the workers' register heap,
and the plan instances move in every step."""
import numpy as np
import pytest

import worker_cases as wc
from p2p_distributed_tswap_amd import maps
from oracle import OracleGraph


@pytest.fixture(scope="module", params=[(120, 100), (200, 130)], ids=["120x100", "200x130"])
def step_inst(request):
    rows = wc.serpentine(*request.param)
    v, g = wc.step_instance(rows)
    return rows, v, g


def test_serpentine_is_the_parity_suite_map():
    """serpentine(200, 130) is the map of test_gpu_parity._grid("serpentine"), restated."""
    a = np.zeros((130, 200), dtype=bool)
    for i, x in enumerate(range(3, 200, 4)):
        a[:, x] = True
        a[(1 if i % 2 else 128), x] = False
    assert wc.serpentine(200, 130) == maps.to_rows(a)
    # 12,000 cells: above the 4,096-cell eager limit, all three g-score placements fit (u32 LDS <= 24k cells);
    # 26,000 cells: past the u32 LDS g-scores
    assert 4096 < 120 * 100 <= 24 * 1024 < 200 * 130


def test_detour_classes_against_a_plain_bfs_scan():
    """detour_classes' vectorised candidate count == a per-cell loop over the oracle's BFS table."""
    rows = wc.serpentine(24, 14)
    cells = maps.rows_to_array(rows)
    H, W = cells.shape
    og = OracleGraph(cells)
    goal = 1 * W + 1
    delta, multi = wc.detour_classes(og, cells, goal)
    D = og.bfs(goal)
    for c in range(W * H):
        x, y = c % W, c // W
        if cells[y, x] == ord("@"):
            assert delta[c] == -1 and not multi[c]
            continue
        assert 2 * delta[c] == int(D[c]) - abs(x - 1) - abs(y - 1)
        n = sum(1 for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0))
                if 0 <= x + dx < W and 0 <= y + dy < H and cells[y + dy, x + dx] != ord("@")
                and int(D[(y + dy) * W + x + dx]) == int(D[c]) - 1)
        assert bool(multi[c]) == (n >= 2)
    assert multi.any() and delta.max() > 8


def test_step_instance_classes(step_inst):
    """Every delta class holds >= 16 agents, every agent's cell is multi-candidate for its goal (so its code is
    0xFF after K1 and a worker's A* answers it), agent cells are distinct and nobody starts at its goal."""
    rows, v, g = step_inst
    delta, multi = wc.instance_classes(rows, v, g)
    assert np.unique(v).size == v.size and np.unique(g).size == 8
    assert multi.all() and (v != g).all()
    sizes = {c: int(np.count_nonzero(delta == c)) for c in wc.CLASSES}
    print(f"{v.size} agents, per class {sizes}")
    assert min(sizes.values()) >= 16, sizes
    # the instance is deterministic
    v2, g2 = wc.step_instance(rows)
    assert np.array_equal(v, v2) and np.array_equal(g, g2)


def test_saturation_instance_needs_the_exit_switched_off():
    """The premise of the saturated GPU case: with the early exit tested after every 2nd pop (TSW_DAG_MASK=1), a
    byte test that does not switch off at a start whose byte is 255 answers >= 16 of the instance's delta = 255
    pairs wrongly (DAG cells with byte 255 are invisible to it), where the test as specified agrees with get_path."""
    rows = wc.serpentine(120, 100)
    v, g = wc.saturation_instance(rows)
    delta, multi = wc.instance_classes(rows, v, g)
    assert np.unique(v).size == v.size and multi.all()
    assert np.array_equal(np.unique(g), np.unique(wc.step_instance(rows)[1]))
    assert all(np.count_nonzero(delta == c) >= 16 for c in (254, 255, 256))
    ref = wc.MapRef(rows)
    wrong = []
    for goal in np.unique(g):
        d, _ = wc.detour_classes(ref.og, ref.cells, int(goal))
        det = np.where(d < 0, 255, np.minimum(d, 255))
        for a in v[(g == goal) & (delta == 255)]:
            want = int(ref.astar_codes([(int(a), int(goal))])[0])
            if wc.byte_exit_model(rows, det, int(a), int(goal), 1, off_when_saturated=False) != want:
                wrong.append((int(a), int(goal), det, want))
    print(f"{len(wrong)} of {np.count_nonzero(delta == 255)} delta = 255 pairs go wrong without the switch")
    assert len(wrong) >= 16
    for a, goal, det, want in wrong[:6]:
        assert wc.byte_exit_model(rows, det, a, goal, 1) == want


def _over(peaks, what):
    over = sum(1 for p in peaks if p > 64)
    print(f"{what}: {over} of {len(peaks)} heaps peak above 64 entries (max {max(peaks)})")
    return over


def test_heap_peaks_step_instance():
    """A quarter or more of a seeded sample of the serpentine step instance outgrows 64 heap entries: the 63-entry
    register heap spills, and a 64-entry LDS heap (TSW_ASTAR_WAVE_HCAP=64) overflows to tier 3."""
    rows = wc.serpentine(120, 100)
    v, g = wc.step_instance(rows)
    idx = np.random.default_rng(1).choice(v.size, 60, replace=False)
    assert 4 * _over(wc.heap_peaks(rows, v[idx], g[idx]), "serpentine 120x100 step instance") >= 60


def test_heap_peaks_cave_plan():
    rows, starts, tasks, _ = wc.plan_cave()
    a, b = wc.plan_pairs(rows, starts, tasks, 60, 1)
    assert 4 * _over(wc.heap_peaks(rows, a, b), "cave 128x97 plan instance") >= 60


@pytest.mark.parametrize("inst", [wc.plan_serpentine, wc.plan_cave], ids=["serpentine", "cave"])
def test_plan_instances_move_every_step(inst):
    rows, starts, tasks, max_t = inst()
    assert len(rows) * len(rows[0]) > 4096  # lazy next hops: the plan runs workers
    rec, _ = OracleGraph(maps.rows_to_array(rows)).mapd(starts, tasks, max_t)
    assert rec.shape[1] == max_t + 1
    assert maps.moving_timesteps(rec) == max_t


@pytest.mark.parametrize("rows,ngoals,pockets", [(maps.cave_map(40, 41, 3), 12, True), (wc.serpentine(24, 14), 12, False),
                                                 (maps.random_map(24, 24, 0.3, 11), 12, True)],
                         ids=["cave", "serpentine", "random"])
def test_mapref_restates_orc_next_codes(rows, ngoals, pockets):
    """The store checker's reference (BFS-decided codes and fallbacks from numpy, the rest from get_path, asked in
    one batch so that the thread pool runs) == orc_next_codes cell for cell; two of the maps have cells that do
    not reach the goal."""
    ref = wc.MapRef(rows)
    goals = [int(g) for g in np.random.default_rng(3).choice(np.flatnonzero(ref.free), ngoals, replace=False)]
    pairs = [(int(c), g) for g in goals for c in np.flatnonzero(ref.k1(g) == wc.ASTAR)]
    assert len(pairs) >= 512  # two threads or more
    ref.astar_codes(pairs)
    assert ref.oracle_calls == len(pairs)
    unreachable = 0
    for g in goals:
        assert np.array_equal(ref.next_codes(g), ref.og.next_codes(g)), g
        unreachable += int(np.count_nonzero(ref.free & (ref.og.bfs(g) == wc.INF)))
    assert ref.oracle_calls == len(pairs)  # memoised
    assert (unreachable > 0) == pockets
