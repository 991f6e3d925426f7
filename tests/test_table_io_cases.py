"""CPU: the store audit of tests/table_io_cases.py cannot pass vacuously — its K1 model agrees with the
oracle's own codes wherever one neighbour decides, and a table with one wrong code or one pending marker
fails it. No GPU use."""
import numpy as np
import pytest

import table_io_cases as tc
from worker_cases import ASTAR, NH_UNKNOWN

FAILS = (AssertionError, pytest.fail.Exception)


class _FakeStore:
    """Stands in for a Planner: next_hop_tables(goals) from a dict of tables."""

    def __init__(self, tabs):
        self.tabs = tabs

    def next_hop_tables(self, goals):
        return np.stack([self.tabs[int(g)] for g in goals])


def _oracle_store(name):
    ref, goals = tc.grid_ref(name), tc.grid_goals(name)
    return ref, goals, {int(g): ref.og.next_codes(int(g)) for g in goals}


def test_k1_model_agrees_with_oracle_on_single_candidate_cells():
    ref, goals, tabs = _oracle_store("rand33x17")
    multi = 0
    for g in goals:
        k1, want = ref.k1(int(g)), tabs[int(g)]
        single = k1 != ASTAR
        assert np.array_equal(k1[single], want[single]), f"goal {g}"
        assert (want[ref.free] <= 4).all() and (want[~ref.free] == NH_UNKNOWN).all()
        multi += int(np.count_nonzero(~single))
    assert multi > 0  # the map has cells the A* decides, so the audit's second half runs too


def test_audit_passes_on_the_oracle_tables_full_and_lazy():
    ref, goals, tabs = _oracle_store("rand33x17")
    _, ug, n = tc.check_store(_FakeStore(tabs), ref, goals, "full")
    assert np.array_equal(ug, np.unique(goals)) and n > 0
    lazy = {g: np.where(ref.k1(g) == ASTAR, NH_UNKNOWN, t).astype(np.uint8) for g, t in tabs.items()}
    assert tc.check_store(_FakeStore(lazy), ref, goals, "lazy")[2] == 0


@pytest.mark.parametrize("kind", ["bfs-decided", "astar-decided", "blocked", "k1-missing"])
def test_audit_fails_on_one_flipped_code(kind):
    ref, goals, tabs = _oracle_store("rand33x17")
    g = int(goals[3])
    k1 = ref.k1(g)
    t = tabs[g].copy()
    if kind == "blocked":
        t[np.flatnonzero(~ref.free)[0]] = 1
    elif kind == "k1-missing":
        t[np.flatnonzero(ref.free & (k1 <= 3))[0]] = NH_UNKNOWN
    else:
        c = np.flatnonzero(ref.free & ((k1 == ASTAR) if kind == "astar-decided" else (k1 <= 3)))[-1]
        t[c] = (int(t[c]) + 1) % 4
    with pytest.raises(FAILS):
        tc.check_store(_FakeStore({**tabs, g: t}), ref, goals, kind)


@pytest.mark.parametrize("marker", [tc.NH_PENDING, tc.NH_PENDING_S])
def test_audit_fails_on_one_pending_marker(marker):
    ref, goals, tabs = _oracle_store("rand33x17")
    g = int(goals[0])
    t = tabs[g].copy()
    t[np.flatnonzero(ref.free & (ref.k1(g) == ASTAR))[0]] = marker
    with pytest.raises(FAILS, match="pending"):
        tc.check_store(_FakeStore({**tabs, g: t}), ref, goals, "marker")


def test_grids_have_the_sizes_the_cases_are_about():
    sizes = {n: (len(r[0]), len(r)) for n, r in ((n, f()) for n, f in tc.GRIDS.items())}
    assert sizes["rand33x17"][0] * sizes["rand33x17"][1] % 2 == 1
    assert sizes["rand100x31"][0] * sizes["rand100x31"][1] % 8 == 4
    assert sizes["rand64x20"][0] % 32 == 0 and sizes["rand64x20"][0] * sizes["rand64x20"][1] % 8 == 0
    w, h = sizes["rand70x130"]
    assert (w + 31) // 32 * h > 256 and w % 32 != 0  # more row words than one ring step, ragged last word
    for name in tc.GRIDS:
        assert tc.grid_goals(name).size == 13 and tc.grid_ref(name).free[tc.grid_goals(name)].all()
