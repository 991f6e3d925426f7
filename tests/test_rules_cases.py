"""CPU: every built state of rules_cases.py is what its name says. For each case the counting restatement of
tswap.rs:180-252 ends with OracleGraph.step's goals, the positions the oracle returns are what the builder's docstring
says, and the restatement's counters (firings in order, rule-3 cascade length, firings per 64-agent chunk, swaps that
close a cycle, rotations per cycle) reach what the case is named for. test_gpu_rules.py runs the same cases through
k_plan and compares the kernel's counters with these."""
import numpy as np
import pytest

import rules_cases as rc


def _exp(name):
    c = rc.case(name)
    e = rc.expected(c)
    assert e["restated_ok"], f"{name}: the restatement's goals differ from the oracle's"
    if c.moved is not None:
        assert e["moved"] == c.moved, f"{name}: {e['moved']} agents moved, the case says {c.moved}"
    return c, e, e["counters"]


def test_names_are_unique_and_small():
    assert len(set(rc.NAMES)) == len(rc.NAMES)
    for name in rc.NAMES:
        c = rc.case(name)
        assert c.name == name
        assert c.n <= 1100 and len(c.rows) <= 66 and len(c.rows[0]) <= 131, name
        assert len(set(c.v.tolist())) == c.n, f"{name}: two agents on one cell"


@pytest.mark.parametrize("name", rc.RING_NAMES)
def test_ring(name):
    c, e, C = _exp(name)
    if name == "rings2":
        assert sorted(C.rot_per_cycle.values()) == [1, 3]
        assert sorted(len(k) for k in C.rot_per_cycle) == [116, 132]
        assert np.all(e["g"] != c.g)
    else:
        L, d = int(name.split("-")[1]), int(name.split("-")[2][1:])
        assert C.firings == [(a, 4, L) for a, _, _ in C.firings] and C.n == d
        assert list(C.rot_per_cycle.values()) == [d]
        assert int(np.count_nonzero(e["g"] != c.g)) == L  # all L goals change
        if name.endswith("spread"):
            members = next(iter(C.rot_per_cycle))
            assert 0 not in C.per_chunk and all(a >= rc.CHUNK for a in members)
            assert len({a // rc.CHUNK for a in members}) == min(L, rc.SPREAD_CHUNKS)  # one member (or more) a chunk
            assert c.n == rc.CHUNK * (rc.SPREAD_CHUNKS + 1)
    assert np.array_equal(e["v"], e["g"]) and np.array_equal(e["v"], c.v)  # everyone on its goal, nobody moved


@pytest.mark.parametrize("name", rc.CASCADE_NAMES)
def test_cascade(name):
    c, e, C = _exp(name)
    K, order = int(name.split("-")[1]), name.split("-")[2]
    assert C.rotations == 0
    if order == "inc":
        assert C.n == K and C.longest_cascade == K
        assert [a for a, _, _ in C.firings] == list(range(K)) and C.partners == list(range(1, K + 1))
        assert int(np.count_nonzero(e["g"] != c.g)) == K
        assert len(C.per_chunk) == (K + rc.CHUNK - 1) // rc.CHUNK
    elif order == "dec":
        assert C.firings == [(K, 3, 0)] and C.partners == [K - 1]
    else:
        assert c.calls == K and [x.n for x in e["per_call"]] == [1] * K  # exactly one swap per step
        assert [a for a, _, _ in C.firings] == list(range(K, 0, -1))
        assert np.array_equal(e["g"], rc.expected(rc.case(f"cascade-{K}-inc"))["g"][::-1])  # the same hand-down


@pytest.mark.parametrize("name", rc.CONVOY_NAMES)
def test_convoy(name):
    c, e, C = _exp(name)
    K = int(name.split("-")[1])
    assert C.firings == [(0, 3, 0)] and C.partners == [1] and C.closes == 0
    assert C.walk_hops == [K]  # s's new successor chain: the K convoy agents, then a free cell
    assert (K < rc.WALK_CAP) == (name == "convoy-15")


@pytest.mark.parametrize("name", rc.PAIR_NAMES)
def test_pairs(name):
    c, e, C = _exp(name)
    P, order = int(name.split("-")[1]), name.split("-")[2]
    assert C.n == P and C.rotations2 == P and C.swaps == 0
    assert [a for a, _, _ in C.firings] == ([2 * p for p in range(P)] if order == "adj" else list(range(P)))
    if order == "split" and P >= rc.CHUNK:  # b and s of every firing in different chunks
        assert all(a // rc.CHUNK != s // rc.CHUNK for (a, _, _), s in zip(C.firings, C.partners))
    assert np.array_equal(e["v"], e["g"]) and np.all(e["g"] != c.g)  # both goals swapped, everybody moved onto its goal
    assert 2 * P <= rc.LIST_CAP or P == 513  # 512 pairs fill the changed list exactly, 513 overflow it


def test_mixed():
    c, e, C = _exp("mixed")
    assert c.n <= rc.CHUNK
    assert C.rotations2 == rc.MIXED_PAIRS and C.rotations == rc.MIXED_PAIRS + 1 and C.swaps == rc.MIXED_K
    assert sorted(len(k) for k in C.rot_per_cycle) == [2] * rc.MIXED_PAIRS + [4]
    assert C.longest_cascade == rc.MIXED_K
    assert C.r4_after_r3_in_chunk == {0}
    kinds = [k for _, k, _ in C.firings]
    assert kinds[:4] == [4, 3, 4, 3]  # the cascade's agents fire between the pairs'


@pytest.mark.parametrize("name", rc.CLOSE_NAMES)
def test_close(name):
    c, e, C = _exp(name)
    assert c.n <= 128 and C.closes > 0
    if name == "close-ring":
        # swaps (0, 3) and (1, 2); the first leaves a chain that ends at the resting agent 2, the second closes the
        # ring through 2 with a walk of nine agents (< walk_cap) past 0 and 3; then the 10-cycle rotates
        assert C.firings[:2] == [(0, 3, 0), (1, 3, 0)] and C.partners[:2] == [3, 2]
        assert C.walk_hops[:2] == [4, 10] and C.closes == 1 and C.walk_hops[1] - 1 < rc.WALK_CAP
        assert C.firings[2] == (2, 4, 10) and C.rotations >= 1


def test_close_search_finds_the_recorded_seeds():
    assert len(rc.CLOSE_SEEDS) == 3
    assert tuple(rc.search_closing(range(rc.CLOSE_SEEDS[-1] + 1))) == rc.CLOSE_SEEDS


@pytest.mark.parametrize("name", rc.FIELD_NAMES)
def test_field(name):
    c, e, C = _exp(name)
    nh = rc.NextHop(rc._oracle(c.rows))
    W = len(c.rows[0])

    def candidates(cell, goal):  # free neighbours one step closer (open field: Manhattan distance)
        d = lambda a: abs(a % W - goal % W) + abs(a // W - goal // W)
        return [q for q in (cell - W, cell + W, cell - 1, cell + 1) if 0 <= q < W * len(c.rows) and d(q) < d(cell)]

    # the goal a firing hands over has two candidate next hops from the taker's cell: no K2 code resolves it
    if name == "field-pairs":
        assert C.n == 8 and C.rotations2 == 8
        handed = [(int(c.v[a]), int(e["g"][a])) for a in range(c.n)]
    else:
        K = int(name.split("-")[2])
        assert C.swaps == K and C.longest_cascade == K and C.n == K
        assert (K <= rc.CHUNK) == (name == "field-cascade-20")  # an incremental relabel's list, and a full one's
        handed = [(int(c.v[a]), int(c.g[0])) for a in range(1, K)]  # the far goal, at every cell of the line
    for cell, goal in handed:
        assert len(candidates(cell, goal)) == 2, (name, cell, goal)
        assert nh(cell, goal) is not None


def test_embedded_cases_are_the_same_states():
    rows = rc.pg_rows()
    assert len(rows) == rc.PG_SIDE and all(len(r) == rc.PG_SIDE for r in rows)
    assert sum(r.count(".") for r in rows) == sum(sum(r.count(".") for r in rc.case(m).rows) for m in rc.PG_MEMBER.values())
    for name in rc.PG_CASES:
        c, b = rc.case(name), rc.embedded(name)
        eb, ec = rc.expected(b), rc.expected(c)
        assert eb["restated_ok"] and eb["counters"].firings == ec["counters"].firings
        w = len(c.rows[0])
        x0, y0 = rc.PG_ORIGIN[rc.pg_region(name)]
        assert np.array_equal(eb["g"], (ec["g"] // w + y0) * rc.PG_SIDE + ec["g"] % w + x0)
        assert np.array_equal(eb["v"], (ec["v"] // w + y0) * rc.PG_SIDE + ec["v"] % w + x0)


def test_place_rows_cover_every_case():
    """tests/host/place_main.cpp pins the ag and global placements at (n, W, H) rows: every case's fleet and grid is one
    of them, and every case of the pg selection has its fleet size among the 208x208 rows."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "place_main.cpp")).read()
    block = src[src.index("const Small small[] = {"):]
    block = block[:block.index("};")]
    rows = {tuple(int(x) for x in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", block)}
    want = {(rc.case(nm).n, len(rc.case(nm).rows[0]), len(rc.case(nm).rows)) for nm in rc.NAMES}
    assert want == rows, (sorted(want - rows), sorted(rows - want))
    pg = src[src.index("for (uint32_t n : {"):]
    sizes = {int(x) for x in re.findall(r"(\d+)u", pg[:pg.index("})")])}
    assert {rc.case(nm).n for nm in rc.PG_CASES} <= sizes
