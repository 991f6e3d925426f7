"""GPU: the fleet-wide decentralized tick. tsw_nearby against the brute-force definition of the lists,
tsw_decide_fleet bit-exact against the CPU oracle's compute_next_move_with_tswap (agent.rs:329-462) run
per agent on its brute-force list, and the documented error codes. The shapes of fleet_cases.py put both
on their internal boundaries: diamonds taller than the 64 rows a wave takes per trip, 2,048-element scan
tiles (one, one and a bit, 256, 257), lists of exactly 1,024 entries and one more."""
import ctypes
import functools

import numpy as np
import pytest

from p2p_distributed_tswap_amd import (Planner, TswapError, maps, TSW_EINVAL, TSW_EOVERFLOW, TSW_OK)
from oracle import OracleGraph

import fleet_cases as fc

pytestmark = pytest.mark.gpu

_U32P = ctypes.POINTER(ctypes.c_uint32)


def _p(a):
    return a.ctypes.data_as(_U32P)


@pytest.fixture(scope="module")
def planners():
    """One context per map for the whole module (tables stay warm between tests, as between ticks)."""
    made = {}

    def get(rows):
        key = tuple(rows)
        if key not in made:
            made[key] = Planner(rows)
        return made[key]

    yield get
    for p in made.values():
        p.close()


@functools.lru_cache(maxsize=None)
def _oracle(name, r):
    rows, v, g = fc.fleet_case(name)
    off, idx = fc.brute_nearby(v, len(rows[0]), r)
    return fc.oracle_fleet(OracleGraph(maps.rows_to_array(rows)), v, g, off, idx)


def _raw_nearby(p, v, r, cap):
    n = v.size
    off = np.full(n + 1, 0xDEADBEEF, dtype=np.uint32)
    idx = np.full(max(cap, 1), 0xDEADBEEF, dtype=np.uint32)
    total = ctypes.c_uint32(0xDEADBEEF)
    rc = p._lib.tsw_nearby(p._ctx, _p(v), n, r, _p(off), _p(idx), cap, ctypes.byref(total))
    return rc, off, idx, total.value


def _raw_fleet(p, v, g, r, cap):
    n = v.size
    act, cell, partner = (np.full(n, 0xDEADBEEF, dtype=np.uint32) for _ in range(3))
    off = np.full(n + 1, 0xDEADBEEF, dtype=np.uint32)
    part = np.full(max(cap, 1), 0xDEADBEEF, dtype=np.uint32)
    rc = p._lib.tsw_decide_fleet(p._ctx, _p(v), _p(g), n, r, _p(act), _p(cell), _p(partner), _p(off), _p(part), cap)
    return rc, act, cell, partner, off, part


def _assert_fleet_equal(got, ref):
    for name, a, b in zip(("act", "cell", "partner", "part_off", "part"), got, ref):
        assert a.dtype == np.uint32 and np.array_equal(a, b), f"{name}: first difference at {_first_diff(a, b)}"


def _first_diff(a, b):
    if a.shape != b.shape:
        return f"shapes {a.shape} vs {b.shape}"
    k = int(np.flatnonzero(a != b)[0])
    return f"[{k}]: gpu {int(a[k])} reference {int(b[k])}"


# ---- nearby vs brute force ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,r", fc.NEARBY_CASES)
def test_nearby_matches_brute_force(planners, name, r):
    W, H, rows, v = fc.nearby_shape(name)
    off, idx = planners(rows).nearby(v, r)
    boff, bidx = fc.brute_case(name, r)
    assert off.dtype == np.uint32 and idx.dtype == np.uint32
    assert np.array_equal(off, boff), _first_diff(off, boff)
    assert np.array_equal(idx, bidx), _first_diff(idx, bidx)


def test_nearby_cap_one_short_is_overflow_with_offsets(planners):
    W, H, rows, v = fc.nearby_shape("rand20")
    boff, bidx = fc.brute_case("rand20", 3)
    p = planners(rows)
    rc, off, idx, total = _raw_nearby(p, v, 3, int(boff[-1]) - 1)
    assert rc == TSW_EOVERFLOW
    assert total == boff[-1] and np.array_equal(off, boff)
    assert np.all(idx == 0xDEADBEEF)  # nb_idx is written only when it fits
    rc, off, idx, total = _raw_nearby(p, v, 3, int(boff[-1]))
    assert rc == TSW_OK and total == boff[-1] and np.array_equal(off, boff) and np.array_equal(idx, bidx)


def test_nearby_rejects_off_grid_cell(planners):
    W, H, rows, v = fc.nearby_shape("open6")
    p = planners(rows)
    bad = v.copy()
    bad[3] = W * H
    rc, _, _, _ = _raw_nearby(p, bad, 2, 1 << 16)
    assert rc == TSW_EINVAL
    with pytest.raises(TswapError):
        p.nearby(bad, 2)
    off, idx = p.nearby(v, 2)  # the context stays usable
    assert np.array_equal(off, fc.brute_case("open6", 2)[0]) and np.array_equal(idx, fc.brute_case("open6", 2)[1])


def test_nearby_half_million_agents_matches_grouping(planners):
    """2,048 * 256 + 2 agents: the offsets' scan has 257 tiles, so k_scan_sums takes a second trip with its
    carry. r = 0 on a fleet with up to three agents per cell, against the grouping reference (proven against
    brute force on the CPU); nb_off and nb_idx compared whole."""
    W, H, rows, v = fc.crowd_fleet()
    boff, bidx = fc.grouped_nearby(v)
    rc, off, idx, total = _raw_nearby(planners(rows), v, 0, bidx.size)
    assert rc == TSW_OK and total == bidx.size
    assert np.array_equal(off, boff), _first_diff(off, boff)
    assert np.array_equal(idx, bidx), _first_diff(idx, bidx)


# ---- fleet decide vs the oracle -----------------------------------------------------------------------

# tall9x200 at r = 40: diamonds of 81 rows, so the fill that writes nb_v / nb_g walks two chunks of rows
@pytest.mark.parametrize("name,r", [("rand20", 15), ("rand20", 3), ("dense12", 2), ("warehouse", 15), ("tall9x200", 40)])
def test_decide_fleet_matches_oracle(planners, name, r):
    rows, v, g = fc.fleet_case(name)
    ref = _oracle(name, r)
    got = planners(rows).decide_fleet(v, g, r)
    _assert_fleet_equal(got, ref)
    if name in ("rand20", "warehouse", "tall9x200"):
        assert set(np.unique(ref[0]).tolist()) == {0, 1, 2, 3}
    assert ref[3][-1] > 0  # rotations, so the participant translation is exercised


def test_decide_fleet_equals_decide_on_nearby_lists(planners):
    rows, v, g = fc.fleet_case("rand20")
    p = planners(rows)
    off, idx = p.nearby(v, 15)
    lists = [idx[off[i]:off[i + 1]] for i in range(v.size)]
    dec = p.decide(v, g, [[(int(v[j]), int(g[j])) for j in li] for li in lists])
    act, cell, partner, part_off, part = p.decide_fleet(v, g, 15)
    for i, (a, c, pt, ps) in enumerate(dec):
        li = lists[i]
        assert (a, c) == (act[i], cell[i]), i
        assert partner[i] == (0xFFFFFFFF if pt == 0xFFFFFFFF else li[pt]), i
        assert [int(li[k]) for k in ps] == part[part_off[i]:part_off[i + 1]].tolist(), i


# ---- lists of exactly 1,024 entries, and of 1,025 ------------------------------------------------------

NONE = 0xFFFFFFFF


def _raw_decide(p, v, g, off, idx):
    """tsw_decide on the lists (off, idx) of agent indices. Returns (rc, act, cell, partner, npart, part) in
    tsw_decide's own form: list indices, agent i's participants at part[off[i] + i ..]."""
    n = v.size
    nv, ng = np.ascontiguousarray(v[idx]), np.ascontiguousarray(g[idx])
    act, cell, partner, npart = (np.full(n, 0xDEADBEEF, dtype=np.uint32) for _ in range(4))
    part = np.zeros(idx.size + n + 1, dtype=np.uint32)
    rc = p._lib.tsw_decide(p._ctx, _p(v), _p(g), n, _p(off), _p(nv), _p(ng), _p(act), _p(cell), _p(partner), _p(npart),
                           _p(part))
    return rc, act, cell, partner, npart, part


def test_cap1025_decides_at_the_full_list_length(planners):
    """1,025 agents that all see each other: every list has 1,024 entries, the LDS sort's last slot and
    Rule 4's whole `chased` mask in use (rotations through agents >= 1,000). TSW_OK, equal to the oracle."""
    rows, v, g = fc.cap_fleet(1025)
    rc, act, cell, partner, off, part = _raw_fleet(planners(rows), v, g, 80, 8192)
    assert rc == TSW_OK
    _assert_fleet_equal((act, cell, partner, off, part[:off[-1]]), fc.cap_oracle(1025))


def test_cap1025_decide_fleet_equals_decide_on_nearby_lists(planners):
    rows, v, g = fc.cap_fleet(1025)
    p = planners(rows)
    off, idx = p.nearby(v, 80)
    assert np.all(np.diff(off.astype(np.int64)) == 1024)
    rc, act, cell, par, npart, lpart = _raw_decide(p, v, g, off, idx)
    assert rc == TSW_OK
    fact, fcell, fpartner, fpart_off, fpart = p.decide_fleet(v, g, 80)
    base = off[:-1].astype(np.int64)
    partner = np.where(par == NONE, NONE, idx[base + np.where(par == NONE, 0, par)]).astype(np.uint32)
    for name, a, b in (("act", act, fact), ("cell", cell, fcell), ("partner", partner, fpartner),
                       ("npart", npart, np.diff(fpart_off))):
        assert np.array_equal(a, b), f"{name}: first difference at {_first_diff(a, b)}"
    assert npart.sum() > 0
    for i in np.flatnonzero(npart):
        lp = lpart[off[i] + i:off[i] + i + npart[i]]
        assert np.array_equal(idx[base[i] + lp], fpart[fpart_off[i]:fpart_off[i + 1]]), int(i)


def test_cap1026_is_overflow_and_cap1025_decides_afterwards(planners):
    """One more agent: lists of 1,025 entries, one past the limit of Rule 4 -> TSW_EOVERFLOW; the same
    context then decides the 1,025-agent fleet."""
    rows, v, g = fc.cap_fleet(1026)
    p = planners(rows)
    rc = _raw_fleet(p, v, g, 80, 8192)[0]
    assert rc == TSW_EOVERFLOW
    assert "1024" in p._lib.tsw_last_error(p._ctx).decode()
    _, v5, g5 = fc.cap_fleet(1025)
    _assert_fleet_equal(p.decide_fleet(v5, g5, 80), fc.cap_oracle(1025))


def test_long_lists_decided_by_rules_1_to_3_match_oracle(planners):
    """1,100 agents with lists of 1,099 entries, none of which goes past Rule 3: tsw_decide_fleet decides
    on the nb_v / nb_g the brute-force fill wrote, and translates the swap partners through its nb_idx."""
    rows, v, g, ref = fc.long_rules123()
    rc, act, cell, partner, off, part = _raw_fleet(planners(rows), v, g, 80, 64)
    assert rc == TSW_OK
    _assert_fleet_equal((act, cell, partner, off, part[:off[-1]]), ref)


# ---- overflow and errors ------------------------------------------------------------------------------

def test_part_cap_zero_is_overflow_with_everything_but_part(planners):
    rows, v, g = fc.fleet_case("rand20")
    ref = _oracle("rand20", 15)
    p = planners(rows)
    rc, act, cell, partner, off, part = _raw_fleet(p, v, g, 15, 0)
    assert rc == TSW_EOVERFLOW
    _assert_fleet_equal((act, cell, partner, off), ref[:4])
    assert np.all(part == 0xDEADBEEF)
    rc, act, cell, partner, off, part = _raw_fleet(p, v, g, 15, int(off[-1]))
    assert rc == TSW_OK
    _assert_fleet_equal((act, cell, partner, off, part[:off[-1]]), ref)


def test_blocked_cell_is_einval_and_context_stays_usable():
    rows, v, g = fc.fleet_case("dense12")
    blocked = int(np.flatnonzero(maps.rows_to_array(rows).reshape(-1) == ord("@"))[0])
    bad = v.copy()
    bad[5] = blocked
    with Planner(rows) as p:
        rc = _raw_fleet(p, bad, g, 2, 1024)[0]
        assert rc == TSW_EINVAL
        badg = g.copy()
        badg[7] = len(rows) * len(rows[0])
        assert _raw_fleet(p, v, badg, 2, 1024)[0] == TSW_EINVAL
        _assert_fleet_equal(p.decide_fleet(v, g, 2), _oracle("dense12", 2))


def test_list_past_the_limit_reaching_rule4_is_overflow(planners):
    """1,100 agents at r = 80: every list has 1,099 entries. Agent 0's next hop is occupied by an agent
    that is not at its goal, so its decision reaches Rule 4 with a list past the documented 1,024-entry
    limit: TSW_EOVERFLOW, an error code and nothing else."""
    W, H, rows, v = fc.nearby_shape("open40")
    v = v.copy()
    occupied = set(v.tolist())
    a = next(i for i, c in enumerate(v.tolist()) if c % W != W - 1 and c + 1 in occupied)
    v[[0, a]] = v[[a, 0]]  # agent 0 now stands left of an occupied cell
    b = int(np.flatnonzero(v == v[0] + 1)[0])
    g = np.full_like(v, v[-1])  # three goal cells in all: three tables to build
    g[0] = v[b]
    g[b] = v[0]
    p = planners(rows)
    rc = _raw_fleet(p, v, g, 80, 8192)[0]
    assert rc == TSW_EOVERFLOW
    assert "1024" in p._lib.tsw_last_error(p._ctx).decode()
    # below the limit the same fleet decides: agent 0 and its blocker head for each other's cell, and
    # nobody stands at agent 0's cell to close the cycle (Rule 5)
    act, cell, partner, part_off, part = p.decide_fleet(v, g, 5)
    assert act[0] == 3 and cell[0] == v[0] and part_off[-1] == part.size


def test_empty_fleet(planners):
    p = planners(maps.open_map(6, 6))
    e = np.zeros(0, dtype=np.uint32)
    off, idx = p.nearby(e, 15)
    assert off.tolist() == [0] and idx.size == 0
    act, cell, partner, part_off, part = p.decide_fleet(e, e, 15)
    assert act.size == cell.size == partner.size == part.size == 0 and part_off.tolist() == [0]


# ---- determinism --------------------------------------------------------------------------------------

def test_two_calls_return_identical_arrays(planners):
    rows, v, g = fc.fleet_case("warehouse")
    p = planners(rows)
    n1, n2 = p.nearby(v, 15), p.nearby(v, 15)
    assert all(np.array_equal(a, b) for a, b in zip(n1, n2))
    d1, d2 = p.decide_fleet(v, g, 15), p.decide_fleet(v, g, 15)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))
