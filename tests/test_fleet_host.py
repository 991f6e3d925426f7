"""CPU: the fleet-wide decentralized tick (tsw_nearby / tsw_decide_fleet, ABI 8) is declared in every
mirror of the C ABI, and the binned list construction of tsw_nearby.hip — restated in numpy — equals the
brute-force definition on every shape the GPU test runs (clipping and index mistakes show here first).
Also the conditions under which the boundary cases of fleet_cases.py / fleet_run_model.py reach what they
are there for: a second trip over the diamond's rows, the scan's tile and block-sum edges, lists of exactly
1,024 entries, kept goal ops in more than one chunk of 256."""
import ctypes
import os
import re

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg

import fleet_cases as fc
import fleet_run_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsw_nearby", "tsw_decide_fleet")


def test_fleet_entry_points_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tswap.h")).read()
    rs = open(os.path.join(ROOT, "rust", "tswap-amd-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in pkg.EXPORTED_SYMBOLS
        assert re.search(rf"\bint {name}\(tsw_ctx \*ctx", hdr), name
        assert re.search(rf"pub fn {name}\(ctx: \*mut TswCtx", rs), name
    assert re.search(r"pub fn nearby\(&mut self", rs) and re.search(r"pub fn decide_fleet\(&mut self", rs)
    assert hasattr(pkg.Planner, "nearby") and hasattr(pkg.Planner, "decide_fleet")
    # the header says which list order the library chose
    assert "ASCENDING AGENT INDEX" in hdr and "HashMap" in hdr


def test_abi_is_8_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tswap.h")).read()
    rs = open(os.path.join(ROOT, "rust", "tswap-amd-sys", "src", "lib.rs")).read()
    assert re.search(r"#define TSW_ABI_VERSION 8\b", hdr)
    assert re.search(r"pub const TSW_ABI_VERSION: c_int = 8;", rs)
    assert pkg.TSW_ABI_VERSION == 8


def test_library_exports_fleet_entry_points():
    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("libtswap_hip.so not built (run __graft_entry__.build())")
    for path in (pkg.LIB_PATH, pkg.DIAG_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), (path, name)
        lib.tsw_abi_version.restype = ctypes.c_int
        assert lib.tsw_abi_version() == 8


@pytest.mark.parametrize("name,r", fc.NEARBY_CASES)
def test_binned_construction_equals_brute_force(name, r):
    W, H, _, v = fc.nearby_shape(name)
    off, idx = fc.binned_nearby(v, W, H, r)
    boff, bidx = fc.brute_case(name, r)
    assert np.array_equal(off, boff)
    assert np.array_equal(idx, bidx)


def test_brute_force_shapes_cover_the_paths():
    """The shapes reach what they are there for: lists past the 1,024-entry LDS sort, co-located agents,
    empty lists, clipping on every side."""
    off, _ = fc.brute_case("open40", 80)
    assert np.all(np.diff(off.astype(np.int64)) == 1099)
    off, _ = fc.brute_case("open6", 0)
    assert 0 < off[-1] < 18 * 17  # r = 0: only the duplicates see anyone
    off, _ = fc.brute_case("edges13x7", 40)
    n = fc.nearby_shape("edges13x7")[3].size
    assert off[-1] == n * (n - 1)  # r > W + H: everyone
    assert fc.brute_case("one", 15)[0].tolist() == [0, 0] and fc.brute_case("none", 15)[0].tolist() == [0]
    # diamonds taller than a wave: list members in a row that only the second trip over the rows reaches
    n9, n3 = fc.nearby_shape("tall9x200")[3].size, fc.nearby_shape("tall3x683")[3].size
    assert fc.second_chunk_agents("tall9x200", 31) == 0  # 63 rows: one partial chunk
    assert fc.second_chunk_agents("tall9x200", 32) >= 1  # 65 rows: the second chunk is the row y + 32 alone
    for r in (100, 300):
        assert 2 * fc.second_chunk_agents("tall9x200", r) >= n9
    assert fc.second_chunk_agents("tall3x683", 15) == 0
    for r in (64, 700):
        assert 2 * fc.second_chunk_agents("tall3x683", r) >= n3
    for name, r in fc.NEARBY_CASES:
        if name.startswith("tall"):  # all of them on the LDS-sorted fill
            assert np.diff(fc.brute_case(name, r)[0].astype(np.int64)).max() < 1024, (name, r)


def test_scan_tile_shapes_sit_on_their_boundaries():
    """Cells and agents per scan tile (2,048) and tiles per trip of the block-sum scan (256): each shape is
    exactly at, or one past, the boundary it is there for, with agents where a wrong tile base shows."""
    tiles = lambda m: -(-m // fc.SCAN_TILE)
    for name, ncell in (("tile64x32", 2048), ("tall3x683", 2049)):
        W, H, _, v = fc.nearby_shape(name)
        assert W * H == ncell and tiles(ncell) == (1 if ncell == 2048 else 2)
        assert {ncell - 1, ncell - 2} <= set(v.tolist())  # agents on the grid's last cells
        assert np.sum(v == ncell - 1) >= 2  # the last cell's own count is not 1
    for name, ntile in (("grid1024x512", 256), ("grid1024x513", 257)):
        W, H, _, v = fc.nearby_shape(name)
        assert tiles(W * H) == ntile and (ntile - 1) // fc.TILES_PER_CHUNK == (ntile == 257)
        lens = np.diff(fc.brute_case(name, 15)[0].astype(np.int64))
        tail = v >= fc.SCAN_TILE * fc.TILES_PER_CHUNK if ntile == 257 else v >= (H - 3) * W
        assert tail.sum() >= 40 and lens[tail].min() >= 1  # past cell 524,288 (1024 x 512: the last three rows)
        assert np.sum(v == W * H - 1) >= 2 and 0 in v.tolist()
        assert np.unique(v).size < v.size  # co-located agents
        # agents above the tail rows whose diamond reaches a row's last cell: their count reads
        # cell_start at the first cell of the tail (on 1024 x 513 the first cell of tile 257)
        x, y = v.astype(np.int64) % W, v.astype(np.int64) // W
        R = (H - 1 if ntile == 257 else H - 3) - 1  # the row above the tail
        assert np.any((y <= R) & (R - y <= 15) & (x + 15 - (R - y) >= W - 1))
        assert np.sum(~tail) >= 200 and np.unique(y[~tail] // 64).size >= 6  # the rest spread over the grid
    for name, n in (("agents2048", 2048), ("agents2049", 2049)):
        v = fc.nearby_shape(name)[3]
        off, _ = fc.brute_case(name, 1)
        assert v.size == n and np.unique(v).size < n
        assert np.unique(np.diff(off.astype(np.int64))).size >= 5  # the offsets are no ramp
        assert off[-1] > off[-2]  # the last agent, alone in its tile when n = 2,049, has a list


def test_grouping_reference_equals_brute_force():
    """grouped_nearby (the r = 0 lists from a stable argsort) against the definition, on open6 and on the
    3,000 agents of the half-million fleet that stand on its smallest cells (co-location kept)."""
    v6 = fc.nearby_shape("open6")[3]
    off, idx = fc.grouped_nearby(v6)
    boff, bidx = fc.brute_case("open6", 0)
    assert np.array_equal(off, boff) and np.array_equal(idx, bidx)
    W, H, _, v = fc.crowd_fleet()
    sel = np.sort(np.argsort(v, kind="stable")[:3000])
    off, idx = fc.grouped_nearby(v[sel])
    boff, bidx = fc.brute_nearby(v[sel], W, 0)
    assert off.dtype == idx.dtype == np.uint32
    assert np.array_equal(off, boff) and np.array_equal(idx, bidx)
    assert set(np.diff(off.astype(np.int64)).tolist()) == {0, 1, 2}
    e = np.zeros(0, dtype=np.uint32)
    assert fc.grouped_nearby(e)[0].tolist() == [0] and fc.grouped_nearby(e)[1].size == 0


def test_half_million_fleet_is_257_tiles_of_agents_and_no_ramp():
    W, H, _, v = fc.crowd_fleet()
    n = v.size
    assert n == fc.SCAN_TILE * fc.TILES_PER_CHUNK + 2 and -(-n // fc.SCAN_TILE) == 257
    assert v.dtype == np.uint32 and v.max() < W * H
    off, idx = fc.grouped_nearby(v)
    lens = np.bincount(np.diff(off.astype(np.int64)))
    assert lens.size == 3 and 2 * (lens[1] + lens[2]) > n and lens[0] > n // 20 and lens[2] > n // 10
    assert off[-1] == idx.size == lens[1] + 2 * lens[2]
    assert lens[0] > 0 and np.diff(off.astype(np.int64))[-2:].sum() > 0  # the last tile's two agents: a list


def _cap_oracle(n):
    _, v, g = fc.cap_fleet(n)
    return v, g, fc.brute_case(f"cap{n}", 80)[0], fc.cap_oracle(n)


def test_cap_fleets_fill_the_1024_entry_limit():
    """cap1025: every list has exactly 1,024 entries (the last slot of the LDS sort buffer, the whole of
    k_decide's `chased` mask), cap1026 one more (the first size on the brute-force fill, past Rule 4's
    limit); rotations whose participants have agent indices >= 1,000 — list indices in the mask's top word."""
    v, g, off, (act, cell, partner, part_off, part) = _cap_oracle(1025)
    assert v.size == 1025 and np.all(np.diff(off.astype(np.int64)) == 1024)
    rots = [(int(i), part[part_off[i]:part_off[i + 1]]) for i in np.flatnonzero(act == 2)]
    assert len(rots) >= 5
    assert sum(1 for _, p in rots if (p >= 1000).any()) >= 1
    # stricter: a CHASED participant (every one but the first) whose list index is in the mask's word 15
    assert sum(1 for i, p in rots if ((p[1:] - (p[1:] > i)) >= 960).any()) >= 1
    assert np.sum((v != g) & (act >= 2)) >= 300  # Wait or Rotation away from the goal: they reached Rule 4
    v6, g6, off6, ref6 = _cap_oracle(1026)
    assert v6.size == 1026 and np.all(np.diff(off6.astype(np.int64)) == 1025)
    assert np.array_equal(v6[1:], v) and np.array_equal(g6[1:], g)  # one more agent in front
    assert np.sum((v6 != g6) & (ref6[0] >= 2)) >= 1  # someone reaches Rule 4 with a list of 1,025


def test_long_rules123_never_reaches_rule4():
    rows, v, g, (act, cell, partner, part_off, part) = fc.long_rules123()
    off, _ = fc.brute_case("open40", 80)
    assert np.all(np.diff(off.astype(np.int64)) == 1099)
    assert set(np.unique(act).tolist()) == {0, 1} and part_off[-1] == 0  # Move or GoalSwap, nothing else
    assert np.sum((act == 0) & (cell != v)) >= 30
    assert np.sum(act == 1) >= 30 and np.all(partner[act == 1] < v.size)


# ---- the hand-made apply cases whose kept ops cross the compaction's chunks of 256 ---------------------

def test_kept_cases_keep_more_than_one_chunk_of_ops():
    """k_fleet_goals compacts the ops that did not fire in chunks of 256 and carries `kept` between them.
    Each case has a round that keeps ops in its first chunk AND in a later one, changes the state, and
    ends within as many rounds as it has ops (the library's no-progress guard)."""
    want = {"chain300": (300, 300, 299), "pairs800": (800, 2, 400), "rotations_kept300": (304, 300, 299)}
    for name in fm.KEPT_CASES:
        _, v, g, act, cell, partner, part_off, part = fm.apply_case(name)
        pend = fm.goal_op_pending(act, partner, part_off, part)
        nops, rounds, kept1 = want[name]
        assert len(pend[0]) == nops and len(pend) == rounds == fm.goal_op_rounds(act, partner, part_off, part)
        assert len(pend[1]) == kept1 > 256  # round 1 keeps more than a chunk
        assert fm.kept_carry_rounds(act, partner, part_off, part) >= 1
        assert np.unique(g).size == g.size  # distinct goals: a lost or twice-fired op changes g
        v1, g1 = fm.apply_model(v, g, *fm.apply_case(name)[3:])
        assert np.array_equal(v1, v) and not np.array_equal(g1, g)
    _, _, _, act, _, partner, part_off, part = fm.apply_case("pairs800")
    pend = fm.goal_op_pending(act, partner, part_off, part)
    assert pend[1] == [3 * k + 1 for k in range(400)]  # the odd ops, interleaved with the fired ones
    _, _, _, act, _, partner, part_off, part = fm.apply_case("rotations_kept300")
    assert int((act == fm.ROTATION).sum()) == 300 and np.all(np.diff(part_off)[act == fm.ROTATION] == 2)
    assert {int(act[i]) for i in fm.goal_op_pending(act, partner, part_off, part)[1]} == {fm.ROTATION}  # kept: rotations
    # the earlier cases never did: at most one chunk pending, or nothing kept
    for name in ("chain200", "disjoint1500", "rotation70"):
        _, _, _, act, _, partner, part_off, part = fm.apply_case(name)
        assert fm.kept_carry_rounds(act, partner, part_off, part) == 0


def test_long_run_case_fails_or_finishes_as_the_model_says():
    v, g, v_rec, g_rec, done, overflow = fm.long_run_case()
    assert 1 <= done <= 3 and v_rec.shape == g_rec.shape == (1100, done + 1)  # tick 0 is Rules 1-3 by construction
    assert overflow or done == 3
    assert not np.array_equal(v_rec[:, 0], v_rec[:, 1]) and not np.array_equal(g_rec[:, 0], g_rec[:, 1])
