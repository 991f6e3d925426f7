"""GPU: where the table entry points write and read caller memory, at the sizes and addresses the rest of the
suite never gives them.

1. K1 into caller memory (tsw_dist_tables_device, tsw_next_hop_tables_device) on grids whose cell count is odd
   or 4 mod 8, single-row / single-column grids, a grid with full 32-cell row words and one with more row
   words than one step of k_bfs_blk's write-out ring — at a 16-byte-aligned base and at bases shifted by 2 and
   8 bytes, for the production kernel choice and every forced kernel of the diagnostic build. run_bfs then
   turns the 16-byte stores and the LDS-staged write-out off (vec16, stage), so the kernels' scalar
   write-outs run: put_direct of k_bfs_blk, the scalar branches of k_bfs_big and k_bfs_wave, the !vec_ok
   paths of k_bfs. Every table == the oracle's BFS, and the 256-byte guard bands around the buffer
   (table_io_cases.GuardedDevBuf) are untouched.
   Not covered: k_bfs<LDS_TABLE = false> needs a grid whose u16 table does not fit LDS beside the bitmaps
   (about 65k cells and up): too large for a test that has to run in seconds, so it is left out.
2. The imports (tsw_import_tables_device, tsw_import_next_hops_device) from a rank-major gathered buffer of
   world = 3 (sharding.gathered_blocks) whose later blocks start 2-byte aligned: into a lazy context, with part
   of the goals already resident and goals listed twice (the source-row index is then not the identity), with
   unresolved codes and a producer's pending markers, and into a store bounded by table_budget_bytes. After
   every import the whole store is audited against the oracle (table_io_cases.check_store) and a plan is exact.
"""
import functools

import numpy as np
import pytest

import table_io_cases as tc
from p2p_distributed_tswap_amd import (TSW_ENOMEM, TSW_F_LAZY_NEXTHOP, TSW_HOST_ASTAR_OFF, Planner, TswapError, maps,
                                       sharding)
from table_io_cases import GuardedDevBuf, check_store
from test_gpu_bfs import _env
from worker_cases import ASTAR, NH_UNKNOWN

pytestmark = pytest.mark.gpu

SHIFTS = (0, 2, 8)
KERNELS = {
    "default": None,  # the production library's own choice
    "blk": dict(TSW_BFS_KERNEL="blk"),
    "blk-pair": dict(TSW_BFS_KERNEL="blk", TSW_BFS_PAIR=1),
    "wave": dict(TSW_BFS_KERNEL="wave"),
    "block": dict(TSW_BFS_KERNEL="block"),
    "big": dict(TSW_BFS_KERNEL="big"),
    "mg": dict(TSW_BFS_KERNEL="mg"),
}
ODD = ("rand33x17", "rand100x31")  # the two grids of the import tests


def _planner(rows, env, **kw):
    return Planner(rows, diag=env is not None, **kw)


def _check_dist_device(name, env, shifts):
    ref, goals, want = tc.grid_ref(name), tc.grid_goals(name), tc.grid_tables(name)
    ncell = ref.W * ref.H
    with _env(**(env or {})), _planner(ref.rows, env) as p:
        for shift in shifts:
            buf = GuardedDevBuf(goals.size * ncell * 2, shift)
            p.dist_tables_device(goals, buf.addr)
            got = buf.read(np.uint16, (goals.size, ncell))
            what = f"{name} shift {shift}"
            # both looked at before either fails: a store past a row's end shows in the next row and in the guard
            diff, damage = tc.first_table_diff(got, want, goals), buf.guard_damage()
            assert not diff and not damage, f"{what}: tables: {diff or 'equal'}; guards: {damage or 'intact'}"


# ---- 1. K1 into caller memory --------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(tc.GRIDS))
def test_dist_tables_device_odd_strides_and_unaligned_bases(name, kernel):
    _check_dist_device(name, KERNELS[kernel], SHIFTS)


def test_dist_tables_device_blk_unstaged_16_byte_stores():
    """TSW_BFS_NOSTAGE with an aligned base and W % 32 == 0: put_direct's 16-byte branch."""
    _check_dist_device("rand64x20", dict(TSW_BFS_KERNEL="blk", TSW_BFS_NOSTAGE=1), (0,))


@functools.lru_cache(maxsize=None)
def _resolved(name, cshift, dshift):
    """(codes (13, ncell) u8, tables (13, ncell) u16) of grid_goals(name) from ONE
    tsw_next_hop_tables_device call of the production library into buffers shifted by (cshift, dshift) bytes;
    the guards are checked here. Shared (read-only)."""
    ref, goals = tc.grid_ref(name), tc.grid_goals(name)
    ncell = ref.W * ref.H
    cbuf, dbuf = GuardedDevBuf(goals.size * ncell, cshift), GuardedDevBuf(goals.size * ncell * 2, dshift)
    with Planner(ref.rows) as p:
        p.next_hop_tables_device(goals, cbuf.addr, dbuf.addr)
    codes, tabs = cbuf.read(np.uint8, (goals.size, ncell)), dbuf.read(np.uint16, (goals.size, ncell))
    cbuf.guards_intact(f"{name} codes shift {cshift}")
    dbuf.guards_intact(f"{name} tables shift {dshift}")
    codes.setflags(write=False)
    tabs.setflags(write=False)
    return codes, tabs


@pytest.mark.parametrize("cshift,dshift", [(0, 0), (1, 2)])
@pytest.mark.parametrize("name", ODD)
def test_next_hop_tables_device_codes_and_tables(name, cshift, dshift):
    ref, goals = tc.grid_ref(name), tc.grid_goals(name)
    codes, tabs = _resolved(name, cshift, dshift)
    diff = tc.first_table_diff(tabs, tc.grid_tables(name), goals)
    assert not diff, diff
    for k, g in enumerate(goals):
        want = ref.og.next_codes(int(g))
        bad = np.flatnonzero(codes[k] != want)
        assert bad.size == 0, f"goal {g}: {bad.size} codes differ, first cell {bad[0]} got {codes[k][bad[0]]} want {want[bad[0]]}"


# ---- 2. imports ------------------------------------------------------------------------------------------------

WORLD = 3
# instance seeds whose plans end by themselves and whose goal count gives an odd block length (below)
SEEDS = {"rand33x17": 3, "rand100x31": 2}


@functools.lru_cache(maxsize=None)
def _instance(name):
    """(ref, starts, tasks, goals of the plan, oracle records, oracle goals), computed once and shared."""
    ref = tc.grid_ref(name)
    starts, tasks = maps.make_instance(ref.rows, 20, 40, SEEDS[name])
    rec, goal = ref.og.mapd(starts, tasks, 2000, trace_goals=True)
    goals = tc.goalset(ref.rows, starts, tasks)
    for a in (starts, tasks, rec, goal, goals):
        a.setflags(write=False)
    return ref, starts, tasks, goals, rec, goal


@functools.lru_cache(maxsize=None)
def _host_tables(name):
    """goal -> og.bfs table of every goal of _instance(name) (read-only)."""
    ref, _, _, goals, _, _ = _instance(name)
    out = {int(g): ref.og.bfs(int(g)) for g in goals}
    for t in out.values():
        t.setflags(write=False)
    return out


def _gather(rows_of, order, itemsize, ncell, shift=0):
    """The all-gather's buffer for the goal list `order` over WORLD ranks: rank r's block holds the rows of
    order[r::WORLD] at row offset r * per (sharding.gathered_blocks), short blocks padded (left as filler)."""
    per = sharding.shard_rows(order.size, WORLD)
    buf = GuardedDevBuf(WORLD * per * ncell * itemsize, shift)
    for _, gl, off in sharding.gathered_blocks(order, WORLD):
        if gl.size:
            buf.from_host(np.stack([rows_of[int(g)] for g in gl]), off * ncell * itemsize)
    return buf


def _blocks(order, ncell, *bufs_itemsizes):
    """[(goals of the block, address of its first row in every buffer)]."""
    return [(gl, [b.addr + off * ncell * sz for b, sz in bufs_itemsizes])
            for _, gl, off in sharding.gathered_blocks(order, WORLD) if gl.size]


def _assert_plan(p, name, what):
    _, starts, tasks, _, rrec, rgoal = _instance(name)
    rec, goal = p.plan_mapd_arrays(starts, tasks, 2000, trace_goals=True)
    assert np.array_equal(goal, rgoal), f"{what}: goals differ from the oracle's"
    assert np.array_equal(rec, rrec), f"{what}: records differ from the oracle's"


@pytest.mark.parametrize("name", ODD)
def test_import_tables_into_lazy_context(name):
    ref, _, _, goals, _, _ = _instance(name)
    ncell = ref.W * ref.H
    # an odd block length: with an odd ncell rank 1's block starts 2-byte aligned, with ncell % 8 == 4 8-byte aligned
    per = sharding.shard_rows(goals.size, WORLD)
    assert per % 2 == 1 and per * ncell * 2 % 16 in (2, 6, 8, 10, 14)
    dbuf = _gather(_host_tables(name), goals, 2, ncell)
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        for gl, (addr,) in _blocks(goals, ncell, (dbuf, 2)):
            p.import_tables_device(gl, addr)
        _, ug, n = check_store(p, ref, goals, name)
        assert n == 0 and np.array_equal(ug, goals)  # lazy: K1 codes only, every multi-candidate cell 0xFF
        assert p.stats()["tables"] == goals.size
        _assert_plan(p, name, name)
        check_store(p, ref, goals, name + " after the plan")
        assert p.stats()["bfs_goals"] == 0  # every table came from the import
    dbuf.guards_intact(name)


def _dup_order(goals):
    """The import list of the partially-resident cases: a seeded permutation of the goals with two of them
    listed twice, one of the repeats in the same block as its first listing."""
    order = [int(g) for g in np.random.default_rng(0xD0B1E).permutation(goals)]
    order.insert(7, order[1])   # 7 = 1 (mod WORLD): both in rank 1's block
    order.append(order[0])
    return np.array(order, dtype=np.uint32)


def _src_not_identity(order, resident):
    """Blocks of the import in which a new goal's row index differs from its index among the new goals."""
    n, seen = 0, set(int(g) for g in resident)
    for _, gl, _ in sharding.gathered_blocks(order, WORLD):
        src = []
        for i, g in enumerate(gl):
            if int(g) not in seen:
                seen.add(int(g))
                src.append(i)
        n += src != list(range(len(src)))
    return n


@pytest.mark.parametrize("codes", [False, True], ids=["import_tables", "import_next_hops"])
@pytest.mark.parametrize("name", ODD)
def test_import_partially_resident_and_duplicated(name, codes):
    """Every third goal is resident before the import and two goals are listed twice, so the rows of the new
    goals are not rows 0, 1, 2, ... of their block: a wrong source row puts another goal's table (codes) into
    a slot, which the audit finds."""
    ref, _, _, goals, _, _ = _instance(name)
    ncell = ref.W * ref.H
    resident = goals[::3]
    order = _dup_order(goals)
    assert _src_not_identity(order, resident) >= 2
    dbuf = _gather(_host_tables(name), order, 2, ncell)
    cbuf = None
    if codes:
        # fully resolved codes of every goal, from the library itself (checked against the oracle by the audit below)
        with Planner(ref.rows) as q:
            full = q.next_hop_tables(goals)
        assert (full[:, ref.free] <= 4).all()
        cbuf = _gather({int(g): full[k] for k, g in enumerate(goals)}, order, 1, ncell)
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        p.next_hop_codes(resident, resident)  # start == goal: code 4 from a K1 table of its own
        assert p.stats()["tables"] == resident.size
        if codes:
            for gl, (da, ca) in _blocks(order, ncell, (dbuf, 2), (cbuf, 1)):
                p.import_next_hops_device(gl, da, ca)
        else:
            for gl, (da,) in _blocks(order, ncell, (dbuf, 2)):
                p.import_tables_device(gl, da)
        assert p.stats()["tables"] == goals.size
        assert p.stats()["bfs_goals"] == resident.size
        check_store(p, ref, goals, name)
        _assert_plan(p, name, name)
    dbuf.guards_intact(name)
    if cbuf:
        cbuf.guards_intact(name)


def _place_markers(ref, tabs, seed):
    """Overwrite a seeded subset of the still-unresolved free cells of every table with the pending markers
    0xFE / 0xFD: per table the first and the last such cell, one at an index = 0 and one = 7 (mod 8) where
    there is one, and a few seeded others. Returns the counts of (0xFE, 0xFD) placed."""
    rng = np.random.default_rng(seed)
    count = {tc.NH_PENDING: 0, tc.NH_PENDING_S: 0}
    edges = 0
    for k in range(tabs.shape[0]):
        open_ = np.flatnonzero(ref.free & (tabs[k] == NH_UNKNOWN))
        if open_.size == 0:
            continue
        pick = {int(open_[0]), int(open_[-1])}
        for r in (0, 7):
            m = open_[open_ % 8 == r]
            if m.size:
                pick.add(int(rng.choice(m)))
                edges += 1
        pick.update(int(c) for c in rng.choice(open_, min(5, open_.size), replace=False))
        for j, c in enumerate(sorted(pick)):
            mk = tc.NH_PENDING if (j + k) % 2 == 0 else tc.NH_PENDING_S
            tabs[k][c] = mk
            count[mk] += 1
    assert edges >= 2
    return count[tc.NH_PENDING], count[tc.NH_PENDING_S]


@pytest.mark.parametrize("name", ODD)
def test_import_next_hops_partial_codes_and_pending_markers(name):
    """Codes as a lazy producer holds them after a short plan (resolved and 0xFF mixed), some of the 0xFF cells
    overwritten with the producer's pending markers: the import turns the markers into 0xFF, keeps the rest,
    and the plan resolves what it needs by itself."""
    ref, starts, tasks, goals, _, _ = _instance(name)
    ncell = ref.W * ref.H
    per = sharding.shard_rows(goals.size, WORLD)
    dbuf = GuardedDevBuf(WORLD * per * ncell * 2)
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP) as q:
        q.plan_mapd_arrays(starts, tasks, 12)
        part = q.next_hop_tables(goals)
        for gl, (da,) in _blocks(goals, ncell, (dbuf, 2)):
            q.dist_tables_device(gl, da)
    multi = sum(int(np.count_nonzero(ref.k1(int(g)) == ASTAR)) for g in goals)
    unresolved = int(np.count_nonzero(part[:, ref.free] == NH_UNKNOWN))
    assert 0 < unresolved < multi  # a mix: the short plan resolved some multi-candidate cells, not all
    n_fe, n_fd = _place_markers(ref, part, 0xFEFD)
    assert n_fe > 0 and n_fd > 0
    cbuf = _gather({int(g): part[k] for k, g in enumerate(goals)}, goals, 1, ncell)
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP, host_astar=TSW_HOST_ASTAR_OFF) as p:
        for gl, (da, ca) in _blocks(goals, ncell, (dbuf, 2), (cbuf, 1)):
            p.import_next_hops_device(gl, da, ca)
        tabs, _, n = check_store(p, ref, goals, name)  # no marker survives; nothing else changed:
        keep = (part != tc.NH_PENDING) & (part != tc.NH_PENDING_S)
        assert np.array_equal(tabs[keep], part[keep]) and (tabs[~keep] == NH_UNKNOWN).all()
        assert n > 0
        p.reset_stats()
        _assert_plan(p, name, name)
        st = p.stats()
        assert st["bfs_goals"] == 0 and st["astar_queries"] > 0
        check_store(p, ref, goals, name + " after the plan")
    dbuf.guards_intact(name)
    cbuf.guards_intact(name)


def test_import_fully_resolved_next_hops_plans_without_k1_or_k3():
    """test_gpu_sharding.test_sharded_next_hops_then_plan on an odd grid, world = 3: the producers write codes and
    tables straight into the (2-byte-aligned) blocks of the gather."""
    name = "rand33x17"
    ref, _, _, goals, _, _ = _instance(name)
    ncell = ref.W * ref.H
    per = sharding.shard_rows(goals.size, WORLD)
    dbuf, cbuf = GuardedDevBuf(WORLD * per * ncell * 2), GuardedDevBuf(WORLD * per * ncell)
    blocks = _blocks(goals, ncell, (dbuf, 2), (cbuf, 1))
    for gl, (da, ca) in blocks:
        with Planner(ref.rows) as q:
            q.next_hop_tables_device(gl, ca, da)
            assert q.stats()["bfs_goals"] == gl.size
    with Planner(ref.rows) as p:
        for gl, (da, ca) in blocks:
            p.import_next_hops_device(gl, da, ca)
        p.reset_stats()
        _assert_plan(p, name, name)
        st = p.stats()
        assert st["bfs_goals"] == 0 and st["astar_queries"] == 0
        _, _, n = check_store(p, ref, goals, name)
        assert n > 0
    dbuf.guards_intact(name)
    cbuf.guards_intact(name)


@pytest.mark.parametrize("name", ODD)
def test_import_into_budgeted_store(name):
    ref, _, _, goals, _, _ = _instance(name)
    ncell = ref.W * ref.H
    B = 8
    first, second, nine = goals[:6], goals[6:12], goals[12:21]
    assert nine.size == 9
    host = _host_tables(name)
    bufs = [_gather(host, gl, 2, ncell) for gl in (first, second, nine)]
    with Planner(ref.rows, flags=TSW_F_LAZY_NEXTHOP, table_budget_bytes=B * ((ncell + 7) // 8 * 8) * 2) as p:
        for order, buf in zip((first, second), bufs):
            for gl, (da,) in _blocks(order, ncell, (buf, 2)):
                p.import_tables_device(gl, da)
        st = p.stats()
        assert st["table_evictions"] > 0 and st["tables"] <= B and st["bfs_goals"] == 0
        check_store(p, ref, second, name + " second six")
        before = p.stats()["tables"]
        # one call with more new goals than the budget holds: refused, nothing registered
        big = GuardedDevBuf(9 * ncell * 2)
        big.from_host(np.stack([host[int(g)] for g in nine]))
        with pytest.raises(TswapError) as ei:
            p.import_tables_device(nine, big.addr)
        assert ei.value.code == TSW_ENOMEM
        assert p.stats()["tables"] == before
        check_store(p, ref, second, name + " after ENOMEM")
        assert p.stats()["tables"] == before and p.stats()["bfs_goals"] == 0  # the audit built nothing: all resident
        # a step toward the first six (at least four of them were evicted) rebuilds them
        comp = np.array([y * ref.W + x for x, y in maps.largest_component(ref.rows)], dtype=np.uint32)
        v = np.random.default_rng(5).choice(comp, first.size, replace=False).astype(np.uint32)
        p.reset_stats()
        hv, hg = p.step(v, first)
        rv, rg = ref.og.step(v, first)
        assert np.array_equal(hv, rv) and np.array_equal(hg, rg)
        assert p.stats()["bfs_goals"] > 0 and p.stats()["tables"] <= B
        check_store(p, ref, first, name + " rebuilt")
    for b in bufs[:2] + [big]:
        b.guards_intact(name)
