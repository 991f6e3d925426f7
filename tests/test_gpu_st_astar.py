"""GPU: tsw_astar_reserved, the batched space-time A* with reservations. path_off, path, status and pops must
equal the CPU model's (tests/st_astar_model.py) and the host twin's on the whole shared case list; any split of the
queries over calls gives the same per-query results; the size query, TSW_EOVERFLOW and TSW_EINVAL contracts; and
the call leaves the context as it found it. Grids are 8x8 and 12x12 but for the two packed-field cases."""
import ctypes

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg
import st_astar_model as sm
from p2p_distributed_tswap_amd import TSW_EINVAL, TSW_EOVERFLOW, TSW_F_LAZY_NEXTHOP, TSW_OK, Planner, maps

pytestmark = pytest.mark.gpu

_U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xABABABAB
CASES = [c.name for c in sm.all_cases()]


@pytest.fixture(scope="module")
def planners():
    """One context per map for the whole module."""
    made = {}

    def get(rows):
        key = tuple(rows)
        if key not in made:
            made[key] = Planner(list(rows))
        return made[key]

    yield get
    for p in made.values():
        p.close()


def _device(p, c, sel=None):
    st, gl, t0, nr, er = c.arrays()
    if sel is not None:
        st, gl, t0 = st[sel], gl[sel], t0[sel]
    return p.astar_reserved(st, gl, t0, nr, er, c.max_time, c.max_nodes)


def _host(c):
    st, gl, t0, nr, er = c.arrays()
    return pkg.host_astar_reserved(c.rows, st, gl, t0, nr, er, c.max_time, c.max_nodes)


def _assert_same(got, ref, what):
    for name, g, e in zip(("status", "pops", "path_off", "path"), (got[2], got[3], got[0], got[1]),
                          (ref[2], ref[3], ref[0], ref[1])):
        if not np.array_equal(g, e):
            i = int(np.nonzero(g != e)[0][0]) if g.shape == e.shape else -1
            raise AssertionError(f"{what}: {name} differs (first at {i}: got {g[i] if i >= 0 else g.shape}, "
                                 f"expected {e[i] if i >= 0 else e.shape})")


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_model_and_the_host_twin(planners, name):
    c = sm.by_name(name)
    got = _device(planners(c.rows), c)
    _assert_same(got, c.expected(), f"{name} vs model")
    _assert_same(got, _host(c), f"{name} vs host twin")


def test_open_8x8_all_pairs_in_one_call(planners):
    """4,032 queries in one call, far above one workgroup; the heap's tie-break decides every path."""
    c = sm.open_case()
    got = _device(planners(c.rows), c)
    _assert_same(got, c.expected(), "open8x8 vs model")
    _assert_same(got, _host(c), "open8x8 vs host twin")


def test_more_queries_than_waves_in_flight(planners):
    """The open 8x8 pairs three times over, 12,096 queries: more than the 8,192 waves a 256-CU device seats, so
    waves run several queries one after the other on the same visited table (the tag tells them apart)."""
    c = sm.repeated(sm.open_case(), 3)
    p = planners(c.rows)
    got = _device(p, c)
    _assert_same(got, c.expected(), "open8x8 x3 vs model")
    assert p.st_astar_probe()["waves"] < len(c.queries)


# The paths a small case never takes, forced through the diagnostic library's test knobs: a heap of 8 entries in
# LDS (the move to the global heap in nearly every search), 3 waves (a wave runs many queries in turn), 600 segment
# words a batch (the call is cut into batches) and a first tag just below 2^18 - 1 (the tags wrap and the tables are
# wiped between two batches).
@pytest.mark.parametrize("name", ["random12-3", "big-heap-40", "x-to-2047"])
def test_forced_spill_batches_and_tag_wrap(monkeypatch, name):
    for k, v in (("TSW_ST_HEAP", 8), ("TSW_ST_WAVES", 3), ("TSW_ST_SEG_WORDS", 600), ("TSW_ST_TAG0", (1 << 18) - 6)):
        monkeypatch.setenv(k, str(v))
    c = sm.by_name(name)
    assert max(c.expected()[5]) > 8
    with Planner(c.rows, diag=True) as p:
        for _ in range(2):  # the second call goes on with the first one's tags
            got = _device(p, c)
            _assert_same(got, c.expected(), f"{name} with the knobs vs model")
            probe = p.st_astar_probe()
            assert probe["waves"] <= 3
            if name == "random12-3":
                assert probe["batches"] >= 4  # 50 queries of 46 or 49 segment words, 600 a batch


@pytest.mark.parametrize("k", [0, 1, 63, 65, 257])
def test_any_k_gives_the_same_per_query_results(planners, k):
    """k queries drawn over the random grid's 50 (with repeats past 50) equal the one big call's, query by query."""
    c = sm.by_name("random12-3")
    off, path, status, pops = c.expected()[:4]
    sel = (np.arange(k) * 7) % len(c.queries)
    g_off, g_path, g_status, g_pops = _device(planners(c.rows), c, sel)
    assert g_off.size == k + 1 and g_off[0] == 0 and g_path.size == g_off[k]
    assert np.array_equal(g_status, status[sel]) and np.array_equal(g_pops, pops[sel])
    for j, i in enumerate(sel):
        assert np.array_equal(g_path[g_off[j]:g_off[j + 1]], path[off[i]:off[i + 1]]), (k, j)


def _raw(p, c, st=..., gl=..., t0=..., k=None, max_time=None, max_nodes=65536, path=None, cap=0, nr=..., n_node=None,
         with_off=True):
    """The C entry point on sentinel-filled outputs."""
    a = c.arrays()
    st = a[0] if st is ... else st
    gl = a[1] if gl is ... else gl
    t0 = a[2] if t0 is ... else t0
    nr = a[3] if nr is ... else nr
    er = a[4]
    k = a[1].size if k is None else k
    off = np.full(k + 1, FILL, dtype=np.uint32)
    status = np.full(max(k, 1), FILL, dtype=np.uint32)
    pops = np.full(max(k, 1), FILL, dtype=np.uint32)
    tot = ctypes.c_uint32(FILL)

    def ptr(x):
        return x.ctypes.data_as(_U32P) if x is not None else None

    rc = p._lib.tsw_astar_reserved(p._ctx, ptr(st), ptr(gl), ptr(t0), k, ptr(nr),
                                   (nr.shape[0] if nr is not None else 0) if n_node is None else n_node, ptr(er), er.shape[0],
                                   c.max_time if max_time is None else max_time, max_nodes, ptr(off) if with_off else None,
                                   ptr(path), cap, ptr(status), ptr(pops), ctypes.byref(tot))
    return rc, off, status, pops, tot.value


def test_size_query_and_overflow_leave_path_untouched(planners):
    c = sm.by_name("random12-0")
    p = planners(c.rows)
    off_e, path_e, status_e, pops_e = c.expected()[:4]
    rc, off, status, pops, tot = _raw(p, c)
    assert rc == TSW_EOVERFLOW and tot == path_e.size
    assert np.array_equal(off, off_e) and np.array_equal(status, status_e) and np.array_equal(pops, pops_e)
    small = np.full(tot - 1, 0xCDCDCDCD, dtype=np.uint32)
    rc, off, status, pops, tot2 = _raw(p, c, path=small, cap=small.size)
    assert rc == TSW_EOVERFLOW and tot2 == tot and (small == 0xCDCDCDCD).all()
    assert np.array_equal(off, off_e) and np.array_equal(status, status_e) and np.array_equal(pops, pops_e)
    exact = np.full(tot, 0xCDCDCDCD, dtype=np.uint32)
    rc, off, status, pops, tot3 = _raw(p, c, path=exact, cap=exact.size)
    assert rc == TSW_OK and tot3 == tot and np.array_equal(exact, path_e)
    rc, off, _, _, tot0 = _raw(p, c, k=0)
    assert rc == TSW_OK and off[0] == 0 and tot0 == 0


def test_einval_leaves_the_outputs_untouched(planners):
    c = sm.by_name("random12-0")
    p = planners(c.rows)
    st, gl, t0, nr, er = c.arrays()
    blocked = np.uint32("".join(c.rows).index("@"))
    bad_cell, bad_time, off_grid = st.copy(), t0.copy(), st.copy()
    bad_cell[3] = blocked
    bad_time[5] = (1 << 20) + 1
    off_grid[0] = c.w * c.h
    for kw in (dict(st=bad_cell), dict(gl=bad_cell), dict(st=off_grid), dict(gl=off_grid), dict(t0=bad_time),
               dict(max_time=(1 << 20) + 1), dict(max_nodes=0), dict(st=None), dict(t0=None), dict(nr=None, n_node=3),
               dict(path=None, cap=4)):
        rc, off, status, pops, tot = _raw(p, c, **kw)
        assert rc == TSW_EINVAL, kw
        assert (off == FILL).all() and (status == FILL).all() and (pops == FILL).all() and tot == FILL, kw
    rc, off, status, pops, tot = _raw(p, c, with_off=False)
    assert rc == TSW_EINVAL and (status == FILL).all() and tot == FILL
    _assert_same(_device(p, c), c.expected(), "after the refused calls")  # the context still works


def test_refused_inside_a_resolver():
    """A context inside its own next-hop resolver refuses the call: TSW_EINVAL, the outputs untouched."""
    c = sm.by_name("random12-0")
    starts, tasks = maps.make_instance(c.rows, 6, 12, 3)
    seen = []
    with Planner(c.rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        def resolve(start, goal):
            rc, off, status, pops, tot = _raw(p, c)
            seen.append((rc, bool((off == FILL).all() and (status == FILL).all() and (pops == FILL).all() and tot == FILL)))
            with pytest.raises(pkg.TswapError) as ei:
                _device(p, c)
            seen.append((ei.value.code, True))
            return pkg.host_next_hop_codes(c.rows, start, goal)

        p.plan_mapd_resolved(starts, tasks, 200, resolve)
        _assert_same(_device(p, c), c.expected(), "after the plan")  # and works again once the plan is over
    assert seen and set(seen) == {(TSW_EINVAL, True)}


def test_a_plan_is_the_same_before_and_after(planners):
    """The call reads the grid only: stats() is unchanged by it and a plan after it equals the plan before."""
    rows = maps.random_map(16, 16, 0.2, 7)
    starts, tasks = maps.make_instance(rows, 10, 20, 7)
    free = np.nonzero(maps.rows_to_array(rows).reshape(-1) != ord("@"))[0].astype(np.uint32)
    with Planner(rows) as p:
        first = p.plan_mapd_arrays(starts, tasks, 400, trace_goals=True)
        before = p.stats()
        rec = first[0]
        x, y = (rec & np.uint64(0xFFFF)).astype(np.uint32), ((rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint32)
        cell = y * 16 + x
        t = np.broadcast_to(np.arange(rec.shape[1], dtype=np.uint32), cell.shape)
        nr = np.stack([cell.reshape(-1), t.reshape(-1)], axis=1)  # every record a reserved vertex
        off, path, status, pops = p.astar_reserved(free[:40], free[::-1][:40], 1, nr, None, 64)
        assert (status == pkg.TSW_SP_FOUND).any() and pops.sum() > 0
        after = p.stats()
        assert after == before
        second = p.plan_mapd_arrays(starts, tasks, 400, trace_goals=True)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
