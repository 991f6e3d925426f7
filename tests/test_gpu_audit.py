"""GPU: tsw_audit_records / tsw_audit_records_device. The device's sum, col and agent words must equal
audit_model.audit_model's word for word (integer work: no tolerance), on: the smallest shapes, the tile and
wave edges of both passes, columns that reuse a workgroup's table under new tags, stride > T with the unused
columns and pad bytes set, the hand-built cases, random records, grids on either side of the LDS / global
table placement, and the records of real fleet_mapd / plan_mapd_arrays runs; then the documented contract:
the TSW_EINVAL cases with the outputs untouched, re-entry from a resolver, and a plan around an audit."""
import ctypes
import functools

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg
from p2p_distributed_tswap_amd import Planner, TswapError, maps, TSW_EINVAL, TSW_OK, TSW_F_LAZY_NEXTHOP
from p2p_distributed_tswap_amd import Audit, _Rec

import audit_model as am
import fleet_mapd_model as mm

pytestmark = pytest.mark.gpu

# the kernels' constants (csrc/tsw_audit.h): pass A works on tiles of AUD_TILE_AGENTS agents x AUD_TILE_COLS
# columns, a wave per agent row; pass B strides the columns over at most AUD_G_MAX workgroups
AUD_TILE_AGENTS, AUD_TILE_COLS, AUD_G_MAX = 64, 64, 128

_U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xDEADBEEF
SMALL = maps.random_map(20, 16, 0.2, 5)  # 320 cells: the table lives in LDS


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


def _check(p, rows, rec, what=""):
    """audit(rec) with every output against the model, and the summary alone (col / agent NULL) against it."""
    ref = am.audit_model(rows, rec)
    got = p.audit(rec, col=True, agents=True)
    am.assert_equal(got, ref, what)
    alone = p.audit(rec)
    assert "col" not in alone and alone == {k: got[k] for k in alone}, what
    return got


def _raw(p, rec_ptr, n, T, stride, fn="tsw_audit_records", with_sum=True):
    """The C entry point on sentinel-filled outputs: (rc, sum bytes, col, agent)."""
    sm = Audit()
    ctypes.memset(ctypes.byref(sm), 0xAB, ctypes.sizeof(sm))
    col = np.full((max(min(T, 4096), 1), am.NCOL), FILL, dtype=np.uint32)
    ag = np.full((max(n, 1), am.NAGENT), FILL, dtype=np.uint32)
    rc = getattr(p._lib, fn)(p._ctx, rec_ptr, n, T, stride, ctypes.byref(sm) if with_sum else None,
                             col.ctypes.data_as(_U32P), ag.ctypes.data_as(_U32P))
    return rc, bytes(sm), col, ag


# ---- the smallest shapes, the tile and wave edges -----------------------------------------------------

def test_one_record(planners):
    got = _check(planners(SMALL), SMALL, am.records([[(0, 0, am.DELIVERED)]]))
    assert got["deliveries"] == 1 and got["moving_columns"] == 0


@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (0, 0)])
def test_nothing_to_audit(planners, shape):
    p = planners(SMALL)
    got = p.audit(np.zeros(shape, dtype=np.uint64), col=True, agents=True)
    am.assert_equal(got, am.audit_model(SMALL, np.zeros(shape, dtype=np.uint64)))
    assert got["first_t"] == got["first_agent"] == [am.NONE] * am.NKIND and got["state_steps"] == [0] * 4
    # col and agent are not written
    rec = np.zeros(max(shape[0] * shape[1], 1), dtype=np.uint64)
    rc, sm, col, ag = _raw(p, rec.ctypes.data_as(ctypes.POINTER(_Rec)), shape[0], shape[1], shape[1])
    assert rc == TSW_OK and np.all(col == FILL) and np.all(ag == FILL)
    assert Audit.from_buffer_copy(sm).as_dict() == {k: got[k] for k in Audit().as_dict()}
    # a NULL rec is fine when there is nothing to read
    assert _raw(p, None, shape[0], shape[1], shape[1])[0] == TSW_OK


@pytest.mark.parametrize("T", [1, 2, AUD_TILE_COLS // 2 + 1, AUD_TILE_COLS + 1])
@pytest.mark.parametrize("n", [AUD_TILE_AGENTS - 1, AUD_TILE_AGENTS, AUD_TILE_AGENTS + 1, 4 * AUD_TILE_AGENTS + 1])
def test_tile_and_wave_edges(planners, n, T):
    _check(planners(SMALL), SMALL, am.random_records(SMALL, n, T, 100 * n + T, dup=0.1, off=0.03, bad=0.03, jump=0.03))


def test_every_workgroup_reuses_its_table(planners):
    """T = 3 * AUD_G_MAX + 1 columns: every workgroup of pass B audits three or four columns on one table,
    each under a new tag. The agents trade places and pile up, so stale entries of the same cells abound."""
    T = 3 * AUD_G_MAX + 1
    rec = np.concatenate([am.swap_walks(SMALL, 4, T, 7), am.random_records(SMALL, 5, T, 8, dup=0.3)])
    got = _check(planners(SMALL), SMALL, rec)
    assert got["swaps"] >= 4 * (T - 1) and got["colocations"] > 0


def test_stride_past_T_and_pad_bytes_are_ignored(planners):
    p = planners(SMALL)
    rows, rec, ref = am.random_case(1)
    n, T = rec.shape
    wide = np.full((n, T + 7), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    wide[:, :T] = rec | np.uint64(0xFFFFFF << 40)
    sm = Audit()
    col = np.zeros((T, am.NCOL), dtype=np.uint32)
    ag = np.zeros((n, am.NAGENT), dtype=np.uint32)
    assert p._lib.tsw_audit_records(p._ctx, wide.ctypes.data_as(ctypes.POINTER(_Rec)), n, T, T + 7, ctypes.byref(sm),
                                    col.ctypes.data_as(_U32P), ag.ctypes.data_as(_U32P)) == TSW_OK
    am.assert_equal({**sm.as_dict(), "col": col, "agents": ag}, ref, "stride > T")
    am.assert_equal(p.audit(rec, col=True, agents=True), ref, "stride == T")


# ---- hand-built and random records -----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(am.HAND))
def test_hand_built_cases(planners, name):
    got = _check(planners(am.HAND_ROWS), am.HAND_ROWS, am.HAND[name][0], name)
    for k, v in am.hand_expected(name).items():
        assert got[k] == v, (name, k)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_records(planners, seed):
    rows, rec, ref = am.random_case(seed)
    am.assert_equal(planners(rows).audit(rec, col=True, agents=True), ref, f"seed {seed}")


# ---- where the table lives ---------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(170, 84), (256, 256), (2048, 512)], ids=["lds-14280", "global-65536", "global-2^20"])
def test_table_placement(w, h):
    """14,280 cells (the C3 warehouse's size) fit the LDS table, 65,536 cells are past any LDS table, 2^20
    cells are the grid limit; agents stand in the last row, the last column and the last corner."""
    rows = am.edge_rows(w, h)
    rec = am.edge_records(w, h, 300, 40, w)
    with Planner(rows) as p:
        got = _check(p, rows, rec, f"{w}x{h}")
    assert got["swaps"] >= 2 * 39 and got["colocations"] > 0 and got["off_map"] > 0


# ---- records of real runs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dense12", "rand20"])
def test_fleet_mapd_records(planners, name):
    rows, starts, tasks, r, max_t, _ = mm.instance(name)
    run = mm.run_case(name)
    p = planners(rows)
    rec, _ = p.fleet_mapd(starts, tasks, max_t, r)
    assert np.array_equal(rec, run.rec)
    got = _check(p, rows, rec, name)
    assert got["colocations"] == run.colocated
    assert got["moving_columns"] == maps.moving_timesteps(rec)


@functools.lru_cache(maxsize=None)
def _busy():
    rows = maps.random_map(16, 16, 0.2, 7)
    return rows, *maps.make_instance(rows, 10, 20, 7)


def test_plan_records_and_the_device_form(planners):
    """The device memory comes from the HIP runtime the library links (GuardedDevBuf), not from a torch tensor:
    torch's bundled runtime cannot open the device in a process where the library's already has
    (test_gpu_bfs._DevBuf). The entry point sees an address either way."""
    from table_io_cases import GuardedDevBuf

    rows, starts, tasks = _busy()
    p = planners(rows)
    rec, _ = p.plan_mapd_arrays(starts, tasks, 2000)
    got = _check(p, rows, rec, "plan")
    assert got["colocations"] == got["swaps"] == got["off_map"] == got["bad_state"] == 0 and got["deliveries"] > 0
    assert got["moving_columns"] == maps.moving_timesteps(rec)
    # the same records in device memory, read in place: contiguous, and as the left part of wider rows whose
    # other columns and pad bytes are all ones; the second buffer starts 8 bytes off a 256-byte boundary
    n, T = rec.shape
    wide = np.full((n, T + 5), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    wide[:, :T] = rec | np.uint64(0xFFFFFF << 40)
    for host, stride, shift in ((rec, T, 0), (wide, T + 5, 8)):
        dev = GuardedDevBuf(host.nbytes, shift)
        dev.from_host(host)
        there = p.audit_device(dev.addr, n, T, stride, col=True, agents=True)
        for k in got:
            assert np.array_equal(there[k], got[k]), (k, stride)
        dev.guards_intact(f"stride {stride}")
        assert np.array_equal(dev.read(np.uint64, host.shape), host)  # read, never written


# ---- the contract ------------------------------------------------------------------------------------------------

def test_einval_leaves_the_outputs_untouched(planners):
    p = planners(SMALL)
    rows, rec, ref = am.random_case(1)
    n, T = rec.shape
    rp = rec.ctypes.data_as(ctypes.POINTER(_Rec))
    untouched = b"\xab" * ctypes.sizeof(Audit)
    for fn in ("tsw_audit_records", "tsw_audit_records_device"):
        for label, args in (("stride < T", (rp, n, T, T - 1)), ("NULL rec", (None, n, T, T)),
                            ("T past the limit", (rp, n, (1 << 20) + 2, (1 << 20) + 2))):
            rc, sm, col, ag = _raw(p, *args, fn=fn)
            assert rc == TSW_EINVAL, (fn, label)
            assert sm == untouched and np.all(col == FILL) and np.all(ag == FILL), (fn, label)
        rc, _, col, ag = _raw(p, rp, n, T, T, fn=fn, with_sum=False)
        assert rc == TSW_EINVAL and np.all(col == FILL) and np.all(ag == FILL), fn
    with pytest.raises(TswapError) as ei:
        p.audit(np.zeros(3, dtype=np.uint64))
    assert ei.value.code == TSW_EINVAL
    am.assert_equal(p.audit(rec, col=True, agents=True), ref, "after the refusals")


def test_refused_inside_a_resolver():
    rows, starts, tasks = _busy()
    _, rec, _ = am.random_case(1)
    refused = []
    with Planner(rows, flags=TSW_F_LAZY_NEXTHOP) as p:
        def resolve(start, goal):
            with pytest.raises(TswapError) as ei:
                p.audit(rec)
            refused.append(ei.value.code)
            return pkg.host_next_hop_codes(rows, start, goal)

        p.plan_mapd_resolved(starts, tasks, 2000, resolve)
    assert refused and set(refused) == {TSW_EINVAL}


def test_a_plan_is_the_same_around_an_audit():
    rows, starts, tasks = _busy()
    rec = am.random_case(2)[1]
    ref = am.audit_model(rows, rec)  # a 20 x 16 map's records on this 16 x 16 grid: plenty of them off it
    with Planner(rows) as p:
        first = p.plan_mapd_arrays(starts, tasks, 2000, trace_goals=True)
        before = p.stats()
        am.assert_equal(p.audit(rec, col=True, agents=True), ref)
        p.audit(first[0])
        after = p.stats()
        assert after["tables"] == before["tables"] and after == before  # the audit touches no counter
        second = p.plan_mapd_arrays(starts, tasks, 2000, trace_goals=True)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
