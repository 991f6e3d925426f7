"""CPU: the space-time A* with reservations (tsw_astar_reserved's definition, include/tswap.h). The model
(tests/st_astar_model.py, a_star.rs:32-112 restated) against an independent formulation — the earliest arrival of
a plain BFS over the time-expanded graph — and the host twin tsw_host_astar_reserved (csrc/tsw_host_st_astar.cpp)
against the model: paths, status and pops on the shared case list. No device is involved."""
import ctypes
import os

import numpy as np
import pytest

import p2p_distributed_tswap_amd as pkg
import st_astar_model as sm

CASES = [c.name for c in sm.all_cases()]


def _lib_or_skip():
    if not os.path.exists(pkg.LIB_PATH):
        pytest.skip("libtswap_hip.so not built (run __graft_entry__.build())")


def _host(c, max_nodes=None):
    st, gl, t0, nr, er = c.arrays()
    return pkg.host_astar_reserved(c.rows, st, gl, t0, nr, er, c.max_time, c.max_nodes if max_nodes is None else max_nodes)


def _assert_equal(got, c):
    off, path, status, pops = c.expected()[:4]
    for name, g, e in zip(("status", "pops", "path_off", "path"), (got[2], got[3], got[0], got[1]), (status, pops, off, path)):
        if not np.array_equal(g, e):
            i = int(np.nonzero(g != e)[0][0]) if g.shape == e.shape else -1
            raise AssertionError(f"{c.name}: {name} differs (first at {i}: got {g[i] if i >= 0 else g.shape}, "
                                 f"model {e[i] if i >= 0 else e.shape})")


# ---- 1. the model against an independent formulation ---------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_arrives_as_early_as_the_time_expanded_bfs(name):
    c = sm.by_name(name)
    off, path, status, pops, pushes = c.expected()[:5]
    ns, es = set(c.node_res), set(c.edge_res)
    for i, (s, g, t0) in enumerate(c.queries):
        p = [(int(v) % c.w, int(v) // c.w) for v in path[off[i]:off[i + 1]]]
        bfs = sm.earliest_arrival(c.rows, s, g, t0, ns, es, c.max_time)
        if status[i] == sm.FOUND:
            assert bfs is not None and len(p) - 1 == bfs - t0, (name, i)
            assert p[0] == s and p[-1] == g
            for j in range(len(p) - 1):  # every step passes the filter
                assert (p[j + 1], t0 + j + 1) in sm.successors(c.rows, p[j], t0 + j, ns, es), (name, i, j)
        elif status[i] == sm.NONE:
            assert bfs is None, (name, i)  # nothing arrives by max_time
        assert pops[i] <= pushes[i] <= c.max_nodes


def test_open_8x8_model_paths_are_shortest():
    c = sm.open_case()
    off, path, status, pops = c.expected()[:4]
    assert len(c.queries) == 4032 and (status == sm.FOUND).all()
    for i, (s, g, _) in enumerate(c.queries):
        assert off[i + 1] - off[i] == abs(s[0] - g[0]) + abs(s[1] - g[1]) + 1


def test_random_cases_search():
    """Equality on cases that never search proves nothing: the model alone finds at least 80 % of the random
    queries and none runs into the capacity."""
    status = np.concatenate([sm.by_name(f"random12-{i}").expected()[2] for i in range(6)])
    assert status.size == 300
    assert (status == sm.FOUND).sum() >= 0.8 * status.size
    assert (status == sm.CAPACITY).sum() == 0


def test_big_heap_case_passes_the_lds_heap():
    """The case is there for the kernel's move of a heap from LDS (512 entries) to global memory."""
    assert max(sm.by_name("big-heap-40").expected()[5]) > 512
    assert max(max(c.expected()[5]) for c in sm.all_cases() if c.name != "big-heap-40") < 512


def test_hand_cases_show_their_rule():
    e = {c.name: c.expected() for c in sm.hand_cases()}
    p = list(e["goal-reserved-until-5"][1])
    assert len(p) == 7 and p[-1] == 3 and 3 not in p[:-1]  # arrival at t = 6
    p = list(e["head-on-edge"][1])
    assert len(p) == 6 and p[-1] == 4 and (p[1], p[2]) != (1, 2)  # one step lost: a wait or a step back
    assert list(e["head-on-edge-3x3"][1]) == [0, 0, 1, 2]  # (0,0) -> (1,0) at t = 1 is the reserved edge reversed
    # at (1, 0) with t = 1 nothing may be generated and (1, 0) itself is taken at t = 2: it is entered at t = 3
    assert list(e["reserved-current-cell"][1]) == [0, 0, 0, 1, 2, 3]
    assert list(e["no-wait-edge"][1]) == [1, 0, 1, 2, 3]  # neither forward nor waiting at t = 1: one step back
    assert e["boxed-in"][2][0] == sm.NONE and e["boxed-in"][3][0] == 1
    assert e["walled-off"][2][0] == sm.NONE
    assert e["walled-off-capacity"][2][0] == sm.CAPACITY and e["walled-off-capacity"][4][0] == 8
    assert list(e["start-is-goal"][1]) == [2] and e["start-is-goal"][3][0] == 1
    assert e["too-far"][2][0] == sm.NONE and e["too-far"][3][0] == 0
    assert list(e["inert-reservations"][1]) == [0, 1, 2, 3, 4, 5]


# ---- 2. the host twin against the model -------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_twin_equals_the_model(name):
    _lib_or_skip()
    c = sm.by_name(name)
    _assert_equal(_host(c), c)


def test_host_twin_open_8x8_all_pairs():
    """Every ordered pair of the open 8x8 grid: the BinaryHeap's tie-break decides the path."""
    _lib_or_skip()
    c = sm.open_case()
    _assert_equal(_host(c), c)


def test_host_twin_contract():
    """The size query, TSW_EOVERFLOW with path untouched, the TSW_EINVAL cases and k == 0, through the C ABI."""
    _lib_or_skip()
    lib = pkg.load_library(pkg.LIB_PATH)
    c = sm.by_name("random12-0")
    st, gl, t0, nr, er = c.arrays()
    off_e, path_e, status_e, pops_e = c.expected()[:4]
    cells, w, h = pkg.grid_to_bytes(c.rows)
    P, u32 = ctypes.POINTER, ctypes.c_uint32

    def p(a):
        return a.ctypes.data_as(P(u32)) if a is not None else None

    def call(st=st, gl=gl, t0=t0, k=None, max_time=c.max_time, max_nodes=65536, path=None, cap=0, cells=cells, nr=nr,
             n_node=None):
        k = gl.size if k is None else k
        off = np.full(k + 1, 0xABABABAB, dtype=np.uint32)
        status = np.full(max(k, 1), 0xABABABAB, dtype=np.uint32)
        pops = np.full(max(k, 1), 0xABABABAB, dtype=np.uint32)
        tot = u32(0xABABABAB)
        rc = lib.tsw_host_astar_reserved(cells.ctypes.data_as(P(ctypes.c_uint8)) if cells is not None else None, w, h,
                                         p(st), p(gl), p(t0), k, p(nr), nr.shape[0] if n_node is None else n_node,
                                         p(er), er.shape[0], max_time, max_nodes, p(off), p(path), cap, p(status),
                                         p(pops), ctypes.byref(tot))
        return rc, off, status, pops, tot.value

    rc, off, status, pops, tot = call()  # the size query
    assert rc == pkg.TSW_EOVERFLOW and tot == path_e.size
    assert np.array_equal(off, off_e) and np.array_equal(status, status_e) and np.array_equal(pops, pops_e)
    small = np.full(tot - 1, 0xCDCDCDCD, dtype=np.uint32)
    rc, off, status, pops, tot2 = call(path=small, cap=small.size)
    assert rc == pkg.TSW_EOVERFLOW and tot2 == tot and (small == 0xCDCDCDCD).all() and np.array_equal(off, off_e)
    rc, off, _, _, tot = call(k=0)
    assert rc == pkg.TSW_OK and off[0] == 0 and tot == 0
    blocked = np.uint32(next(i for i, ch in enumerate("".join(c.rows)) if ch == "@"))
    bad_start, bad_time = st.copy(), t0.copy()
    bad_start[3] = blocked
    bad_time[5] = (1 << 20) + 1
    off_grid = st.copy()
    off_grid[0] = w * h
    for kw in (dict(st=bad_start), dict(gl=bad_start), dict(st=off_grid), dict(t0=bad_time), dict(max_time=(1 << 20) + 1),
               dict(max_nodes=0), dict(cells=None), dict(st=None), dict(nr=None, n_node=3), dict(path=None, cap=4)):
        rc, off, status, pops, tot = call(**kw)
        assert rc == pkg.TSW_EINVAL, kw
        assert (off == 0xABABABAB).all() and (status == 0xABABABAB).all() and (pops == 0xABABABAB).all() and tot == 0xABABABAB
