"""Shared helpers of the table entry-point tests (test_gpu_table_io.py, test_gpu_store_lifecycle.py,
test_gpu_workers.py): a device buffer with guard bands around a payload that starts at a chosen byte shift, the
audit of everything a context's table store holds for a set of goals, and the grids / goal sets of the
odd-sized cases. No GPU use at import; test_table_io_cases.py checks the audit on the CPU. No test in here."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import worker_cases as wc
from p2p_distributed_tswap_amd import maps
from test_gpu_bfs import _DevBuf
from worker_cases import ASTAR as _ASTAR, NH_UNKNOWN, MapRef

NH_PENDING, NH_PENDING_S = 0xFE, 0xFD  # a producer's "queued for K3" markers (tsw_internal.h)
GUARD, FILL = 256, 0xA5


class GuardedDevBuf(_DevBuf):
    """`payload` bytes of device memory starting `shift` bytes past a 256-byte guard band, with another
    band behind them; the whole allocation is filled with 0xA5. The bands are wider than any single store
    the kernels issue (64 B), so a store that leaves the payload lands in memory this buffer owns, and
    guards_intact() finds it."""

    def __init__(self, payload: int, shift: int = 0):
        assert 0 <= shift < GUARD
        super().__init__(payload + 2 * GUARD)
        self.payload, self.shift = payload, shift
        assert self.hip.hipMemset(self.ptr, FILL, self.ct.c_size_t(self.nbytes)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    @property
    def addr(self) -> int:
        """Device address of the payload's first byte."""
        return self.ptr.value + GUARD + self.shift

    def from_host(self, arr: np.ndarray, byte_offset: int = 0):
        arr = np.ascontiguousarray(arr)
        assert 0 <= byte_offset and byte_offset + arr.nbytes <= self.payload
        assert self.hip.hipMemcpy(self.ct.c_void_p(self.addr + byte_offset), arr.ctypes.data_as(self.ct.c_void_p),
                                  self.ct.c_size_t(arr.nbytes), 1) == 0  # hipMemcpyHostToDevice

    def _all(self) -> np.ndarray:
        return self.to_host(np.empty(self.nbytes, dtype=np.uint8))

    def read(self, dtype, shape) -> np.ndarray:
        """The payload's first bytes as an array of `shape`."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert n <= self.payload
        lo = GUARD + self.shift
        return self._all()[lo:lo + n].copy().view(dtype).reshape(shape)

    def guard_damage(self) -> str:
        """'' while every guard byte still holds the filler, else where the bands were written."""
        raw = self._all()
        lo = GUARD + self.shift
        front, back = np.flatnonzero(raw[:lo] != FILL), np.flatnonzero(raw[lo + self.payload:] != FILL)
        msg = []
        if front.size:
            msg.append(f"{front.size} bytes written before the payload, the nearest {lo - int(front[-1])} B in front")
        if back.size:
            msg.append(f"{back.size} bytes written behind the payload, the farthest {int(back[-1]) + 1} B past its end")
        return "; ".join(msg)

    def guards_intact(self, what: str = ""):
        damage = self.guard_damage()
        assert not damage, f"{what}: {damage}"


def audit_tables(tabs: np.ndarray, ref: MapRef, goals, what: str):
    """`tabs[k]` = the next-hop codes a store holds for goals[k]: every code != 0xFF at a free cell equals the
    oracle's (none skipped or sampled), no code is a pending marker, cells K1 alone decides are resolved,
    blocked cells hold 0xFF. Returns the number of A*-decided codes that were checked."""
    pairs, where = [], []
    for k, goal in enumerate(goals):
        got, k1 = tabs[k], ref.k1(int(goal))
        pend = np.flatnonzero((got == NH_PENDING) | (got == NH_PENDING_S))
        assert pend.size == 0, (f"{what}: goal {goal}: {pend.size} pending markers left in the store, first cell "
                                f"{pend[0]} holds 0x{got[pend[0]]:02x}")
        assert (got[~ref.free] == NH_UNKNOWN).all(), f"{what}: goal {goal}: a blocked cell holds a code"
        res = ref.free & (got != NH_UNKNOWN)
        bad = np.flatnonzero(res & (k1 != _ASTAR) & (got != k1))
        assert bad.size == 0, (f"{what}: goal {goal}: {bad.size} BFS-decided codes differ, first cell {bad[0]} "
                               f"got {got[bad[0]]} want {k1[bad[0]]}")
        # cells K1 alone decides are never left unresolved
        assert not (ref.free & (k1 != _ASTAR) & (got == NH_UNKNOWN)).any(), f"{what}: goal {goal}: K1 code missing"
        for c in np.flatnonzero(res & (k1 == _ASTAR)):
            pairs.append((int(c), int(goal)))
            where.append(k)
    want = ref.astar_codes(pairs)
    got = np.array([tabs[k][c] for (c, _), k in zip(pairs, where)], dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    if bad.size:
        c, goal = pairs[bad[0]]
        delta, multi = wc.detour_classes(ref.og, ref.cells, goal)
        pytest.fail(f"{what}: {bad.size} of {len(pairs)} A*-decided codes in the store differ from get_path; first "
                    f"(cell {c}, goal {goal}): got {got[bad[0]]} want {want[bad[0]]}, delta {delta[c]}, "
                    f"multi-candidate {bool(multi[c])}")
    return len(pairs)


def check_store(p, ref: MapRef, goals, what: str):
    """Everything the store holds for `goals` (audit_tables over p.next_hop_tables). Returns the tables (goal
    order: np.unique(goals)), those goals and the number of A*-decided codes that were checked."""
    goals = np.unique(np.asarray(goals, dtype=np.uint32))
    tabs = p.next_hop_tables(goals)
    n = audit_tables(tabs, ref, goals, what)
    return tabs, goals, n


# ---- the odd-sized grids of test_gpu_table_io.py -------------------------------------------------------------

GRIDS = {
    "rand33x17": lambda: maps.random_map(33, 17, 0.25, 11),    # 561 cells: odd
    "rand100x31": lambda: maps.random_map(100, 31, 0.35, 5),   # 3,100 cells: % 8 == 4
    "col1x40": lambda: maps.open_map(1, 40),                   # single column
    "row40x1": lambda: maps.open_map(40, 1),                   # single row
    "rand64x20": lambda: maps.random_map(64, 20, 0.2, 3),      # W % 32 == 0: full 32-cell row words
    "rand70x130": lambda: maps.random_map(70, 130, 0.25, 7),   # 390 row words: k_bfs_blk's write-out loop runs twice
}


@functools.lru_cache(maxsize=None)
def grid_ref(name: str) -> MapRef:
    """The MapRef of a GRIDS map, made once and shared (read-only results)."""
    return MapRef(GRIDS[name]())


@functools.lru_cache(maxsize=None)
def grid_goals(name: str) -> np.ndarray:
    """13 distinct goals: the first and the last free cell and 11 seeded free cells between them (an odd count:
    the last pair of k_bfs_blk's two-goals-per-wave variant has a goal-less upper half)."""
    ref = grid_ref(name)
    free = np.flatnonzero(ref.free).astype(np.uint32)
    mid = np.random.default_rng(0x7AB1E).choice(free[1:-1], 11, replace=False)
    goals = np.concatenate([mid, free[:1], free[-1:]]).astype(np.uint32)
    assert np.unique(goals).size == 13
    goals.setflags(write=False)
    return goals


@functools.lru_cache(maxsize=None)
def grid_tables(name: str) -> np.ndarray:
    """og.bfs of every grid_goals(name) goal, (13, ncell) u16, computed once and shared (read-only)."""
    ref = grid_ref(name)
    t = np.stack([ref.og.bfs(int(g)) for g in grid_goals(name)])
    t.setflags(write=False)
    return t


def first_table_diff(got: np.ndarray, want: np.ndarray, goals) -> str:
    """'' when the (k, ncell) arrays agree, else a description of the first differing table."""
    if np.array_equal(got, want):
        return ""
    k = int(np.argmax((got != want).any(axis=1)))
    bad = np.flatnonzero(got[k] != want[k])
    return (f"table {k} (goal {int(goals[k])}): {bad.size} cells differ, first cell {int(bad[0])} got "
            f"{int(got[k][bad[0]])} want {int(want[k][bad[0]])}")


def goalset(rows, starts, tasks) -> np.ndarray:
    """Every cell a plan of (starts, tasks) can use as a goal: starts, pickups, deliveries (sorted, distinct)."""
    w = len(rows[0])
    cells = np.concatenate([starts[:, 1] * w + starts[:, 0], tasks[:, 1] * w + tasks[:, 0],
                            tasks[:, 3] * w + tasks[:, 2]])
    return np.unique(cells.astype(np.uint32))
