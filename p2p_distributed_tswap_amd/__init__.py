"""MI355X-native TSWAP planning core — Python mirror of the reference interface.

Drop-in for the src/algorithm path of RenKoya1/p2p_distributed_tswap
(@ 2025-11-21). Everything here is a thin ctypes layer over the C ABI in
include/tswap.h (libtswap_hip.so: hand-written gfx950 HIP kernels + C++ host
runtime). There is NO CPU fallback: if the HIP library or a GPU is missing,
every call raises.

Reference interface mirrored (same names, argument meaning, error behaviour):
  tswap_mapd(grid, initial_positions, tasks)  src/algorithm/tswap.rs:39-43
      -> list[list[((x, y), AgentState)]]; panics become TswapError(EINVAL)
  AgentState                                  src/map/agent.rs:9-15
  Task(pickup, delivery, peer_id, task_id)    src/map/task_generator.rs:6-12
  Point = (x, y)                              src/map/map.rs:4
"""
from __future__ import annotations

import ctypes
import enum
import os
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence

import numpy as np

__all__ = [
    "AgentState", "Task", "TswapError", "Planner", "tswap_mapd", "tswap_step",
    "load_library", "LIB_PATH", "grid_to_bytes", "build_id",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtswap_hip.so")
# diagnostic build (-DTSW_DIAG): the same kernels plus the TSW_* environment knobs (kernel A/B variants,
# instrumentation). Tests of the A/B variants and measurement scripts only; products load LIB_PATH.
DIAG_LIB_PATH = os.path.join(_HERE, "libtswap_hip_diag.so")

TSW_OK, TSW_EINVAL, TSW_ENOMEM, TSW_EHIP, TSW_EOVERFLOW = 0, -22, -12, -5, -75
TSW_ABI_VERSION = 8  # include/tswap.h
TSW_HOST_ASTAR_OFF = 0xFFFFFFFF  # tsw_opts.host_astar: no host A* service
TSW_F_EAGER_NEXTHOP, TSW_F_LAZY_NEXTHOP, TSW_F_EXIT_MODE = 1, 2, 4
# TswapAction (bin/decentralized/agent.rs:321-326), include/tswap.h TSW_ACT_*
TSW_ACT_MOVE, TSW_ACT_GOAL_SWAP, TSW_ACT_ROTATION, TSW_ACT_WAIT = 0, 1, 2, 3
# tsw_audit_records (include/tswap.h): words per column / per agent, violation kinds
TSW_AUDIT_NCOL, TSW_AUDIT_NAGENT, TSW_AUDIT_NKIND = 11, 4, 5
AUDIT_KINDS = ("colocation", "swap", "jump", "off_map", "bad_state")
# tsw_task_timeline (include/tswap.h): dispatch rules, words per task
TSW_TL_NEAREST, TSW_TL_STREAM, TSW_TL_NTASK = 0, 1, 4
TIMELINE_RULES = {"nearest": TSW_TL_NEAREST, "stream": TSW_TL_STREAM}
# tsw_astar_reserved (include/tswap.h): per-query status
TSW_SP_FOUND, TSW_SP_NONE, TSW_SP_CAPACITY = 0, 1, 2
DIST_INF = 0xFFFF


class AgentState(enum.IntEnum):
    """src/map/agent.rs:9-15 (discriminants in declaration order)."""
    PICKING = 0
    CARRYING = 1
    DELIVERED = 2
    IDLE = 3


@dataclass
class Task:
    """src/map/task_generator.rs:6-12. peer_id/task_id are carried, never read by the planner."""
    pickup: tuple
    delivery: tuple
    peer_id: Optional[str] = None
    task_id: Optional[int] = None


class TswapError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"tswap error {code}: {msg}")
        self.code = code


class _Point(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32)]


class _Task(ctypes.Structure):
    _fields_ = [("pickup", _Point), ("delivery", _Point)]


class _Rec(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint16), ("y", ctypes.c_uint16), ("state", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 3)]


class _Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("table_budget_bytes", ctypes.c_uint64), ("watchdog_ms", ctypes.c_uint32),
                ("host_astar", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [
        ("bfs_goals", ctypes.c_uint64), ("bfs_launches", ctypes.c_uint64), ("bfs_ms", ctypes.c_double),
        ("astar_queries", ctypes.c_uint64), ("astar_launches", ctypes.c_uint64), ("astar_ms", ctypes.c_double),
        ("walker_launches", ctypes.c_uint64), ("walker_ms", ctypes.c_double),
        ("assign_launches", ctypes.c_uint64), ("assign_ms", ctypes.c_double),
        ("steps", ctypes.c_uint64), ("tables", ctypes.c_uint64), ("plan_ms", ctypes.c_double),
        ("plan_section_ms", ctypes.c_double * 8), ("rule_rounds", ctypes.c_uint64),
        ("plan_exits", ctypes.c_uint64 * 8), ("table_evictions", ctypes.c_uint64),
        ("coop_waits", ctypes.c_uint64), ("coop_wait_ms", ctypes.c_double),
        ("coop_wait_sec_ms", ctypes.c_double * 8), ("coop_waits_sec", ctypes.c_uint64 * 8),
        ("relabels_full", ctypes.c_uint64), ("relabels_inc", ctypes.c_uint64),
        ("move_rounds", ctypes.c_uint64), ("plan_block", ctypes.c_uint32),
        ("coop_workers", ctypes.c_uint32), ("coop_worker_busy_ms", ctypes.c_double * 3),
        ("watchdog_fires", ctypes.c_uint64), ("tableless_goals", ctypes.c_uint64),
        ("coop_worker_queries", ctypes.c_uint64 * 3), ("coop_worker_pops", ctypes.c_uint64 * 3),
        ("host_astar_queries", ctypes.c_uint64), ("host_astar_used", ctypes.c_uint64),
        ("host_astar_ms", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["plan_section_ms"] = list(self.plan_section_ms)
        d["plan_exits"] = list(self.plan_exits)
        d["coop_wait_sec_ms"] = list(self.coop_wait_sec_ms)
        d["coop_waits_sec"] = list(self.coop_waits_sec)
        d["coop_worker_busy_ms"] = list(self.coop_worker_busy_ms)
        d["coop_worker_queries"] = list(self.coop_worker_queries)
        d["coop_worker_pops"] = list(self.coop_worker_pops)
        return d


class Audit(ctypes.Structure):
    """tsw_audit (include/tswap.h)."""
    _fields_ = [
        ("state_steps", ctypes.c_uint64 * 4), ("bad_state", ctypes.c_uint64), ("moves", ctypes.c_uint64),
        ("deliveries", ctypes.c_uint64), ("colocations", ctypes.c_uint64), ("swaps", ctypes.c_uint64),
        ("jumps", ctypes.c_uint64), ("off_map", ctypes.c_uint64), ("moving_columns", ctypes.c_uint32),
        ("first_t", ctypes.c_uint32 * 5), ("first_agent", ctypes.c_uint32 * 5),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("state_steps", "first_t", "first_agent"):
            d[k] = list(d[k])
        return d


class Timeline(ctypes.Structure):
    """tsw_timeline (include/tswap.h)."""
    _fields_ = [
        ("wait_sum", ctypes.c_uint64), ("service_sum", ctypes.c_uint64), ("carry_sum", ctypes.c_uint64),
        ("assigned", ctypes.c_uint32), ("carried", ctypes.c_uint32), ("delivered", ctypes.c_uint32),
        ("unreleased", ctypes.c_uint32), ("service_min", ctypes.c_uint32), ("service_max", ctypes.c_uint32),
        ("makespan", ctypes.c_uint32), ("consistent", ctypes.c_uint32), ("bad_kind", ctypes.c_uint32),
        ("bad_t", ctypes.c_uint32), ("bad_agent", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol declared in include/tswap.h (tests check the .so exports them)
EXPORTED_SYMBOLS = (
    "tsw_create", "tsw_destroy", "tsw_last_error", "tsw_plan_mapd", "tsw_plan_mapd_trace",
    "tsw_step", "tsw_get_path_next", "tsw_decide", "tsw_dist_tables", "tsw_dist_tables_device",
    "tsw_import_tables_device", "tsw_next_hop_tables", "tsw_next_hop_tables_device", "tsw_import_next_hops_device",
    "tsw_clear_tables", "tsw_get_stats", "tsw_reset_stats", "tsw_set_timing", "tsw_probe_round_floors",
    "tsw_abi_version", "tsw_plan_mapd_resolved", "tsw_next_hop_codes", "tsw_build_id",
    "tsw_host_next_hop_codes", "tsw_nearby", "tsw_decide_fleet", "tsw_fleet_apply", "tsw_fleet_run",
    "tsw_fleet_mapd", "tsw_audit_records", "tsw_audit_records_device", "tsw_plan_mapd_online",
    "tsw_task_timeline", "tsw_task_timeline_device", "tsw_probe_timeline",
    "tsw_astar_reserved", "tsw_host_astar_reserved", "tsw_probe_st_astar",
)

# tsw_resolve_fn (include/tswap.h): int (*)(void *user, uint32_t k, const uint32_t *start,
# const uint32_t *goal, uint8_t *code)
_RESOLVE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                               ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8))

_libs = {}


def load_library(path: str = LIB_PATH):
    """Load libtswap_hip.so (built by __graft_entry__.build()). Raises if absent."""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise TswapError(TSW_EHIP, f"HIP library not built: {path} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    # the ABI revision first: an older library lacks the newer symbols, and binding them
    # before this check would fail with a bare AttributeError instead of the rebuild message
    abi = None
    if hasattr(lib, "tsw_abi_version"):
        lib.tsw_abi_version.argtypes = []
        lib.tsw_abi_version.restype = ctypes.c_int
        abi = lib.tsw_abi_version()
    if abi != TSW_ABI_VERSION:
        raise TswapError(TSW_EINVAL, f"{path}: ABI {abi}, this binding mirrors {TSW_ABI_VERSION} "
                                     "(rebuild with __graft_entry__.build())")
    P = ctypes.POINTER
    u32, i32, u64 = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    vp = ctypes.c_void_p
    lib.tsw_create.argtypes = [P(ctypes.c_uint8), u32, u32, P(_Opts)]
    lib.tsw_create.restype = vp
    lib.tsw_destroy.argtypes = [vp]
    lib.tsw_destroy.restype = None
    lib.tsw_last_error.argtypes = [vp]
    lib.tsw_last_error.restype = ctypes.c_char_p
    lib.tsw_plan_mapd.argtypes = [vp, P(_Point), u32, P(_Task), u32, u32, P(_Rec), P(u32)]
    lib.tsw_plan_mapd_trace.argtypes = [vp, P(_Point), u32, P(_Task), u32, u32, P(_Rec), P(u32), P(u32)]
    lib.tsw_plan_mapd_online.argtypes = [vp, P(_Point), u32, P(_Task), P(u32), u32, u32, P(_Rec), P(u32), P(u32)]
    lib.tsw_plan_mapd_online.restype = ctypes.c_int
    lib.tsw_step.argtypes = [vp, P(u32), P(u32), u32]
    lib.tsw_get_path_next.argtypes = [vp, P(u32), P(u32), u32, P(u32), P(i32)]
    lib.tsw_decide.argtypes = [vp, P(u32), P(u32), u32, P(u32), P(u32), P(u32), P(u32), P(u32), P(u32), P(u32),
                               P(u32)]
    lib.tsw_nearby.argtypes = [vp, P(u32), u32, u32, P(u32), P(u32), u32, P(u32)]
    lib.tsw_nearby.restype = ctypes.c_int
    lib.tsw_decide_fleet.argtypes = [vp, P(u32), P(u32), u32, u32, P(u32), P(u32), P(u32), P(u32), P(u32), u32]
    lib.tsw_decide_fleet.restype = ctypes.c_int
    lib.tsw_fleet_apply.argtypes = [vp, P(u32), P(u32), u32, P(u32), P(u32), P(u32), P(u32), P(u32)]
    lib.tsw_fleet_apply.restype = ctypes.c_int
    lib.tsw_fleet_run.argtypes = [vp, P(u32), P(u32), u32, u32, u32, P(u32), P(u32), P(u32)]
    lib.tsw_fleet_run.restype = ctypes.c_int
    lib.tsw_fleet_mapd.argtypes = [vp, P(_Point), u32, P(_Task), u32, u32, u32, P(_Rec), P(u32), P(u32), P(u32), P(u32)]
    lib.tsw_fleet_mapd.restype = ctypes.c_int
    lib.tsw_audit_records.argtypes = [vp, P(_Rec), u32, u32, u32, P(Audit), P(u32), P(u32)]
    lib.tsw_audit_records.restype = ctypes.c_int
    lib.tsw_audit_records_device.argtypes = [vp, vp, u32, u32, u32, P(Audit), P(u32), P(u32)]
    lib.tsw_audit_records_device.restype = ctypes.c_int
    lib.tsw_task_timeline.argtypes = [vp, P(_Rec), u32, u32, u32, P(_Point), P(_Task), P(u32), u32, u32, P(Timeline),
                                      P(u32)]
    lib.tsw_task_timeline.restype = ctypes.c_int
    lib.tsw_task_timeline_device.argtypes = [vp, vp, u32, u32, u32, P(_Point), P(_Task), P(u32), u32, u32, P(Timeline),
                                             P(u32)]
    lib.tsw_task_timeline_device.restype = ctypes.c_int
    lib.tsw_probe_timeline.argtypes = [vp, P(ctypes.c_double)]
    lib.tsw_probe_timeline.restype = ctypes.c_int
    st_args = [P(u32), P(u32), P(u32), u32, P(u32), u32, P(u32), u32, u32, u32, P(u32), P(u32), u32, P(u32), P(u32), P(u32)]
    lib.tsw_astar_reserved.argtypes = [vp, *st_args]
    lib.tsw_astar_reserved.restype = ctypes.c_int
    lib.tsw_host_astar_reserved.argtypes = [P(ctypes.c_uint8), u32, u32, *st_args]
    lib.tsw_host_astar_reserved.restype = ctypes.c_int
    lib.tsw_probe_st_astar.argtypes = [vp, P(ctypes.c_double)]
    lib.tsw_probe_st_astar.restype = ctypes.c_int
    lib.tsw_dist_tables.argtypes = [vp, P(u32), u32, P(ctypes.c_uint16)]
    lib.tsw_dist_tables_device.argtypes = [vp, P(u32), u32, vp]
    lib.tsw_import_tables_device.argtypes = [vp, P(u32), u32, vp]
    lib.tsw_clear_tables.argtypes = [vp]
    lib.tsw_next_hop_tables.argtypes = [vp, P(u32), u32, P(ctypes.c_uint8)]
    lib.tsw_next_hop_tables_device.argtypes = [vp, P(u32), u32, vp, vp]
    lib.tsw_import_next_hops_device.argtypes = [vp, P(u32), u32, vp, vp]
    lib.tsw_get_stats.argtypes = [vp, P(Stats)]
    lib.tsw_reset_stats.argtypes = [vp]
    lib.tsw_set_timing.argtypes = [vp, ctypes.c_int]
    lib.tsw_probe_round_floors.argtypes = [vp, ctypes.c_uint32, P(ctypes.c_double)]
    lib.tsw_plan_mapd_resolved.argtypes = [vp, P(_Point), u32, P(_Task), u32, u32, P(_Rec), P(u32), P(u32),
                                           _RESOLVE_FN, vp]
    lib.tsw_plan_mapd_resolved.restype = ctypes.c_int
    lib.tsw_next_hop_codes.argtypes = [vp, P(u32), P(u32), u32, P(ctypes.c_uint8)]
    lib.tsw_host_next_hop_codes.argtypes = [P(ctypes.c_uint8), u32, u32, P(u32), P(u32), u32, P(ctypes.c_uint8)]
    lib.tsw_next_hop_codes.restype = ctypes.c_int
    lib.tsw_build_id.argtypes = []
    lib.tsw_build_id.restype = ctypes.c_uint64
    for name in ("tsw_plan_mapd", "tsw_plan_mapd_trace", "tsw_step", "tsw_get_path_next", "tsw_decide", "tsw_dist_tables",
                 "tsw_dist_tables_device", "tsw_import_tables_device", "tsw_clear_tables", "tsw_next_hop_tables",
                 "tsw_next_hop_tables_device", "tsw_import_next_hops_device", "tsw_get_stats", "tsw_reset_stats",
                 "tsw_set_timing", "tsw_probe_round_floors"):
        getattr(lib, name).restype = ctypes.c_int
    _libs[path] = lib
    return lib


def build_id(diag: bool = False) -> str:
    """tsw_build_id() of the loaded library as 16 hex digits: the sha1 of the sources it was built from
    (__graft_entry__.source_hash). Profiles record it; bench.py pairs a profile only with its build."""
    return f"{load_library(DIAG_LIB_PATH if diag else LIB_PATH).tsw_build_id():016x}"


def grid_to_bytes(grid) -> tuple:
    """grid: list[str] | list[list[str]] | np.ndarray(uint8, HxW). Returns (bytes_array, w, h).

    Mirrors the reference: h = len(grid), w = len(grid[0]) (tswap.rs:46-47).
    """
    if isinstance(grid, np.ndarray):
        a = np.ascontiguousarray(grid, dtype=np.uint8)
        return a, a.shape[1], a.shape[0]
    rows = ["".join(r) if not isinstance(r, str) else r for r in grid]
    h = len(rows)
    w = len(rows[0])
    if any(len(r) != w for r in rows):
        raise TswapError(TSW_EINVAL, "ragged grid rows (the reference indexes grid[y][x] for x < len(grid[0]))")
    a = np.frombuffer("".join(rows).encode("latin-1"), dtype=np.uint8).reshape(h, w).copy()
    return a, w, h


def _u32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def host_next_hop_codes(grid, start, goal) -> np.ndarray:
    """tsw_host_next_hop_codes: the next-hop codes of get_path(start[i], goal[i]) from the host's exact
    A* (the plan dispatch's host service) — no context, no device."""
    lib = load_library(LIB_PATH)
    cells, w, h = grid_to_bytes(grid)
    st = np.ascontiguousarray(start, dtype=np.uint32)
    gl = np.ascontiguousarray(goal, dtype=np.uint32)
    if st.shape != gl.shape:
        raise TswapError(TSW_EINVAL, "start and goal must have the same length")
    out = np.zeros(st.size, dtype=np.uint8)
    rc = lib.tsw_host_next_hop_codes(cells.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), w, h, _u32p(st), _u32p(gl),
                                     st.size, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc != TSW_OK:
        raise TswapError(rc, "tsw_host_next_hop_codes: bad grid, or a start / goal that is not a free cell")
    return out


def _st_astar_call(call, what, start, goal, start_time, node_res, edge_res, max_time, max_nodes):
    """The argument handling tsw_astar_reserved and tsw_host_astar_reserved share: call(*args) -> rc. A size
    query first, then the call with a path array of that size — the searches run TWICE; when the paths' upper
    bound (every query arriving at max_time, sum of max_time + 1 - start_time) is at most 2^24 entries the bound is
    the first call's capacity and one call does."""
    st = np.ascontiguousarray(start, dtype=np.uint32).reshape(-1)
    gl = np.ascontiguousarray(goal, dtype=np.uint32).reshape(-1)
    t0 = np.ascontiguousarray(start_time, dtype=np.uint32).reshape(-1)
    if t0.size == 1 and st.size != 1:
        t0 = np.full(st.size, t0[0], dtype=np.uint32)
    if not (st.size == gl.size == t0.size):
        raise TswapError(TSW_EINVAL, "start, goal and start_time must have the same length")
    nr = np.zeros((0, 2), np.uint32) if node_res is None else np.ascontiguousarray(node_res, dtype=np.uint32).reshape(-1, 2)
    er = np.zeros((0, 3), np.uint32) if edge_res is None else np.ascontiguousarray(edge_res, dtype=np.uint32).reshape(-1, 3)
    k = st.size
    off = np.zeros(k + 1, dtype=np.uint32)
    status = np.zeros(k, dtype=np.uint32)
    pops = np.zeros(k, dtype=np.uint32)
    total = ctypes.c_uint32(0)
    bound = int(np.maximum(np.int64(max_time) + 1 - t0.astype(np.int64), 0).sum())
    cap = bound if bound <= (1 << 24) else 0
    for _ in range(2):
        path = np.zeros(cap, dtype=np.uint32)
        rc = call(_u32p(st), _u32p(gl), _u32p(t0), k, _u32p(nr) if nr.size else None, nr.shape[0],
                  _u32p(er) if er.size else None, er.shape[0], int(max_time), int(max_nodes), _u32p(off),
                  _u32p(path) if cap else None, cap, _u32p(status), _u32p(pops), ctypes.byref(total))
        if rc != TSW_EOVERFLOW or total.value <= cap:
            break
        cap = total.value
    if rc != TSW_OK:
        raise TswapError(rc, what())
    return off, path[:total.value].copy(), status, pops


def host_astar_reserved(grid, start, goal, start_time, node_res=None, edge_res=None, max_time: int = 1 << 20,
                        max_nodes: int = 65536):
    """tsw_host_astar_reserved: astar_with_reservation (a_star.rs:32-112) for k queries on the calling thread
    — no context, no device. Arguments and results as Planner.astar_reserved."""
    lib = load_library(LIB_PATH)
    cells, w, h = grid_to_bytes(grid)
    cp = cells.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    return _st_astar_call(lambda *a: lib.tsw_host_astar_reserved(cp, w, h, *a),
                          lambda: "tsw_host_astar_reserved: bad grid, cell, time or cap",
                          start, goal, start_time, node_res, edge_res, max_time, max_nodes)


class Planner:
    """One device context (tsw_ctx) bound to a grid."""

    def __init__(self, grid, device: int = 0, flags: int = 0, table_budget_bytes: int = 0, watchdog_ms: int = 0,
                 diag: bool = False, host_astar: int = 0):
        """flags: TSW_F_*; watchdog_ms: tsw_opts.watchdog_ms (0 = 10 s); host_astar: tsw_opts.host_astar
        (0 = default, TSW_HOST_ASTAR_OFF = no host A* service, else host threads); diag: bind the diagnostic
        build (reads the TSW_* environment knobs at creation) instead of the production library."""
        self._lib = load_library(DIAG_LIB_PATH if diag else LIB_PATH)
        cells, w, h = grid_to_bytes(grid)
        self.w, self.h = int(w), int(h)
        opts = _Opts(device, flags, table_budget_bytes, watchdog_ms, host_astar)
        ptr = self._lib.tsw_create(cells.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), w, h,
                                   ctypes.byref(opts))
        if not ptr:
            raise TswapError(TSW_EHIP, self._lib.tsw_last_error(None).decode())
        self._ctx = ptr

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.tsw_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != TSW_OK:
            raise TswapError(rc, self._lib.tsw_last_error(self._ctx).decode())

    # --- tswap_mapd -------------------------------------------------------
    def plan_mapd_arrays(self, starts_xy: np.ndarray, tasks_xyxy: np.ndarray, max_t: int = 2000,
                         trace_goals: bool = False):
        """starts_xy: (n,2) uint32; tasks_xyxy: (m,4) uint32 (pickup x,y, delivery x,y).

        Returns (rec (n, T) uint64 packed x | y<<16 | state<<32, goals (n, T) or None).
        """
        starts = np.ascontiguousarray(starts_xy, dtype=np.uint32).reshape(-1, 2)
        tasks = np.ascontiguousarray(tasks_xyxy, dtype=np.uint32).reshape(-1, 4)
        n, m = starts.shape[0], tasks.shape[0]
        stride = max_t + 1
        out = np.zeros((max(n, 1), stride), dtype=np.uint64)
        T = ctypes.c_uint32(0)
        sp = starts.ctypes.data_as(ctypes.POINTER(_Point))
        tp = tasks.ctypes.data_as(ctypes.POINTER(_Task))
        op = out.ctypes.data_as(ctypes.POINTER(_Rec))
        goals = None
        if trace_goals:
            goals = np.zeros((max(n, 1), stride), dtype=np.uint32)
            rc = self._lib.tsw_plan_mapd_trace(self._ctx, sp, n, tp, m, max_t, op, _u32p(goals), ctypes.byref(T))
        else:
            rc = self._lib.tsw_plan_mapd(self._ctx, sp, n, tp, m, max_t, op, ctypes.byref(T))
        self._check(rc)
        t = T.value
        rec = out[:n, :t] & np.uint64(0xFFFFFFFFFF)
        return rec, (goals[:n, :t] if goals is not None else None)

    def plan_mapd_online(self, starts_xy: np.ndarray, tasks_xyxy: np.ndarray, release, max_t: int = 2000,
                         trace_goals: bool = False):
        """tsw_plan_mapd_online: as plan_mapd_arrays, with task k visible from iteration release[k] on
        (release: (m,) uint32; None: every task at 0). The run goes on while tasks are still to come, so
        it ends when every task is used and every agent idle, or at max_t. Returns what plan_mapd_arrays
        returns."""
        starts = np.ascontiguousarray(starts_xy, dtype=np.uint32).reshape(-1, 2)
        tasks = np.ascontiguousarray(tasks_xyxy, dtype=np.uint32).reshape(-1, 4)
        n, m = starts.shape[0], tasks.shape[0]
        rel = None
        if release is not None:
            rel = np.ascontiguousarray(release, dtype=np.uint32).reshape(-1)
            if rel.size != m:
                raise TswapError(TSW_EINVAL, "release must hold one time per task")
        stride = max_t + 1
        out = np.zeros((max(n, 1), stride), dtype=np.uint64)
        goals = np.zeros((max(n, 1), stride), dtype=np.uint32) if trace_goals else None
        T = ctypes.c_uint32(0)
        self._check(self._lib.tsw_plan_mapd_online(
            self._ctx, starts.ctypes.data_as(ctypes.POINTER(_Point)), n, tasks.ctypes.data_as(ctypes.POINTER(_Task)),
            _u32p(rel) if rel is not None else None, m, max_t, out.ctypes.data_as(ctypes.POINTER(_Rec)),
            _u32p(goals) if goals is not None else None, ctypes.byref(T)))
        t = T.value
        rec = out[:n, :t] & np.uint64(0xFFFFFFFFFF)
        return rec, (goals[:n, :t] if goals is not None else None)

    def plan_mapd_resolved(self, starts_xy: np.ndarray, tasks_xyxy: np.ndarray, max_t: int, resolve,
                           trace_goals: bool = False):
        """tsw_plan_mapd_resolved: as plan_mapd_arrays, with every K3 batch answered by
        resolve(start u32[k], goal u32[k]) -> u8[k] codes (e.g. sharding.ShardedK3.resolve)."""
        starts = np.ascontiguousarray(starts_xy, dtype=np.uint32).reshape(-1, 2)
        tasks = np.ascontiguousarray(tasks_xyxy, dtype=np.uint32).reshape(-1, 4)
        n, m = starts.shape[0], tasks.shape[0]
        stride = max_t + 1
        out = np.zeros((max(n, 1), stride), dtype=np.uint64)
        goals = np.zeros((max(n, 1), stride), dtype=np.uint32) if trace_goals else None
        T = ctypes.c_uint32(0)
        failure = []

        def cb(user, k, sp, gp, cp):
            try:
                st = np.ctypeslib.as_array(sp, shape=(k,)).copy()
                gl = np.ctypeslib.as_array(gp, shape=(k,)).copy()
                codes = np.ascontiguousarray(resolve(st, gl), dtype=np.uint8)
                if codes.shape != (k,):
                    raise ValueError(f"resolver returned {codes.shape}, expected ({k},)")
                ctypes.memmove(cp, codes.ctypes.data, k)
                return 0
            except BaseException as e:  # noqa: BLE001 — re-raised after the call returns
                failure.append(e)
                return 1

        fn = _RESOLVE_FN(cb)
        rc = self._lib.tsw_plan_mapd_resolved(
            self._ctx, starts.ctypes.data_as(ctypes.POINTER(_Point)), n,
            tasks.ctypes.data_as(ctypes.POINTER(_Task)), m, max_t, out.ctypes.data_as(ctypes.POINTER(_Rec)),
            _u32p(goals) if goals is not None else None, ctypes.byref(T), fn, None)
        if failure:
            raise failure[0]
        self._check(rc)
        t = T.value
        rec = out[:n, :t] & np.uint64(0xFFFFFFFFFF)
        return rec, (goals[:n, :t] if goals is not None else None)

    def next_hop_codes(self, start, goal) -> np.ndarray:
        """tsw_next_hop_codes: u8 next-hop code of get_path(start[i], goal[i]) (0..3 S,E,N,W, 4 stay),
        from this context's table store (K1 / exact A* for what it does not hold yet)."""
        st = np.ascontiguousarray(start, dtype=np.uint32)
        gl = np.ascontiguousarray(goal, dtype=np.uint32)
        if st.shape != gl.shape:
            raise TswapError(TSW_EINVAL, "start and goal must have the same length")
        out = np.zeros(st.size, dtype=np.uint8)
        if st.size:
            self._check(self._lib.tsw_next_hop_codes(self._ctx, _u32p(st), _u32p(gl), st.size,
                                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def tswap_mapd(self, initial_positions: Sequence, tasks: Iterable, max_t: int = 2000):
        starts = np.array([[p[0], p[1]] for p in initial_positions], dtype=np.uint32).reshape(-1, 2)
        tl = []
        for t in tasks:
            pu, dl = (t.pickup, t.delivery) if isinstance(t, Task) else (t[0], t[1])
            tl.append([pu[0], pu[1], dl[0], dl[1]])
        tarr = np.array(tl, dtype=np.uint32).reshape(-1, 4)
        rec, _ = self.plan_mapd_arrays(starts, tarr, max_t)
        x = (rec & np.uint64(0xFFFF)).astype(np.int64)
        y = ((rec >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
        s = ((rec >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64)
        return [[((int(x[i, t]), int(y[i, t])), AgentState(int(s[i, t]))) for t in range(rec.shape[1])]
                for i in range(rec.shape[0])]

    # --- tswap_step (per tick, bin/centralized/manager.rs:101-144) ---------
    def step(self, v: np.ndarray, g: np.ndarray):
        v = np.ascontiguousarray(v, dtype=np.uint32).copy()
        g = np.ascontiguousarray(g, dtype=np.uint32).copy()
        if v.shape != g.shape:
            raise TswapError(TSW_EINVAL, "v and g must have the same length")
        self._check(self._lib.tsw_step(self._ctx, _u32p(v), _u32p(g), v.size))
        return v, g

    # --- decentralized decision (bin/decentralized/agent.rs:329-462) ----------
    def decide(self, my_v, my_g, nearby):
        """Batched compute_next_move_with_tswap. my_v, my_g: (n,) cell ids; nearby: list of n
        sequences of (cell, goal_cell) pairs (the agent's get_nearby list, self excluded, in
        order). Returns a list of (act, cell, partner, participants) with act one of
        TSW_ACT_MOVE / _GOAL_SWAP / _ROTATION / _WAIT and list indices for partner/participants."""
        my_v = np.ascontiguousarray(my_v, dtype=np.uint32)
        my_g = np.ascontiguousarray(my_g, dtype=np.uint32)
        n = my_v.size
        if my_g.size != n or len(nearby) != n:
            raise TswapError(TSW_EINVAL, "my_v, my_g and nearby must have the same length")
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(x) for x in nearby]) if n else []
        flat = [p for x in nearby for p in x]
        nv = np.array([p[0] for p in flat], dtype=np.uint32)
        ng = np.array([p[1] for p in flat], dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint32)
        cell = np.zeros(n, dtype=np.uint32)
        partner = np.zeros(n, dtype=np.uint32)
        npart = np.zeros(n, dtype=np.uint32)
        part = np.zeros(int(off[-1]) + n + 1, dtype=np.uint32)
        self._check(self._lib.tsw_decide(self._ctx, _u32p(my_v), _u32p(my_g), n, _u32p(off), _u32p(nv),
                                         _u32p(ng), _u32p(act), _u32p(cell), _u32p(partner), _u32p(npart),
                                         _u32p(part)))
        out = []
        for i in range(n):
            b = int(off[i]) + i
            out.append((int(act[i]), int(cell[i]), int(partner[i]), [int(x) for x in part[b:b + npart[i]]]))
        return out

    # --- decentralized mode for a whole fleet (tsw_nearby / tsw_decide_fleet) ---
    def nearby(self, v, radius: int = 15):
        """NearbyAgents::get_nearby (agent.rs:108-153) for every agent at once, on the device.
        v: (n,) cell ids. Returns (nb_off (n+1,), nb_idx): agent i's list is the agent indices
        nb_idx[nb_off[i]:nb_off[i+1]], every j != i within Manhattan `radius`, ascending."""
        v = np.ascontiguousarray(v, dtype=np.uint32)
        n = v.size
        off = np.zeros(n + 1, dtype=np.uint32)
        total = ctypes.c_uint32(0)
        rc = self._lib.tsw_nearby(self._ctx, _u32p(v), n, radius, _u32p(off), None, 0, ctypes.byref(total))  # size query
        if rc != TSW_EOVERFLOW or total.value == 0:
            self._check(rc)
            return off, np.zeros(0, dtype=np.uint32)
        idx = np.zeros(total.value, dtype=np.uint32)
        self._check(self._lib.tsw_nearby(self._ctx, _u32p(v), n, radius, _u32p(off), _u32p(idx), idx.size,
                                         ctypes.byref(total)))
        return off, idx

    def decide_fleet(self, v, g, radius: int = 15, part_cap: Optional[int] = None):
        """One decentralized tick for the fleet (tsw_decide_fleet): every agent's nearby list and its
        compute_next_move_with_tswap decision, on the device. v, g: (n,) cell / goal cell ids.
        Returns numpy arrays (act, cell, partner, part_off, part): act[i] one of TSW_ACT_*, cell[i] the
        Move destination, partner[i] the goal-swap partner's AGENT index (0xFFFFFFFF otherwise), and
        agent i's rotation participants as agent indices part[part_off[i]:part_off[i+1]]."""
        v = np.ascontiguousarray(v, dtype=np.uint32)
        g = np.ascontiguousarray(g, dtype=np.uint32)
        n = v.size
        if g.size != n:
            raise TswapError(TSW_EINVAL, "v and g must have the same length")
        act, cell, partner = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        off = np.zeros(n + 1, dtype=np.uint32)
        cap = 4 * n + 64 if part_cap is None else int(part_cap)
        for attempt in range(2):
            part = np.zeros(cap, dtype=np.uint32)
            rc = self._lib.tsw_decide_fleet(self._ctx, _u32p(v), _u32p(g), n, radius, _u32p(act), _u32p(cell),
                                            _u32p(partner), _u32p(off), _u32p(part), cap)
            # TSW_EOVERFLOW with part_off[n] > cap: part was too small, and part_off[n] is what it takes
            if rc != TSW_EOVERFLOW or attempt or part_cap is not None or int(off[n]) <= cap:
                break
            cap = int(off[n])
        self._check(rc)
        return act, cell, partner, off, part[:int(off[n])]

    def fleet_apply(self, v, g, act, cell, partner, part_off, part):
        """One tick's decisions (decide_fleet's outputs, or the caller's own in that form) applied in the
        lock-step model of include/tswap.h: Moves, goal swaps and rotations with the reference handlers'
        sequential semantics, agents taking their turns in ascending index. Works on copies, like step.
        Returns (v, g) after the tick."""
        v = np.ascontiguousarray(v, dtype=np.uint32).copy()
        g = np.ascontiguousarray(g, dtype=np.uint32).copy()
        act, cell, partner, part_off, part = (np.ascontiguousarray(a, dtype=np.uint32)
                                              for a in (act, cell, partner, part_off, part))
        n = v.size
        if g.size != n or act.size != n or cell.size != n or partner.size != n or part_off.size != n + 1:
            raise TswapError(TSW_EINVAL, "v, g, act, cell, partner need n entries and part_off n + 1")
        if n and part.size < int(part_off.max()):
            raise TswapError(TSW_EINVAL, "part is shorter than part_off says")
        self._check(self._lib.tsw_fleet_apply(self._ctx, _u32p(v), _u32p(g), n, _u32p(act), _u32p(cell),
                                              _u32p(partner), _u32p(part_off), _u32p(part) if part.size else None))
        return v, g

    def fleet_run(self, v, g, ticks: int, radius: int = 15, record: bool = False):
        """Up to `ticks` lock-step ticks (lists, decisions, application) with v and g resident on the
        device (tsw_fleet_run); stops early at a fixed point. Returns (v, g, ticks_done), with
        record=True also (v_rec, g_rec) of shape (n, ticks_done + 1): column t is the state after t ticks."""
        v = np.ascontiguousarray(v, dtype=np.uint32).copy()
        g = np.ascontiguousarray(g, dtype=np.uint32).copy()
        n = v.size
        if g.size != n:
            raise TswapError(TSW_EINVAL, "v and g must have the same length")
        ticks = int(ticks)
        done = ctypes.c_uint32(0)
        vr = gr = None
        if record:
            vr = np.zeros((n, ticks + 1), dtype=np.uint32)
            gr = np.zeros((n, ticks + 1), dtype=np.uint32)
        self._check(self._lib.tsw_fleet_run(self._ctx, _u32p(v), _u32p(g), n, radius, ticks,
                                            _u32p(vr) if record else None, _u32p(gr) if record else None,
                                            ctypes.byref(done)))
        if record:
            return v, g, done.value, vr[:, :done.value + 1].copy(), gr[:, :done.value + 1].copy()
        return v, g, done.value

    def fleet_mapd(self, starts_xy, tasks_xyxy, max_t: int = 2000, radius: int = 15, trace: bool = False):
        """A MAPD run on the lock-step decentralized tick, resident on the device (tsw_fleet_mapd): an agent
        without a task takes the next one of the stream, pickup and delivery are keyed on v == g, every
        step is one tick. starts_xy: (n,2) uint32; tasks_xyxy: (m,4) uint32 (pickup x,y, delivery x,y).
        Returns (rec, stalled), with trace=True (rec, goals, tasks, stalled): rec (n, T) uint64 packed
        x | y<<16 | state<<32 exactly as plan_mapd_arrays packs it, goals / tasks (n, T) uint32 the goal cell
        and the task index (0xFFFFFFFF: none) of every agent after each step, stalled True when the run
        ended at a fixed point with tasks still open."""
        starts = np.ascontiguousarray(starts_xy, dtype=np.uint32).reshape(-1, 2)
        tasks = np.ascontiguousarray(tasks_xyxy, dtype=np.uint32).reshape(-1, 4)
        n, m = starts.shape[0], tasks.shape[0]
        max_t = int(max_t)
        stride = max_t + 1 if 0 <= max_t <= 1 << 20 else 1  # past the limit the call fails before it writes
        out = np.zeros((max(n, 1), stride), dtype=np.uint64)
        goals = np.zeros((max(n, 1), stride), dtype=np.uint32) if trace else None
        tks = np.zeros((max(n, 1), stride), dtype=np.uint32) if trace else None
        T, stalled = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self._lib.tsw_fleet_mapd(
            self._ctx, starts.ctypes.data_as(ctypes.POINTER(_Point)), n, tasks.ctypes.data_as(ctypes.POINTER(_Task)),
            m, radius, max_t, out.ctypes.data_as(ctypes.POINTER(_Rec)), _u32p(goals) if trace else None,
            _u32p(tks) if trace else None, ctypes.byref(T), ctypes.byref(stalled)))
        t = T.value
        rec = out[:n, :t] & np.uint64(0xFFFFFFFFFF)
        if trace:
            return rec, goals[:n, :t].copy(), tks[:n, :t].copy(), bool(stalled.value)
        return rec, bool(stalled.value)

    # --- audit ------------------------------------------------------------
    def _audit(self, call, n, T, col, agents):
        sm = Audit()
        cw = np.zeros((T, TSW_AUDIT_NCOL), dtype=np.uint32) if col else None
        aw = np.zeros((n, TSW_AUDIT_NAGENT), dtype=np.uint32) if agents else None
        if aw is not None:
            aw[:, 3] = 0xFFFFFFFF  # what an agent without a violation reports (the call writes nothing for n * T == 0)
        self._check(call(ctypes.byref(sm), _u32p(cw) if col else None, _u32p(aw) if agents else None))
        out = sm.as_dict()
        if col:
            out["col"] = cw
        if agents:
            out["agents"] = aw
        return out

    def audit(self, rec, col: bool = False, agents: bool = False) -> dict:
        """tsw_audit_records: conflicts, legality and deliveries of plan records, counted on the device.
        rec: the packed (n, T) uint64 array plan_mapd_arrays and fleet_mapd return (x | y<<16 | state<<32;
        higher bits are ignored). Returns the summary (tsw_audit's fields: state_steps, bad_state, moves,
        deliveries, colocations, swaps, jumps, off_map, moving_columns, first_t / first_agent per
        AUDIT_KINDS), plus "col" (T, 11) uint32 with col=True and "agents" (n, 4) uint32 with agents=True
        (the columns as include/tswap.h lists them)."""
        rec = np.ascontiguousarray(rec, dtype=np.uint64)
        if rec.ndim != 2:
            raise TswapError(TSW_EINVAL, "rec must be an (n, T) array")
        n, T = rec.shape
        rp = rec.ctypes.data_as(ctypes.POINTER(_Rec))
        return self._audit(lambda s, c, a: self._lib.tsw_audit_records(self._ctx, rp, n, T, T, s, c, a), n, T, col, agents)

    def audit_device(self, ptr: int, n: int, T: int, stride: int, col: bool = False, agents: bool = False) -> dict:
        """tsw_audit_records_device: as audit, the records in device memory on the context's device (e.g. a
        torch int64 tensor's data_ptr), agent i's column t at ptr + 8 * (i * stride + t)."""
        return self._audit(lambda s, c, a: self._lib.tsw_audit_records_device(self._ctx, ptr, n, T, stride, s, c, a),
                           int(n), int(T), col, agents)

    # --- task timeline ------------------------------------------------------
    def _timeline(self, call, starts_xy, tasks_xyxy, release, rule):
        if rule not in TIMELINE_RULES:
            raise TswapError(TSW_EINVAL, f"rule must be one of {sorted(TIMELINE_RULES)}")
        tasks = np.ascontiguousarray(tasks_xyxy, dtype=np.uint32).reshape(-1, 4)
        m = tasks.shape[0]
        starts = None if starts_xy is None else np.ascontiguousarray(starts_xy, dtype=np.uint32).reshape(-1, 2)
        rel = None
        if release is not None:
            rel = np.ascontiguousarray(release, dtype=np.uint32).reshape(-1)
            if rel.size != m:
                raise TswapError(TSW_EINVAL, "release must hold one time per task")
        sm = Timeline()
        tw = np.full((m, TSW_TL_NTASK), 0xFFFFFFFF, dtype=np.uint32)
        self._check(call(starts.ctypes.data_as(ctypes.POINTER(_Point)) if starts is not None and starts.size else None,
                         tasks.ctypes.data_as(ctypes.POINTER(_Task)) if m else None,
                         _u32p(rel) if rel is not None else None, m, TIMELINE_RULES[rule], ctypes.byref(sm),
                         _u32p(tw) if m else None))
        out = sm.as_dict()
        out["task"] = tw
        return out

    def task_timeline(self, rec, starts_xy, tasks_xyxy, release=None, rule: str = "nearest") -> dict:
        """tsw_task_timeline: which agent took each task and when it was assigned, picked up and delivered,
        replayed on the device from plan records alone. rec: the packed (n, T) uint64 array plan_mapd_arrays,
        plan_mapd_online and fleet_mapd return, or any prefix of its columns; starts_xy, tasks_xyxy, release:
        what that plan call was given. rule: "nearest" for the centralized plans, "stream" for fleet_mapd
        (release must be None; starts_xy may be). Returns tsw_timeline's fields (wait_sum, service_sum,
        carry_sum, assigned, carried, delivered, unreleased, service_min, service_max, makespan, consistent,
        bad_kind, bad_t, bad_agent) plus "task", an (m, 4) uint32 array of agent, t_assign, t_carry, t_deliver
        (0xFFFFFFFF: did not happen)."""
        rec = np.ascontiguousarray(rec, dtype=np.uint64)
        if rec.ndim != 2:
            raise TswapError(TSW_EINVAL, "rec must be an (n, T) array")
        n, T = rec.shape
        if starts_xy is not None and np.asarray(starts_xy).size != 2 * n:
            raise TswapError(TSW_EINVAL, "starts_xy must hold one point per row of rec")
        rp = rec.ctypes.data_as(ctypes.POINTER(_Rec))
        return self._timeline(lambda *a: self._lib.tsw_task_timeline(self._ctx, rp, n, T, T, *a),
                              starts_xy, tasks_xyxy, release, rule)

    def task_timeline_device(self, ptr: int, n: int, T: int, stride: int, starts_xy, tasks_xyxy, release=None,
                             rule: str = "nearest") -> dict:
        """tsw_task_timeline_device: as task_timeline, the records in device memory on the context's device
        (e.g. a torch int64 tensor's data_ptr), agent i's column t at ptr + 8 * (i * stride + t)."""
        if starts_xy is not None and np.asarray(starts_xy).size != 2 * int(n):
            raise TswapError(TSW_EINVAL, "starts_xy must hold one point per agent")
        return self._timeline(lambda *a: self._lib.tsw_task_timeline_device(self._ctx, ptr, int(n), int(T), int(stride), *a),
                              starts_xy, tasks_xyxy, release, rule)

    def timeline_probe(self) -> dict:
        """tsw_probe_timeline: the last timeline call's kernel times per pass (ms) and its replay counters."""
        out = (ctypes.c_double * 5)()
        self._check(self._lib.tsw_probe_timeline(self._ctx, out))
        return {"events_ms": out[0], "replay_ms": out[1], "attach_ms": out[2], "takes": int(out[3]),
                "candidates_scanned": int(out[4])}

    # --- space-time A* with reservations -------------------------------------
    def astar_reserved(self, start, goal, start_time, node_res=None, edge_res=None, max_time: int = 1 << 20,
                       max_nodes: int = 65536):
        """tsw_astar_reserved: astar_with_reservation (a_star.rs:32-112) for k queries on the device. start,
        goal: (k,) free cell ids; start_time: (k,) or one time for all; node_res: (n, 2) uint32 rows (cell, t);
        edge_res: (n, 3) uint32 rows (from, to, t); max_time: a popped node with f > max_time ends a search;
        max_nodes: pushes a search may make. Returns (path_off (k + 1,), path, status (k,) of TSW_SP_*, pops (k,)):
        query i's path is path[path_off[i]:path_off[i + 1]], the cell at time start_time[i] + j at index j, empty
        unless status[i] == TSW_SP_FOUND. Cost: when sum(max_time + 1 - start_time) over the queries exceeds 2^24 (large
        k with a generous max_time, the default 2^20 among them) the wrapper asks for the paths' size first and the
        searches run twice; give the tightest max_time you can. The context keeps the call's scratch (see
        include/tswap.h: 1.5 MiB per search wave in flight at the default max_nodes, 12 GiB for 8,192 queries or
        more) until it is closed; a smaller max_nodes shrinks it."""
        return _st_astar_call(lambda *a: self._lib.tsw_astar_reserved(self._ctx, *a),
                              lambda: self._lib.tsw_last_error(self._ctx).decode(),
                              start, goal, start_time, node_res, edge_res, max_time, max_nodes)

    def st_astar_probe(self) -> dict:
        """tsw_probe_st_astar: the last astar_reserved call's kernel times (ms), batches and resident waves."""
        out = (ctypes.c_double * 5)()
        self._check(self._lib.tsw_probe_st_astar(self._ctx, out))
        return {"reservations_ms": out[0], "search_ms": out[1], "pack_ms": out[2], "batches": int(out[3]),
                "waves": int(out[4])}

    # --- get_path -----------------------------------------------------------
    def get_path_next(self, start: np.ndarray, goal: np.ndarray):
        s = np.ascontiguousarray(start, dtype=np.uint32)
        g = np.ascontiguousarray(goal, dtype=np.uint32)
        nxt = np.zeros(s.size, dtype=np.uint32)
        ln = np.zeros(s.size, dtype=np.int32)
        self._check(self._lib.tsw_get_path_next(self._ctx, _u32p(s), _u32p(g), s.size, _u32p(nxt),
                                                ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return nxt, ln

    # --- K1 tables ----------------------------------------------------------
    def dist_tables(self, goals) -> np.ndarray:
        g = np.ascontiguousarray(goals, dtype=np.uint32)
        out = np.zeros((g.size, self.h * self.w), dtype=np.uint16)
        self._check(self._lib.tsw_dist_tables(self._ctx, _u32p(g), g.size,
                                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))))
        return out

    def dist_tables_device(self, goals, dev_ptr: int):
        g = np.ascontiguousarray(goals, dtype=np.uint32)
        self._check(self._lib.tsw_dist_tables_device(self._ctx, _u32p(g), g.size, ctypes.c_void_p(dev_ptr)))

    def import_tables_device(self, goals, dev_ptr: int):
        g = np.ascontiguousarray(goals, dtype=np.uint32)
        self._check(self._lib.tsw_import_tables_device(self._ctx, _u32p(g), g.size, ctypes.c_void_p(dev_ptr)))

    def next_hop_tables(self, goals) -> np.ndarray:
        g = np.ascontiguousarray(goals, dtype=np.uint32)
        out = np.zeros((g.size, self.h * self.w), dtype=np.uint8)
        self._check(self._lib.tsw_next_hop_tables(self._ctx, _u32p(g), g.size,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def next_hop_tables_device(self, goals, dev_ptr: int, dist_ptr: int = 0):
        """Resolved next-hop codes of `goals` (eager A*) into device memory (len(goals) x w*h u8);
        dist_ptr (optional): their K1 distance tables too (len(goals) x w*h u16)."""
        g = np.ascontiguousarray(goals, dtype=np.uint32)
        self._check(self._lib.tsw_next_hop_tables_device(self._ctx, _u32p(g), g.size, ctypes.c_void_p(dev_ptr),
                                                         ctypes.c_void_p(dist_ptr or None)))

    def import_next_hops_device(self, goals, dist_ptr: int, nh_ptr: int):
        """Ingest tables + next-hop codes from device memory (e.g. an all-gather of rank shards)."""
        g = np.ascontiguousarray(goals, dtype=np.uint32)
        self._check(self._lib.tsw_import_next_hops_device(self._ctx, _u32p(g), g.size, ctypes.c_void_p(dist_ptr),
                                                          ctypes.c_void_p(nh_ptr)))

    def clear_tables(self):
        self._check(self._lib.tsw_clear_tables(self._ctx))

    def stats(self) -> dict:
        s = Stats()
        self._check(self._lib.tsw_get_stats(self._ctx, ctypes.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._check(self._lib.tsw_reset_stats(self._ctx))

    def probe_round_floors(self, block: int = 0) -> tuple:
        """(us per wave-0 rules firing chain, us per block-wide pass) of the plan kernel's round
        shapes on a `block`-thread workgroup (0 = the last plan's): its latency floors (bench.py)."""
        out = (ctypes.c_double * 2)()
        self._check(self._lib.tsw_probe_round_floors(self._ctx, block, out))
        return float(out[0]), float(out[1])

    def set_timing(self, on: bool):
        self._check(self._lib.tsw_set_timing(self._ctx, 1 if on else 0))


def tswap_mapd(grid, initial_positions, tasks, max_t: int = 2000):
    """Drop-in for `pub fn tswap_mapd` (src/algorithm/tswap.rs:39-43)."""
    with Planner(grid) as p:
        return p.tswap_mapd(initial_positions, tasks, max_t)


def tswap_step(grid, agents_v, agents_g):
    """One `tswap_step` over cell ids (y*w+x) on a throw-away context (tests, one-off calls).

    For the centralized manager's per-tick use (plan_all_paths, bin/centralized/manager.rs:101-144)
    keep ONE `Planner` for the grid and call `Planner.step` every tick: its goal tables and resolved
    next hops persist across ticks (LRU-bounded by table_budget_bytes), where this function rebuilds
    the context — grid upload, BFS tables, A* scratch — on every call."""
    with Planner(grid) as p:
        return p.step(np.asarray(agents_v), np.asarray(agents_g))
