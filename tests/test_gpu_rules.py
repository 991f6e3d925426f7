"""GPU: k_plan's rules phase (SEC_RULES, tsw_plan_kernel.h) on the built states of rules_cases.py, one Planner.step
per state (the chained cascade: K of them), bit-exact against OracleGraph.step, and its counters against the counting
restatement of the sequential phase: each path of the phase is reached on purpose and a counter says so.

Contexts. The product library with TSW_F_EAGER_NEXTHOP, TSW_F_LAZY_NEXTHOP and TSW_F_LAZY_NEXTHOP | TSW_F_EXIT_MODE runs
every case. The diagnostic library (TSW_PLAN_DEBUG=1, lazy next hops, so that the block join is reachable) runs:

  ag         no other knob: k_plan<true, true, true, false>, every case — the counters of the batch, the wave rotation and the
             parallel settle are asserted here
  global     TSW_AGENTS_LDS=0 TSW_PART_LDS=0x7F: k_plan<false, true, true, false>, every case — no batch (AG only), rule 4 in
             fire() with the members in S.F2, the serial settle, single fast firings from registers for every swap and
             2-cycle (the l == 63 mask: cascade-64/65/130, pairs-32/512 split)
  pg         TSW_AGENTS_LDS=0 TSW_PART_LDS=0x3F on the one 208x208 map of rules_cases.pg_rows(): k_plan<false, false, false,
             true>; the rings around the 64-member edge, pairs-33, mixed and cascade-65 — PG has the wave rotation and the
             parallel settle without the batch
  ab1/8/9    TSW_AB_FLAGS: 1 sends 2-cycles to the wave rotation, 8 keeps walking firings out of batches. Cases with
             2-cycles or walks: the pairs, mixed, the close and field cases, the convoys (ab8)
  walkcap4   TSW_WALK_CAP=4: the cascades (no firing of theirs walks: unchanged), the convoys (every walk too long), mixed
  block64 / block1024
             TSW_PLAN_BLOCK: cases whose block-wide passes depend on the block size (n above and below it, a join)
  wrm0       TSW_WAVE_RULES_MAX=0, the block-rounds form no product context reaches: rings, cascades, pairs-33, mixed

The placements themselves are pinned on the CPU by tests/host/place_main.cpp.

Lines of plan_debug_report (tsw_plan_host.hip) that _diag() reads:
  "[k_plan] planner LDS: agents %u part 0x%x flinks %u occ %u mu %u tasks %u (%zu B)"
  "[k_plan] wave rules kcycles: load ... | loads %llu fast firings %llu | rotations %llu, settle kcycles: ..."
  "[k_plan] wave rules batches %llu (longest walks %llu hops) kcycles: ..."
"""
import os
import re

import numpy as np
import pytest

import rules_cases as rc
from p2p_distributed_tswap_amd import TSW_F_EAGER_NEXTHOP, TSW_F_EXIT_MODE, TSW_F_LAZY_NEXTHOP, Planner

pytestmark = pytest.mark.gpu

WATCHDOG_MS = 2000
LAZY = TSW_F_LAZY_NEXTHOP

# name -> (flags, environment of the diagnostic library or None for the product library)
CONTEXTS = {
    "eager": (TSW_F_EAGER_NEXTHOP, None),
    "lazy": (LAZY, None),
    "lazy-exit": (LAZY | TSW_F_EXIT_MODE, None),
    "ag": (LAZY, {}),
    "global": (LAZY, {"TSW_AGENTS_LDS": "0", "TSW_PART_LDS": str(0x7F)}),
    "pg": (LAZY, {"TSW_AGENTS_LDS": "0", "TSW_PART_LDS": str(0x3F)}),
    "ab1": (LAZY, {"TSW_AB_FLAGS": "1"}),
    "ab8": (LAZY, {"TSW_AB_FLAGS": "8"}),
    "ab9": (LAZY, {"TSW_AB_FLAGS": "9"}),
    "walkcap4": (LAZY, {"TSW_WALK_CAP": "4"}),
    "block64": (LAZY, {"TSW_PLAN_BLOCK": "64"}),
    "block1024": (LAZY, {"TSW_PLAN_BLOCK": "1024"}),
    "wrm0": (LAZY, {"TSW_WAVE_RULES_MAX": "0"}),
}
PLACEMENT = {"global": "agents 0 part 0x7f flinks 1 occ 1 mu 1", "pg": "agents 0 part 0x3f flinks 1 occ 0 mu 0"}

WALKERS = rc.PAIR_NAMES + ["mixed"] + rc.CLOSE_NAMES + rc.FIELD_NAMES  # 2-cycles, or firings that walk
SELECTED = {
    "eager": rc.NAMES, "lazy": rc.NAMES, "lazy-exit": rc.NAMES, "ag": rc.NAMES, "global": rc.NAMES,
    "pg": rc.PG_CASES,
    "ab1": WALKERS, "ab8": WALKERS + rc.CONVOY_NAMES, "ab9": WALKERS,
    "walkcap4": rc.CASCADE_NAMES + rc.CONVOY_NAMES + ["mixed"],
    "block64": ["ring-64-d3-spread", "ring-128-d3-id", "pairs-513-split", "cascade-130-inc", "mixed", "field-cascade-70",
                "close-0"],
    "block1024": ["ring-64-d3-spread", "ring-128-d3-id", "pairs-513-split", "cascade-130-inc", "mixed", "field-cascade-70",
                  "close-0"],
    "wrm0": rc.RING_NAMES + rc.CASCADE_NAMES + ["pairs-33-adj", "pairs-33-split", "mixed"],
}


def _params():
    out = []
    for ctx, names in SELECTED.items():
        order = {}
        for nm in names:  # cases on one map next to each other: one planner serves them
            order.setdefault(rc.case(nm).rows if ctx != "pg" else (), []).append(nm)
        out += [pytest.param(ctx, nm, id=f"{ctx}-{nm}") for group in order.values() for nm in group]
    return out


# ---- one planner per (context, map), kept while consecutive tests use it ------------------------------------------
_live = {}


def _planner(ctx, rows):
    key = (ctx, rows)
    if _live.get("key") != key:
        _close()
        flags, env = CONTEXTS[ctx]
        saved = {}
        if env is not None:  # the diagnostic library reads its knobs once, when the context is created
            env = dict(env, TSW_PLAN_DEBUG="1")
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
        try:
            _live["planner"] = Planner(list(rows), flags=flags, watchdog_ms=WATCHDOG_MS, diag=env is not None)
        finally:
            for k, val in saved.items():
                if val is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = val
        _live["key"] = key
    return _live["planner"]


def _close():
    p = _live.pop("planner", None)
    _live.pop("key", None)
    if p is not None:
        p.close()


@pytest.fixture(scope="module", autouse=True)
def _planners():
    yield
    _close()


_RE_LDS = re.compile(r"\[k_plan\] planner LDS: (agents \d+ part 0x[0-9a-f]+ flinks \d+ occ \d+ mu \d+) tasks")
_RE_WAVE = re.compile(r"\[k_plan\] wave rules kcycles: .*\| loads (\d+) fast firings (\d+) \| rotations (\d+), settle")
_RE_BATCH = re.compile(r"\[k_plan\] wave rules batches (\d+) \(longest walks (\d+) hops\)")


def _diag(err):
    """Counters since the reset_stats before the case (the ticks accumulate over a context's calls): the last report."""
    lds, w, b = _RE_LDS.findall(err), _RE_WAVE.findall(err), _RE_BATCH.findall(err)
    assert lds and w and b, "no k_plan report in the diagnostic output"
    loads, fast, rot = (int(x) for x in w[-1])
    return dict(lds=lds[-1], loads=loads, fast=fast, rotations=rot, batches=int(b[-1][0]), walk_hops=int(b[-1][1]))


def _run(ctx, name, capfd):
    c = rc.embedded(name) if ctx == "pg" else rc.case(name)
    e = rc.expected(c)
    diag = CONTEXTS[ctx][1] is not None
    p = _planner(ctx, c.rows)
    p.reset_stats()
    capfd.readouterr()
    v, g = c.v, c.g
    for _ in range(c.calls):
        v, g = p.step(v, g)
    st = p.stats()
    d = _diag(capfd.readouterr().err) if diag else None
    r = dict(rule_rounds=st["rule_rounds"], inc=st["relabels_inc"], full=st["relabels_full"], fires=st["watchdog_fires"],
             exits=sum(st["plan_exits"]), diag=d)
    bad = np.flatnonzero((v != e["v"]) | (g != e["g"]))
    assert bad.size == 0, (f"{ctx} {name}: {bad.size} agents differ from the oracle, first {bad[0]}: v {v[bad[0]]} g {g[bad[0]]}, "
                           f"oracle v {e['v'][bad[0]]} g {e['g'][bad[0]]}")
    assert r["fires"] == 0
    return c, e["counters"], r


def _ring_shape(name):
    if name == "rings2":
        return 132, 4
    return int(name.split("-")[1]), int(name.split("-")[2][1:])


@pytest.mark.parametrize("ctx,name", _params())
def test_rules_case(ctx, name, capfd):
    c, C, r = _run(ctx, name, capfd)
    d = r["diag"]
    wave = ctx != "wrm0"
    # Firing count: every firing path counts exactly once — fire() adds 1 to rule_rounds, a batch its nb, a single fast
    # firing 1 (rr), the wave rotation 1; a chained run sums over its calls.
    assert r["rule_rounds"] == C.n, f"{r['rule_rounds']} rule rounds, the sequential phase fires {C.n} times"

    # Relabels. Every call's phase begins with one rules_init (relabel_full). On a corridor K2 resolves every code,
    # so no firing of the ring, cascade, convoy and corridor-pairs cases misses and nothing else relabels fully:
    corridor = name in rc.RING_NAMES + rc.CASCADE_NAMES + rc.CONVOY_NAMES + rc.PAIR_NAMES + ["mixed"]
    if name in rc.RING_NAMES:
        L, d_rot = _ring_shape(name)
        if wave or L <= 64:
            # wave rounds: a rotation settles inside wave 0 (rot_settle: the parallel form for (AG || PG) && L <= 64,
            # relabel_reset + relabel_walks otherwise), one relabel_inc each. Block rounds: fire() sets s_miss, the
            # join relabels incrementally while the changed list (the L members) has <= 64 entries
            assert (r["inc"], r["full"]) == (d_rot, 1), r
        else:
            # block rounds, L > 64: the join's `s_cnt <= 64u` fails and every rotation costs a rules_init
            assert (r["inc"], r["full"]) == (0, 1 + d_rot), r
    elif corridor:
        # swaps and 2-cycles never relabel; mixed's 4-cycle and, with TSW_AB_FLAGS bit 1, every 2-cycle (wave rotation
        # and settle, AG / PG; fire() and the serial settle otherwise) relabel incrementally, once each
        rot = C.rotations if (ctx in ("ab1", "ab9") or not wave) else C.rotations - C.rotations2
        if wave:
            assert (r["inc"], r["full"]) == (rot, c.calls), r
        else:  # block rounds: fire() handles a 2-cycle as a rotation, s_miss, join; 2 or 4 changed agents: incremental
            assert (r["inc"], r["full"]) == (C.rotations, c.calls), r
    if name in ("field-cascade-20", "field-cascade-70"):
        # Unresolved codes. Exit mode has no worker: the first firing whose new code is NH_UNKNOWN misses, refresh_codes
        # queues it, `!coop_resolve` leaves the kernel (exit_need_queries), and the relaunch re-enters SEC_RULES through
        # rules_init — one more full relabel per exit taken inside the phase, whatever K is. In coop mode the workers
        # race the firings, so how many of them miss is a matter of timing (measured: 9 of 20, 21 to 34 of 70), and a
        # join never relabels fully here: `if (tid == 0) s_cnt = 0` after every join keeps the changed list at the
        # firings since the last one, far below the `s_cnt <= 64u` of the incremental relabel, for K = 70 as for 20.
        # The join's full form is reached deterministically by the block rounds' rings with L > 64 above.
        if ctx == "lazy-exit":
            assert r["exits"] >= 1 and 1 < r["full"] <= 1 + r["exits"] and r["inc"] == 0, r
        elif ctx == "eager":
            assert (r["inc"], r["full"], r["exits"]) == (0, 1, 0), r  # nothing is unresolved
    if name in rc.FIELD_NAMES and ctx not in ("lazy-exit", "eager"):
        # Coop mode, what holds whatever the workers' timing: a relabel past the phase's rules_init follows a firing
        # (a miss's join, or a rotation's settle or join), at most one each; and a join relabels fully only with more
        # than 64 entries in the changed list, two a firing since the last join (`s_cnt = 0` there): never for the 20
        # firings of field-cascade-20 or the 8 of field-pairs, at most twice in field-cascade-70's 70
        assert r["exits"] == 0 and r["inc"] + r["full"] - 1 <= C.n, r
        assert r["full"] <= 1 + C.n // 33, r

    if d is None:
        return
    if ctx in PLACEMENT:
        assert d["lds"] == PLACEMENT[ctx], d
    else:
        assert d["lds"].startswith("agents 1 part 0x0 flinks 0 occ 1 mu 1"), d
    assert d["rotations"] == C.rotations, d
    if not wave:
        assert d["loads"] == 0 and d["fast"] == 0 and d["batches"] == 0, d  # no wave-0 round ran
        return
    assert d["loads"] > 0, d
    if ctx in ("global", "pg"):
        assert d["batches"] == 0 and d["fast"] == 0, d  # the batch is AG only ("fast firings" counts batched firings)
        return
    # the default placement (AG). "fast firings" is TK_WR_FAST_FIRINGS: firings applied by a batch
    two_cycles = 0 if ctx in ("ab1", "ab9") else C.rotations2
    if name in rc.PAIR_NAMES:
        if ctx in ("ab8", "ab9"):
            # a 2-cycle's firing always walks (p_walk), and without batched walks lane l never enters the batch code
            assert d["fast"] == 0 and d["batches"] == 0, d
        else:
            assert d["fast"] == two_cycles, d  # ab1: no 2-cycle precomputation, every pair takes the wave rotation
            # adj: lane 2p + 1 carries lane 2p's mark, one firing a batch. split: a chunk's firing lanes are first
            # members only (their partners lie 64 or more lanes on, or behind every firing lane of the chunk): one
            # batch a chunk of 64 pairs
            P = C.rotations2
            assert d["batches"] == (0 if not two_cycles else P if name.endswith("adj") else (P + 63) // 64), d
    elif name == "mixed" and ctx in ("ag", "walkcap4", "block64", "block1024"):
        # Agents 0-8: pair, cascade, pair, cascade, pair, cascade; 9-12 the 4-cycle; 13-21 three more pairs and cascade
        # agents. A batch ends before a pair's second member and before a cascade's next agent (both carry an earlier
        # lane's mark and reload), and before the 4-cycle's first member (a firing lane without a precomputation):
        # {0}, {2, 3}, {5, 6}, {8}, then the wave rotation of 9-12 and a rescan from 10, {13}, {15, 16}, {18, 19}.
        # Agent 21 ends with its own cell as goal. Seven batches apply the 6 two-cycles and 5 swaps
        assert d["fast"] == C.swaps + C.rotations2 == 11 and d["batches"] == 7, d
    elif name in rc.CASCADE_NAMES:
        # every firing is a rule-3 swap with a resolved code whose s gets a resting successor (no walk): batched,
        # one firing a batch (lane l + 1 carries lane l's mark)
        assert d["fast"] == C.swaps and d["batches"] == C.swaps, d
    elif name == "close-ring" and ctx in ("ag", "ab1"):
        # lane 1's walk meets lane 0's marks on agents 0 and 3: the first batch is lane 0 alone (`cw < lane` cuts lane 1,
        # whose own `c` is clean, and lane 2 would cut only after it); reloaded, lane 1's walk closes the ring, its
        # batch comes out empty and it fires from registers, labelling the new cycle
        assert d["fast"] == 1 and d["batches"] == 2, d
    elif name in rc.CONVOY_NAMES:
        K = int(name.split("-")[1])
        cap = 4 if ctx == "walkcap4" else rc.WALK_CAP
        if ctx == "ab8":
            assert d["fast"] == 0 and d["batches"] == 0, d
        else:
            # the walk passes K agents and needs one more iteration to see the chain's end: it fits when K < walk_cap;
            # a walk that runs long empties the batch and lane l fires alone from registers
            assert d["batches"] == 1 and d["fast"] == (1 if K < cap else 0), d
            assert d["walk_hops"] == min(K, cap), d


def test_every_path_has_a_case():
    """The table of DESIGN.md ("Rules phase: what tests reach which path"), as selections of this file."""
    ids = {p.id for p in _params()}
    for want in ("ag-pairs-512-split", "ag-pairs-513-split", "global-cascade-64-inc", "global-pairs-512-split",
                 "ag-ring-64-d3-id", "pg-ring-64-d3-perm", "ag-ring-66-d1-id", "global-ring-64-d1-id", "pg-ring-66-d3-perm",
                 "lazy-field-cascade-20", "lazy-field-cascade-70", "lazy-exit-field-pairs", "wrm0-ring-128-d3-id",
                 "ag-convoy-16", "ag-close-0", "ag-mixed", "ag-ring-64-d3-spread"):
        assert want in ids, want
