"""CPU model of k_plan's K4 assignment scan (round 12) against the sequential assignment.

The kernel (tsw_plan_assign.h, sec_assign) takes a step's idle agents in index order in adaptive batches.
Per batch it bounds every agent's minimum from the chunk boxes of the Morton index (phase A), lets the
threads that own a chunk within some agent's bound append (chunk, agent mask) to an LDS list of fixed
capacity, walks the list with one lane per entry (rounds over the list when more chunks pass than fit),
merges per-agent minima of (distance, task index), accepts them in agent order up to the first agent whose
task an earlier batch agent took, removes the taken tasks, and adapts the width (doubling up to the cap
after a batch without a conflict, dropping to the accepted count after one).

This file restates that over the same index (tasks in Morton order of their pickup points, chunks of KCH
entries with a static box and a live count) and checks it against the definition it must equal
(tswap.rs:123-138): for each idle agent in index order, the first minimum of (Manhattan distance, task
index) over the tasks not yet used. The mutants at the end each break one property of the scan; the inputs
here must tell every one of them from the definition.
"""
from __future__ import annotations

import numpy as np
import pytest

KCH = 32
TAKEN = None


def morton(x, y):
    z = 0
    for b in range(16):
        z |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return z


class Index:
    """The host's K4 index (tsw_plan_host.hip plan_impl): live[pos] = pickup point or TAKEN, klt[pos] = task,
    kbox[chunk] = static bounding box, kcnt[chunk] = untaken entries; the tail chunk is padded with TAKEN."""

    def __init__(self, picks, kch=KCH):
        self.kch = kch
        m = len(picks)
        order = sorted(range(m), key=lambda k: (morton(*picks[k]), k))
        self.nch = max((m + kch - 1) // kch, 1)
        self.live = [TAKEN] * (self.nch * kch)
        self.klt = [0xFFFFFFFF] * (self.nch * kch)
        self.kpos = [0] * m
        self.kcnt = [0] * self.nch
        self.kbox = [(0, 0, 0, 0)] * self.nch
        for pos, k in enumerate(order):
            x, y = picks[k]
            ch = pos // kch
            self.live[pos], self.klt[pos], self.kpos[k] = (x, y), k, pos
            if self.kcnt[ch] == 0:
                self.kbox[ch] = (x, y, x, y)
            else:
                x0, y0, x1, y1 = self.kbox[ch]
                self.kbox[ch] = (min(x0, x), min(y0, y), max(x1, x), max(y1, y))
            self.kcnt[ch] += 1

    def take(self, k):
        pos = self.kpos[k]
        assert self.live[pos] is not TAKEN
        self.live[pos] = TAKEN
        self.kcnt[pos // self.kch] -= 1


def box_lb(p, box):
    x0, y0, x1, y1 = box
    dx = x0 - p[0] if p[0] < x0 else (p[0] - x1 if p[0] > x1 else 0)
    dy = y0 - p[1] if p[1] < y0 else (p[1] - y1 if p[1] > y1 else 0)
    return dx + dy


INF = (1 << 32) - 1


class Scan:
    """One step's assignments as the kernel computes them. `stats` counts what the tests assert ran."""

    def __init__(self, picks, width=16, cap=64, kch=KCH, *, tie_by_pos=False, no_diam=False, drop_overflow=False,
                 accept_past_conflict=False, keep_taken=False, one_per_batch=False):
        self.ix = Index(picks, kch)
        self.picks = picks
        self.unused = len(picks)
        self.width, self.cap = (1 if one_per_batch else width), cap
        self.mut = dict(tie_by_pos=tie_by_pos, no_diam=no_diam, drop_overflow=drop_overflow,
                        accept_past_conflict=accept_past_conflict, keep_taken=keep_taken)
        self.stats = dict(batches=0, rounds=0, conflicts=0, widths=[], pairs=0)

    # phase A: U_b = min over chunks with an untaken entry of lb + diam
    def bound(self, p):
        ub = INF
        for c in range(self.ix.nch):
            if self.ix.kcnt[c] == 0:
                continue
            x0, y0, x1, y1 = self.ix.kbox[c]
            diam = 0 if self.mut["no_diam"] else (x1 - x0) + (y1 - y0)
            ub = min(ub, box_lb(p, self.ix.kbox[c]) + diam)
        return ub

    def batch_minima(self, pos):
        ix, B = self.ix, len(pos)
        ub = [self.bound(p) for p in pos]
        # every chunk's owner computes the mask of batch agents whose bound the chunk's box is within
        pending = []
        for c in range(ix.nch):
            if ix.kcnt[c] == 0:
                continue
            mask = sum(1 << b for b in range(B) if box_lb(pos[b], ix.kbox[c]) <= ub[b])
            if mask:
                pending.append((c, mask))
                self.stats["pairs"] += bin(mask).count("1")
        best = [None] * B  # (distance, task index[, position for the tie mutant])
        # rounds over a list of `cap` entries; the owners' arrival order is arbitrary: walk it backwards
        pending.reverse()
        while True:
            lst, pending = pending[:self.cap], pending[self.cap:]
            self.stats["rounds"] += 1
            for c, mask in lst:
                for e in range(ix.kch):  # one lane per entry
                    p = ix.live[c * ix.kch + e]
                    if p is TAKEN:
                        continue
                    t = ix.klt[c * ix.kch + e]
                    for b in range(B):
                        if not (mask >> b) & 1:
                            continue
                        d = abs(pos[b][0] - p[0]) + abs(pos[b][1] - p[1])
                        key = (d, c * ix.kch + e, t) if self.mut["tie_by_pos"] else (d, t)
                        if best[b] is None or key < best[b]:
                            best[b] = key
            if not pending or self.mut["drop_overflow"]:
                break
        return [None if k is None else (k[0], k[-1]) for k in best]

    def step(self, idle_pos):
        """idle_pos: the idle agents' positions in agent order -> the task each gets (None: none left)."""
        out = [None] * len(idle_pos)
        kk, bcur = 0, self.width
        while kk < len(idle_pos):
            B = min(bcur, len(idle_pos) - kk)
            self.stats["batches"] += 1
            self.stats["widths"].append(B)
            best = self.batch_minima(idle_pos[kk:kk + B])
            acc, stop, took = 0, False, []
            for b in range(B):
                if self.unused - acc == 0 or best[b] is None:
                    stop = True
                    break
                t = best[b][1]
                if t in took:
                    self.stats["conflicts"] += 1
                    if not self.mut["accept_past_conflict"]:
                        break
                    took.append(None)  # the mutant leaves the agent without a task and goes on
                    acc += 1
                    continue
                took.append(t)
                acc += 1
            for b, t in enumerate(took):
                if t is None:
                    continue
                out[kk + b] = t
                self.unused -= 1
                if not self.mut["keep_taken"]:
                    self.ix.take(t)
            if stop:
                break
            kk += acc
            bcur = min(self.width, 2 * bcur) if acc == B else max(acc, 1)
        return out


def sequential(picks, used, idle_pos):
    """tswap.rs:123-138: each idle agent in index order takes min_by_key's first minimum over unused tasks."""
    out = []
    for p in idle_pos:
        cand = [(abs(p[0] - q[0]) + abs(p[1] - q[1]), k) for k, q in enumerate(picks) if k not in used]
        if not cand:
            out.append(None)
            continue
        t = min(cand)[1]
        used.add(t)
        out.append(t)
    return out


def run_steps(picks, steps, **kw):
    """Several steps' idle sets through the model and the definition: (model, sequential, stats)."""
    sc, used = Scan(picks, **kw), set()
    got, want = [], []
    for idle in steps:
        got.append(sc.step(idle))
        want.append(sequential(picks, used, idle))
    return got, want, sc.stats


def _random_case(rng, w, h, m, n, steps):
    picks = [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(m)]
    return picks, [[(int(rng.integers(w)), int(rng.integers(h))) for _ in range(int(rng.integers(0, n + 1)))]
                   for _ in range(steps)]


def case_tie_across_chunks():
    """Two pickup cells at equal distance from the agent, in different chunks, the lower task index in the
    later chunk of the Morton order; chunks filled up with far tasks."""
    # agent at (0, 0): (20, 0) and (0, 20) are both 20 away, Morton codes 272 and 544; the 40 far cells of
    # (24..31, 8..12) lie between them in the Morton order
    fill = [(24 + k % 8, 8 + k // 8) for k in range(40)]
    picks = [(0, 20)] + fill + [(20, 0)]  # task 0 at the Morton-later cell, task 41 at the earlier one
    ix = Index(picks)
    assert ix.kpos[41] == 0 and ix.kpos[0] == 41 and ix.kpos[0] // KCH != ix.kpos[41] // KCH
    return picks, [[(0, 0)]]


def case_same_cell(m=100):
    """>= 3 chunks of tasks at one cell: every chunk ties for every agent."""
    return [(5, 5)] * m, [[(0, 0), (9, 9), (5, 5)], [(1, 1)] * 20]


def case_ring():
    """More idle agents than the batch width around three pickups: conflicts in every batch."""
    picks = [(10, 10), (11, 10), (10, 11)] * 6 + [(30, 30)] * 40
    ring = [(10 + dx, 10 + dy) for dx in range(-3, 4) for dy in range(-3, 4) if abs(dx) + abs(dy) == 3]
    return picks, [ring * 2]


def case_diam():
    """A wide chunk whose box is near the agent but whose only live entry is far, beside a compact chunk
    a little farther: without the diameter the bound cuts the chunk that holds the true minimum."""
    wide = [(0, 0)] + [(31, k) for k in range(31)]  # box (0,0)-(31,30)
    picks = wide + [(20, 40 + k % 2) for k in range(32)]
    st = [[(2, 36)]]  # inside neither box; nearest live entry decides after (0, 0)'s neighbours are gone
    return picks, st


CASES = {
    "tie": case_tie_across_chunks,
    "same-cell": case_same_cell,
    "ring": case_ring,
    "diam": case_diam,
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("width,cap", [(16, 64), (16, 2), (8, 64), (1, 1), (32, 3)])
def test_adversarial_cases_match_sequential(name, width, cap):
    picks, steps = CASES[name]()
    got, want, _ = run_steps(picks, steps, width=width, cap=cap)
    assert got == want


@pytest.mark.parametrize("seed", range(12))
def test_random_steps_match_sequential(seed):
    rng = np.random.default_rng(seed)
    m = int(rng.choice([0, 1, 32, 33, 65, 200, 700]))
    picks, steps = _random_case(rng, 48, 48, m, 40, 6)
    for width, cap, kch in ((16, 64, 32), (16, 3, 32), (4, 2, 8), (32, 64, 16)):
        got, want, _ = run_steps(picks, steps, width=width, cap=cap, kch=kch)
        assert got == want, (seed, width, cap, kch)


def test_more_idle_agents_than_tasks():
    picks = [(3, 3), (8, 1), (2, 9)]
    got, want, st = run_steps(picks, [[(k, k) for k in range(10)], [(1, 1)]], width=16, cap=64)
    assert got == want and got[0][3:] == [None] * 7 and got[1] == [None]


def test_list_overflow_takes_rounds_and_small_list_fits_one():
    picks, steps = case_same_cell(200)  # 7 chunks, all tied
    _, _, st = run_steps(picks, steps, width=16, cap=2)
    assert st["rounds"] > st["batches"]
    _, _, st = run_steps(picks, steps, width=16, cap=64)
    assert st["rounds"] == st["batches"]


def test_width_drops_after_a_conflict_and_regrows():
    picks, steps = case_ring()
    got, want, st = run_steps(picks, steps, width=16, cap=64)
    assert got == want and st["conflicts"] > 0
    w = st["widths"]
    assert w[0] == 16 and min(w) < 16
    assert any(b > a for a, b in zip(w, w[1:])), w  # doubles again after a clean batch
    _, _, st1 = run_steps(picks, steps, width=16, cap=64, one_per_batch=True)
    assert set(st1["widths"]) == {1} and st1["conflicts"] == 0


MUTANTS = ["tie_by_pos", "no_diam", "drop_overflow", "accept_past_conflict", "keep_taken"]


def _all_inputs():
    for name in sorted(CASES):
        yield name, CASES[name](), dict(width=16, cap=2)
    rng = np.random.default_rng(99)
    yield "random", _random_case(rng, 48, 48, 300, 40, 6), dict(width=16, cap=2)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_inputs_kill_mutant(mutant):
    """Each broken scan differs from the definition on at least one input of this file (and the unbroken one on
    none: the tests above)."""
    killed = []
    for name, (picks, steps), kw in _all_inputs():
        try:
            got, want, _ = run_steps(picks, steps, **kw, **{mutant: True})
        except AssertionError:  # the model's own consistency check (a task taken twice)
            killed.append(name)
            continue
        if got != want:
            killed.append(name)
    assert killed, f"mutant {mutant} survives every input"
