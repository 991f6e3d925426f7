"""CPU model of the planner's cached, budgeted step-start walk-ahead (tsw_plan_walk.h nextnext_prefetch /
walk_prefetch, round 10).

Per agent the kernel keeps a frontier entry (PlanArgs::wf: the cell the agent stood on at the walk, its goal,
the cell the walk stopped at, that cell's hop index past the agent's next cell). A step's walk resumes at the
entry — the hop index drops by one when the agent moved exactly one hop along the cached path, any other
change is a miss — reads at most `walk_step` new hops and stops at the first unresolved code, which it queues
together with the DAG past it. A walk that reaches the pickup goes on along the delivery leg for what is left
of the step's budget; that part is not cached.

Three forms that round 10 built, measured and took out of the kernel again (its register allocation, or no
gain: DESIGN.md) stay in the model as options, under the same invariants, so that a later attempt starts from
a checked restatement: `dlv_cache` (the hop index runs on past the pickup and the delivery-leg frontier is
cached in the entry), `memo` (the DAG past a stop cell is queued once per (stop cell, goal)) and `follow`
(entries keyed by the goal, so that a goal's new holder resumes the previous holder's walk).

This file restates that in plain Python over small random grids whose next hops come from BFS trees, with
agents that move one hop, stay, miss a step's walk, switch from their pickup to their delivery, get new tasks
and exchange goals with another agent (and sometimes back) as the rules do, and with codes that become
resolved at random times. Checked:

 1. after every walk the entry's stop cell is exactly `hop` resolved hops from the agent's next cell toward
    its goal (on past the pickup toward the delivery goal under WF_DLV, whose pickup hop index is right);
 2. every pair queued is a free cell paired with the agent's goal or delivery goal at that step;
 3. the DAG past every unresolved stop cell is queued (now or earlier);
 4. against the plain walk (no cache, no budget, no memo) in the same world, where codes resolve at random
    times whatever is queued: every pair the budgeted walk queues the plain walk queued at that step or
    earlier — the budget only delays. Where codes resolve only after the walker itself queued them, goals
    change only at pickups and deliveries, and the run lasts until every agent rests, both walks queue the
    same set of pairs, only later — but for pairs that another agent's own step needed (and the planner
    then waited for) between the plain walk's read and the slower frontier's.

Mutants that must fail: no decrement on a move; a resume without the on-path check; and, for the `memo`
option, a DAG memo that is not cleared when the stop cell changes."""
from __future__ import annotations

import collections

import numpy as np
import pytest

GOAL, DAG = 1, 2


def _grid(w, h, p_block, rng):
    free = rng.random((h, w)) >= p_block
    free[0, :] = True  # a connected spine
    free[:, 0] = True
    return free


class World:
    """Free cells reachable from the spine, and for every goal the BFS distance and next cell of every cell."""

    def __init__(self, free):
        self.h, self.w = free.shape
        w = self.w
        seen = {0}
        q = collections.deque([0])
        while q:
            c = q.popleft()
            for n in self._nb(c, free):
                if n not in seen:
                    seen.add(n)
                    q.append(n)
        self.cells = sorted(seen)
        self.free = seen
        self.dist, self.nxt = {}, {}
        for g in self.cells:
            d = {g: 0}
            q = collections.deque([g])
            while q:
                c = q.popleft()
                for n in self._nb(c, free):
                    if n in seen and n not in d:
                        d[n] = d[c] + 1
                        q.append(n)
            self.dist[g] = d
            self.nxt[g] = {c: next(n for n in self._nb(c, free) if n in d and d[n] == d[c] - 1) for c in d if c != g}

    def _nb(self, c, free):
        y, x = divmod(c, self.w)
        for dy, dx in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            ny, nx = y + dy, x + dx
            if 0 <= ny < self.h and 0 <= nx < self.w and free[ny, nx]:
                yield ny * self.w + nx

    def dag(self, u, g, levels=1):
        """Cells of the shortest-path DAG toward g within `levels` of u (u excluded, g excluded)."""
        out, fr = [], [u]
        for _ in range(levels):
            nx = []
            for x in fr:
                y0, x0 = divmod(x, self.w)
                for dy, dx in ((1, 0), (0, 1), (-1, 0), (0, -1)):
                    c = (y0 + dy) * self.w + x0 + dx
                    if 0 <= y0 + dy < self.h and 0 <= x0 + dx < self.w and c in self.free and c != g \
                            and self.dist[g].get(c, -1) == self.dist[g][x] - 1 and c not in nx:
                        nx.append(c)
            out += nx
            fr = nx
        return out


class Agent:
    def __init__(self, v, g, dg):
        self.v, self.g, self.dg = v, g, dg  # dg: delivery goal while heading to the pickup, else None


class Walker:
    """nextnext_prefetch for one agent per call. own=False: codes resolve at world times (shared with any
    other walker); own=True: a code resolves `delay` steps after this walker queued it. Either way the pair
    an agent stands on is resolved when the step begins (the planner waits for it)."""

    def __init__(self, world, n, depth, step, cache=True, dag=True, own=False, seed=0, mutant=None, follow=False,
                 dlv_cache=False, memo=False):
        self.W, self.depth, self.step, self.cache, self.use_dag, self.own = world, depth, step, cache, dag, own
        self.seed, self.mutant, self.follow, self.dlv_cache, self.memo = seed, mutant, follow, dlv_cache, memo
        self.entry = {}  # by goal (follow) or by agent
        self.resumed_after_handover = 0
        self.forced = set()
        self.queued = {}  # pair -> step first queued
        self.t = 0
        self.allowed = ()

    def _h(self, c, g):
        return (c * 7919 + g * 104729 + self.seed * 31) % 1000

    def resolved(self, c, g):
        if (c, g) in self.forced:
            return True
        if self.own:
            return (c, g) in self.queued and self.queued[(c, g)] + 1 + self._h(c, g) % 4 <= self.t
        return self._h(c, g) % 40 <= self.t

    def queue(self, c, g):
        assert c in self.W.free and g in self.allowed, "a pair off the grid or toward a foreign goal"
        self.queued.setdefault((c, g), self.t)

    def dag_prefetch(self, u, g):
        for c in self.W.dag(u, g):
            if not self.resolved(c, g):
                self.queue(c, g)

    def walk(self, u, g, h, hlim, dagdone):
        fl = 0
        while h < hlim:
            if u == g:
                fl = GOAL
                break
            if not self.resolved(u, g):
                self.queue(u, g)
                if self.use_dag:
                    if not dagdone:
                        self.dag_prefetch(u, g)
                    fl = DAG
                break
            u = self.W.nxt[g][u]
            h += 1
            if self.mutant != "memo_sticky":
                dagdone = False
        return u, h, fl

    def step_agent(self, k, a, t):
        """The kernel's loop body for an agent whose own code is resolved and that is not at its goal."""
        self.t = t
        v, g = a.v, a.g
        leg_ok = a.dg is not None and a.dg != g
        self.allowed = (g, a.dg) if leg_ok else (g,)
        u0, h0, dlv, dagf, dh = self.W.nxt[g][v], 0, False, False, 0
        key = g if self.follow else k
        f = self.entry.get(key) if self.cache else None
        if f is not None:
            on = f["goal"] == g and f["at"] == v
            if f["goal"] == g and f["at"] != v:
                on = self.mutant == "no_onpath" or (self.resolved(f["at"], g) and self.W.nxt[g].get(f["at"]) == v)
            if on and f["dlv"] and not (leg_ok and f["dgoal"] == a.dg):
                on = False
            if on:
                dec = 0 if f["at"] == v or self.mutant == "no_dec" else 1
                hp = max(f["hop"] - dec, 0)
                if hp > 0:
                    u0, h0, dlv, dagf, dh = f["stop"], hp, f["dlv"], f["dag"] and self.memo, max(f["dhop"] - dec, 0)
                    if f["agent"] != k:
                        self.resumed_after_handover += 1
        cell, hop, fl = u0, h0, (DAG if dagf else 0)
        if h0 < self.depth:
            hlim = min(self.depth, h0 + self.step) if (self.step and self.cache) else self.depth
            if not dlv:
                cell, hop, fl = self.walk(u0, g, h0, hlim, dagf)
                if (fl & GOAL) and leg_ok:
                    if self.dlv_cache:
                        dlv, dh = True, hop
                        cell, hop, fl = self.walk(g, a.dg, dh, hlim, False)
                    else:  # what is left of the step's budget, from the pickup, not remembered
                        self.walk(g, a.dg, hop, hlim, False)
            else:
                cell, hop, fl = self.walk(u0, a.dg, h0, hlim, dagf)
        if self.cache:
            self.entry[key] = dict(agent=k, at=v, goal=g, stop=cell, hop=hop, dlv=dlv, dag=bool(fl & DAG),
                                 dgoal=a.dg if dlv else None, dhop=dh if dlv else 0)
        return cell, hop, fl, dlv, dh

    def check(self, a, res):
        """Invariants 1 and 3 for the walk just made."""
        cell, hop, fl, dlv, dh = res
        cur, goal, leg = self.W.nxt[a.g][a.v], a.g, False
        for i in range(hop):
            if not leg and dlv and cur == a.g:
                assert i == dh, "the pickup's hop index"
                goal, leg = a.dg, True
            assert cur != goal and self.resolved(cur, goal), "an unresolved or goal cell inside the walked stretch"
            cur = self.W.nxt[goal][cur]
        if dlv and not leg:
            assert cur == a.g and dh == hop, "the pickup's hop index"
            goal = a.dg
        assert cur == cell, f"stop cell {cell} is not {hop} hops along (that is {cur})"
        if (fl & DAG) and not self.resolved(cell, goal):
            for c in self.W.dag(cell, goal):
                assert self.resolved(c, goal) or (c, goal) in self.queued, "the DAG past a stop cell was never queued"


def _run(seed, walkers, steps=70, exchanges=True, skips=True, tasks_per_agent=None, n=8, size=7):
    """One scripted world (the script does not depend on what any walker does), every walker stepping each
    agent; returns the walkers. tasks_per_agent: agents rest after that many tasks and the run goes on until
    all rest."""
    rng = np.random.default_rng(seed)
    world = World(_grid(size, size, 0.15, rng))
    cells = world.cells
    ws = [mk(world, n) for mk in walkers]

    def task(a):
        a.g, a.dg = (int(c) for c in rng.choice(cells, 2, replace=False))

    agents = []
    left = []
    for _ in range(n):
        a = Agent(int(rng.choice(cells)), 0, None)
        task(a)
        agents.append(a)
        left.append((tasks_per_agent or 10 ** 9) - 1)
    back = []  # goal exchanges to undo: (step, a, b)
    t = 0
    while t < steps or (tasks_per_agent and any(a.v != a.g or a.dg is not None for a in agents)):
        assert t < 2000
        for k, a in enumerate(agents):
            if a.v == a.g:
                continue
            skip = skips and rng.random() < 0.12
            for w in ws:
                w.forced.add((a.v, a.g))  # the step's refresh waits for the agent's own pair
                if not skip:
                    w.check(a, w.step_agent(k, a, t))
        for k, a in enumerate(agents):  # movement, then the state machine
            if a.v != a.g and rng.random() < 0.8:
                a.v = world.nxt[a.g][a.v]
            if a.v == a.g:
                if a.dg is not None:
                    a.g, a.dg = a.dg, None
                elif left[k] > 0:
                    left[k] -= 1
                    task(a)
        if exchanges:
            for (tb, i, j) in [b for b in back if b[0] == t]:
                agents[i].g, agents[j].g = agents[j].g, agents[i].g
            back = [b for b in back if b[0] > t]
            if rng.random() < 0.3:
                i, j = (int(x) for x in rng.choice(n, 2, replace=False))
                # as the rules do where the geometry allows: j stands on i's next cell (rule 3, 2-cycle rotation)
                near = [(a, b) for a in range(n) for b in range(n) if a != b and agents[a].v != agents[a].g
                        and world.nxt[agents[a].g][agents[a].v] == agents[b].v and agents[a].g != agents[b].g]
                if near:
                    i, j = near[int(rng.integers(len(near)))]
                agents[i].g, agents[j].g = agents[j].g, agents[i].g
                if rng.random() < 0.5:
                    back.append((t + int(rng.integers(1, 3)), i, j))
        t += 1
    return ws


def _budgeted(step, **kw):
    return lambda world, n: Walker(world, n, depth=8, step=step, **kw)


KERNEL = dict()  # the kernel's form
OPTIONS = dict(dlv_cache=True, memo=True)  # forms kept in the model only


def _plain(**kw):
    return lambda world, n: Walker(world, n, depth=8, step=0, cache=False, **kw)


@pytest.mark.parametrize("form", [KERNEL, OPTIONS, dict(follow=True, **OPTIONS)], ids=["kernel", "options", "follow"])
@pytest.mark.parametrize("step", [0, 1, 2, 4])
def test_frontier_invariants_and_budget_only_delays(step, form):
    for seed in range(12):
        b, p = _run(seed, [_budgeted(step, seed=seed, **form), _plain(seed=seed)])
        assert b.queued, "nothing queued: the script exercises nothing"
        for pair, t in b.queued.items():
            assert pair in p.queued and p.queued[pair] <= t, f"seed {seed}: {pair} queued at {t}, plain walk {p.queued.get(pair)}"


@pytest.mark.parametrize("form", [KERNEL, OPTIONS], ids=["kernel", "options"])
@pytest.mark.parametrize("step", [1, 2, 4])
def test_same_pairs_as_the_plain_walk_when_codes_wait_for_the_queue(step, form):
    for seed in range(12):
        b, p = _run(seed, [_budgeted(step, seed=seed, own=True, dag=False, **form), _plain(seed=seed, own=True, dag=False)],
                    steps=0, exchanges=False, skips=False, tasks_per_agent=3)
        assert b.forced == p.forced
        assert set(b.queued) <= set(p.queued), f"seed {seed}: {set(b.queued) - set(p.queued)}"
        assert set(p.queued) - set(b.queued) <= p.forced, f"seed {seed}: {set(p.queued) - set(b.queued) - p.forced}"
        assert all(b.queued[x] >= p.queued[x] for x in b.queued)


def test_goal_keyed_entries_resume_the_previous_holders_walk():
    resumed = {True: 0, False: 0}
    for seed in range(12):
        for follow in (True, False):
            (b,) = _run(seed, [_budgeted(2, seed=seed, follow=follow, **OPTIONS)])
            resumed[follow] += b.resumed_after_handover
    assert resumed[True] > 0 and resumed[False] == 0, resumed


@pytest.mark.parametrize("mutant", ["no_dec", "no_onpath", "memo_sticky"])
def test_mutants_fail(mutant):
    failed = 0
    for seed in range(12):
        try:
            _run(seed, [_budgeted(2, seed=seed, mutant=mutant, **(OPTIONS if mutant == "memo_sticky" else KERNEL))])
        except AssertionError:
            failed += 1
    assert failed > 0, f"mutant {mutant} passed every seed"
