"""An independent host model of the liveness check under per-process weak
fairness (include/kubecheck.h, "Liveness", fairness = 1).

The graph is live_model.Model's (the CPU oracle's successors).  The process of
an edge is derived from the two canonical tuples and the oracle's action name
alone: APIStart is the server's step; any other step is taken by the one actor
whose pc word (t[1 + 19 a]) changed.  SCCs by Tarjan's algorithm on Python
lists and sets, then F and L as the header defines them.  Nothing here runs the
product's code (csrc/liveness.h, liveness.hip).

Not a test module: tests/test_fair_host.py and tests/test_gpu_fairness.py use it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

import live_model
from live_model import PER_PROC


def edge_process(m, s, action: str, t) -> int:
    """The process that takes the step s -> t of model m (single server)."""
    A = m.nc + m.np
    if action == "APIStart":
        assert m.ns == 1
        return A
    moved = [a for a in range(A) if s[1 + PER_PROC * a] != t[1 + PER_PROC * a]]
    assert len(moved) == 1, (action, moved)          # unambiguous on every model used
    return moved[0]


def edge_process_by_pc(tuples, src, dst, A: int):
    """The process of every edge src[k] -> dst[k] from the two canonical tuples
    alone (rows of `tuples`), with no action name: the one actor whose pc word
    moved, or the single server (process A) when none did.  For graphs too
    large to build from the oracle; tests/test_live_graphs_host.py holds it
    against edge_process on every edge of the small models."""
    pcs = np.asarray(tuples)[:, [1 + PER_PROC * a for a in range(A)]]
    moved = pcs[np.asarray(src, dtype=np.int64)] != pcs[np.asarray(dst, dtype=np.int64)]
    count = moved.sum(axis=1)
    assert count.size == 0 or count.max() <= 1          # unambiguous
    return np.where(count == 1, moved.argmax(axis=1), A)


def edge_procs(m) -> List[List[int]]:
    """procs[i][k] = the process of m's k-th edge out of state i."""
    return [[edge_process(m, m.states[i], a, m.states[j]) for a, j in zip(m.actions[i], m.succ[i])]
            for i in range(len(m.states))]


def tarjan(succ: Sequence[Sequence[int]], nodes: Set[int]) -> List[List[int]]:
    """The SCCs of the subgraph `nodes` induces (self-loops are irrelevant),
    iteratively."""
    index: Dict[int, int] = {}
    low: Dict[int, int] = {}
    on: Set[int] = set()
    stack: List[int] = []
    out: List[List[int]] = []
    for root in sorted(nodes):
        if root in index:
            continue
        index[root] = low[root] = len(index)
        stack.append(root)
        on.add(root)
        work = [(root, iter(succ[root]))]
        while work:
            v, it = work[-1]
            pushed = False
            for w in it:
                if w not in nodes or w == v:
                    continue
                if w not in index:
                    index[w] = low[w] = len(index)
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(succ[w])))
                    pushed = True
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            if pushed:
                continue
            work.pop()
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                out.append(comp)
    return out


@dataclass
class FairVerdict:
    stay: Set[int]
    sccs: List[Set[int]]          # the SCCs of more than one state in S
    fair_sccs: List[Set[int]]
    fair: Set[int]                # F
    live: Set[int]                # L
    terminal: Set[int]            # the graph's terminal states
    enabled: List[int]            # per state, the mask of enabled processes
    scc_of: Dict[int, int]        # state of a fair SCC -> its position in fair_sccs
    min_level: Optional[int]

    @property
    def violated(self) -> bool:
        return bool(self.fair)

    @property
    def live_terminal(self) -> int:
        return len(self.live & self.terminal)


def fair_check(succ: Sequence[Sequence[int]], procs: Sequence[Sequence[int]], nproc: int, S: Set[int],
               level: Optional[Sequence[int]] = None) -> FairVerdict:
    """F and L of the graph (succ, procs) for the stay set S, by the definition."""
    n = len(succ)
    enabled = [0] * n
    for i in range(n):
        for j, p in zip(succ[i], procs[i]):
            if j != i:
                enabled[i] |= 1 << p
    terminal = {i for i in range(n) if enabled[i] == 0}
    full = (1 << nproc) - 1
    sccs, fair_sccs = [], []
    for comp in tarjan(succ, S):
        if len(comp) < 2:
            continue
        C = set(comp)
        sccs.append(C)
        wit = 0
        for i in C:
            wit |= ~enabled[i] & full
            for j, p in zip(succ[i], procs[i]):
                if j != i and j in C:
                    wit |= 1 << p
        if wit == full:
            fair_sccs.append(C)
    F = set().union(*fair_sccs) | (terminal & S)
    # L: backward closure of F inside S
    pred: Dict[int, List[int]] = {}
    for i in S:
        for j in succ[i]:
            if j != i and j in S:
                pred.setdefault(j, []).append(i)
    L, todo = set(F), list(F)
    while todo:
        j = todo.pop()
        for i in pred.get(j, ()):
            if i not in L:
                L.add(i)
                todo.append(i)
    scc_of = {i: k for k, C in enumerate(fair_sccs) for i in C}
    min_level = min((level[i] for i in L), default=None) if level is not None else None
    return FairVerdict(set(S), sccs, fair_sccs, F, L, terminal, enabled, scc_of, min_level)


_procs_cache: Dict[int, List[List[int]]] = {}


def check(m, prop: int) -> FairVerdict:
    """The verdict of property `prop` on live_model.Model m."""
    if id(m) not in _procs_cache:
        _procs_cache[id(m)] = edge_procs(m)
    S = {i for i, t in enumerate(m.states) if m.stay(prop, t)}
    return fair_check(m.succ, _procs_cache[id(m)], m.nc + m.np + m.ns, S, m.level)


def procs_of(m) -> List[List[int]]:
    if id(m) not in _procs_cache:
        _procs_cache[id(m)] = edge_procs(m)
    return _procs_cache[id(m)]


def check_lasso_graph(succ: Sequence[Sequence[int]], procs: Sequence[Sequence[int]], nproc: int,
                      level: Sequence[int], want: FairVerdict, idx: List[int], prefix_len: int, kind: str,
                      loop_start: int) -> None:
    """The counterexample, as state indices of the graph (succ, procs) with BFS
    levels `level`, is valid by the definition: an Init state, steps of the
    graph, a shortest prefix to L, everything from there on inside S (so inside
    L), then a terminal state, or a cycle inside one fair SCC that has, for
    every process, a step of it or a state with it disabled."""
    assert len(idx) >= prefix_len >= 1 and level[idx[0]] == 1
    for a, b in zip(idx, idx[1:]):
        assert b in succ[a] and a != b
    assert prefix_len == want.min_level
    assert all(i not in want.live for i in idx[:prefix_len - 1])
    assert all(i in want.stay and i in want.live for i in idx[prefix_len - 1:])
    last = idx[-1]
    if kind == "stuttering":
        assert loop_start == -1 and last in want.terminal and last in want.fair
        return
    assert kind == "back-to-state" and prefix_len - 1 <= loop_start < len(idx)
    cycle = idx[loop_start:]
    assert idx[loop_start] in succ[last] and idx[loop_start] != last
    k = want.scc_of[cycle[0]]
    assert all(want.scc_of.get(i) == k for i in cycle)        # one fair SCC
    wit = 0
    for a, b in zip(cycle, cycle[1:] + cycle[:1]):
        wit |= ~want.enabled[a] & ((1 << nproc) - 1)
        for j, p in zip(succ[a], procs[a]):
            if j == b:
                wit |= 1 << p
    assert wit == (1 << nproc) - 1, bin(wit)


def check_lasso(m, want: FairVerdict, idx: List[int], prefix_len: int, kind: str, loop_start: int) -> None:
    """check_lasso_graph on live_model.Model m (idx = state indices of m)."""
    check_lasso_graph(m.succ, procs_of(m), m.nc + m.np + m.ns, m.level, want, idx, prefix_len, kind, loop_start)


NONE = 0xffffffff


@dataclass
class Schedule:
    trim_rounds: int              # trim launches, the last (empty) one included
    launches: int                 # reset, push, pull and close launches
    outer_rounds: int             # reset launches that left something open
    comp: List[int]               # per state: its SCC's label (NONE outside the trimmed set)
    fair: Set[int]
    live: Set[int]


def jacobi_schedule(succ: Sequence[Sequence[int]], procs: Sequence[Sequence[int]], nproc: int,
                    S: Set[int]) -> Schedule:
    """The product's whole launch schedule (include/kubecheck.h, "Liveness";
    DESIGN.md 4.7) as synchronous rounds on numpy arrays: every launch is
    judged on the values it started with.  The trim to its fixed point; then
    per outer round a reset launch (an open state with no open successor other
    than itself becomes an SCC of its own, every other open state takes its
    index as its colour), push launches (the largest colour moves along the
    edges between open states) until one raises nothing and pull launches (a
    state whose colour is its index joins, and so does an open state with a
    successor of its colour that has joined) until one adds nothing, until a
    reset leaves nothing open; then F by the definition and close launches (a
    state with a successor that reaches F reaches F) until one adds nothing.
    Counts every launch that the product follows with a counter read."""
    n = len(succ)
    src = np.array([i for i in range(n) for _ in succ[i]], dtype=np.int64)
    dst = np.array([j for i in range(n) for j in succ[i]], dtype=np.int64)
    prc = np.array([p for i in range(n) for p in procs[i]], dtype=np.int64)
    keep = src != dst                                     # edges s -> s are dropped
    src, dst, prc = src[keep], dst[keep], prc[keep]
    idx = np.arange(n, dtype=np.int64)
    full = (1 << nproc) - 1

    def any_edge(mask):                                   # per state: has an edge selected by mask
        out = np.zeros(n, dtype=bool)
        out[src[mask]] = True
        return out

    enabled = np.zeros(n, dtype=np.int64)
    np.bitwise_or.at(enabled, src, 1 << prc)
    terminal = enabled == 0
    alive = np.zeros(n, dtype=bool)
    alive[sorted(S)] = True
    trim_rounds = 0
    while True:
        trim_rounds += 1
        die = alive & ~terminal & ~any_edge(alive[src] & alive[dst])
        if not die.any():
            break
        alive &= ~die
    comp = np.full(n, NONE, dtype=np.int64)
    color = np.zeros(n, dtype=np.int64)
    launches = outer = 0
    while True:
        launches += 1                                     # reset
        opn = alive & (comp == NONE)
        still = opn & any_edge(opn[src] & opn[dst])
        single = opn & ~still
        comp[single] = idx[single]
        color[still] = idx[still]
        if not still.any():
            break
        outer += 1
        opn = still
        while True:                                       # push
            launches += 1
            m = opn[src] & opn[dst] & (color[dst] < color[src])
            if not m.any():
                break
            new = color.copy()
            np.maximum.at(new, dst[m], color[src[m]])
            color = new
        while True:                                       # pull
            launches += 1
            opn = alive & (comp == NONE)
            join = opn & ((color == idx) | any_edge(opn[src] & alive[dst] & (comp[dst] == color[src])))
            if not join.any():
                break
            comp[join] = color[join]
    # accumulate and mark
    size = np.bincount(comp[alive], minlength=n)
    wit = np.zeros(n, dtype=np.int64)
    np.bitwise_or.at(wit, comp[alive], ~enabled[alive] & full)
    inside = alive[src] & alive[dst] & (comp[src] == comp[dst])
    np.bitwise_or.at(wit, comp[src[inside]], 1 << prc[inside])
    fair_scc = (size > 1) & (wit == full)
    F = alive & (terminal | fair_scc[np.where(alive, comp, 0)])
    reach = F.copy()
    while True:                                           # close
        launches += 1
        add = alive & ~reach & any_edge(reach[dst])
        if not add.any():
            break
        reach |= add
    return Schedule(trim_rounds, launches, outer, [int(c) for c in comp], set(np.flatnonzero(F).tolist()),
                    set(np.flatnonzero(reach).tolist()))
