"""Made graphs for the liveness graph kernels (kc_live_selftest,
csrc/live_selftest.hip): the families tests/test_gpu_live_graphs.py runs on the
device and tests/test_live_graphs_host.py checks on the host, and the two ways
of making a graph's indices a legal discovery order:

  bfs_form   renumber by a level-synchronous BFS from the Init set, dropping
             what is unreachable;
  hub_form   state 0 is the only Init state, lies outside S and has an edge to
             every other state in index order, so any index pattern among the
             states 1 .. n - 1 is a legal level 2.

A Graph is plain Python lists; nothing here runs the product's code.

Not a test module."""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

NOPARENT = (1 << 64) - 1
Edge = Tuple[int, int, int]          # (source, target, process)


@dataclass
class Graph:
    name: str
    nproc: int
    succ: List[List[int]]
    procs: List[List[int]]
    stay: List[int]
    parent: List[int]
    level: List[int]
    lasso_only: bool = False         # a lasso shape: run under fairness 1 only
    next_only: bool = False          # ... under fairness 0 only
    note: Dict[str, object] = field(default_factory=dict)   # what the case expects beyond the model

    @property
    def n(self) -> int:
        return len(self.succ)

    @property
    def S(self) -> Set[int]:
        return {i for i, s in enumerate(self.stay) if s}

    def words(self):
        """deg, edges, eproc, stay, parent, level as u64 arrays."""
        u = lambda x: np.array(x, dtype=np.uint64)
        return (u([len(o) for o in self.succ]), u([j for o in self.succ for j in o]),
                u([p for o in self.procs for p in o]), u(self.stay), u(self.parent), u(self.level))


def _lists(n: int, edges: Sequence[Edge]):
    succ: List[List[int]] = [[] for _ in range(n)]
    procs: List[List[int]] = [[] for _ in range(n)]
    for s, t, p in edges:
        succ[s].append(t)
        procs[s].append(p)
    return succ, procs


def hub_form(name: str, n: int, edges: Sequence[Edge], nproc: int, stay: Optional[Sequence[int]] = None,
             **kw) -> Graph:
    """States 1 .. n - 1 with `edges` among them (and into the hub, state 0);
    stay = the states of S, default all of 1 .. n - 1."""
    assert all(s >= 1 for s, _, _ in edges)
    succ, procs = _lists(n, edges)
    succ[0] = list(range(1, n))
    procs[0] = [0] * (n - 1)
    st = [0] * n
    for i in (range(1, n) if stay is None else stay):
        assert i >= 1
        st[i] = 1
    return Graph(name, nproc, succ, procs, st, [NOPARENT] + [0] * (n - 1), [1] + [2] * (n - 1), **kw)


def bfs_form(name: str, n: int, edges: Sequence[Edge], nproc: int, stay: Sequence[int], inits: Sequence[int],
             **kw) -> Graph:
    """Renumber by BFS from `inits` (in that order); unreachable states go."""
    succ, procs = _lists(n, edges)
    order, new, parent, level = [], {}, [], []
    for i in inits:
        new[i] = len(order)
        order.append(i)
        parent.append(NOPARENT)
        level.append(1)
    k = 0
    while k < len(order):
        for j in succ[order[k]]:
            if j not in new:
                new[j] = len(order)
                order.append(j)
                parent.append(k)
                level.append(level[k] + 1)
        k += 1
    st = set(stay)
    return Graph(name, nproc, [[new[j] for j in succ[i]] for i in order], [procs[i] for i in order],
                 [1 if i in st else 0 for i in order], parent, level, **kw)


def validate(g: Graph) -> None:
    """kc_live_selftest's input rules (include/kubecheck.h), restated."""
    n = g.n
    assert 1 <= n <= 1 << 22 and 1 <= g.nproc <= 8
    assert len(g.procs) == len(g.stay) == len(g.parent) == len(g.level) == n
    assert sum(len(o) for o in g.succ) < 1 << 31
    for i in range(n):
        assert len(g.succ[i]) == len(g.procs[i])
        assert all(0 <= j < n for j in g.succ[i]) and all(0 <= p < g.nproc for p in g.procs[i])
        assert g.stay[i] in (0, 1)
    assert g.level[0] == 1
    for i in range(n):
        assert i == 0 or g.level[i] >= g.level[i - 1]
        if g.level[i] == 1:
            assert g.parent[i] == NOPARENT
        else:
            p = g.parent[i]
            assert 0 <= p < i and g.level[p] == g.level[i] - 1 and i in g.succ[p]


# ---------------------------------------------------------------- the families

def _ring(members: Sequence[int], proc) -> List[Edge]:
    """members[k] -> members[k + 1], the last back to the first; proc(k) = the process of the k-th edge."""
    m = len(members)
    return [(members[k], members[(k + 1) % m], proc(k)) for k in range(m)]


RING_SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1000)


def rings() -> List[Graph]:
    """One cycle through all of 1 .. n, along the index order and against it:
    the largest colour and then the pull each walk the whole cycle."""
    out = []
    for n in RING_SIZES:
        body = list(range(1, n + 1))
        out.append(hub_form(f"ring-{n}-up", n + 1, _ring(body, lambda k: k % 2), 2))
        out.append(hub_form(f"ring-{n}-down", n + 1, _ring(body[::-1], lambda k: k % 2), 2))
    return out


CHAIN_LENGTHS = (1, 2, 7, 40)


def scc_chains() -> List[Graph]:
    """m SCCs of 2 .. 5 states, SCC k feeding SCC k + 1.  Descending: SCC k + 1
    has the smaller indices, so SCC k's largest member colours everything below
    and one SCC closes per outer round.  Ascending: every SCC is its own root
    in the first round.  3 processes: SCCs with even k lack process 2
    everywhere (fair: it is disabled), those with odd k have it enabled in
    every member by an edge to the hub and never take it inside (unfair)."""
    out = []
    for m in CHAIN_LENGTHS:
        sizes = [2 + k % 4 for k in range(m)]
        total = sum(sizes)
        for desc in (True, False):
            blocks, at = [], 1
            for sz in (sizes[::-1] if desc else sizes):
                blocks.append(list(range(at, at + sz)))
                at += sz
            if desc:
                blocks = blocks[::-1]            # blocks[k] = SCC k; SCC 0 has the largest indices
            edges: List[Edge] = []
            for k, b in enumerate(blocks):
                edges += _ring(b, lambda e: e % 2)
                if k % 2:
                    edges += [(i, 0, 2) for i in b]
                if k + 1 < m:
                    edges.append((b[-1], blocks[k + 1][0], 1))
            out.append(hub_form(f"chain-{m}-{'desc' if desc else 'asc'}", total + 1, edges, 3,
                                note={"outer": m if desc else 1, "sccs": m}))
    return out


def straddle() -> List[Graph]:
    """A path 1 -> 2 -> ... -> 299 with two back edges: SCCs at 62 .. 65 (across
    a wave boundary; fair, process 2 disabled) and at 254 .. 258 (across a
    block boundary; unfair, process 2 leaves from every member), every other
    state an SCC of its own, 299 terminal."""
    n = 300
    edges: List[Edge] = [(i, i + 1, 0) for i in range(1, n - 1)]
    edges += [(65, 62, 1), (258, 254, 1)]
    edges += [(i, 0, 2) for i in range(254, 259)]
    return [hub_form("straddle-64-256", n, edges, 3, note={"classes": [[62, 63, 64, 65], [254, 255, 256, 257, 258]]})]


def shared_and_cut() -> List[Graph]:
    """Two cycles through one state; a ring S keeps all but one state of; the
    induced-subgraph case of test_fair_host.test_tarjan."""
    fig8 = _ring([1, 2, 3], lambda k: 0) + _ring([3, 4, 5], lambda k: 1)
    cut = _ring([1, 2, 3, 4, 5, 6], lambda k: k % 2)
    # 1 -> 2 -> 3 -> 1 ; 3 -> 4 ; 4 -> 5 -> 4 ; 6 alone ; 7 -> 7  (test_tarjan's graph, shifted by one)
    tj = [(1, 2, 0), (2, 3, 0), (3, 1, 0), (3, 4, 1), (4, 5, 0), (5, 4, 1), (7, 7, 0)]
    return [hub_form("figure-8", 6, fig8, 2, note={"classes": [[1, 2, 3, 4, 5]]}),
            hub_form("ring-cut-by-stay", 7, cut, 2, stay=[1, 2, 3, 5, 6], note={"classes": [], "live": set()}),
            hub_form("tarjan-whole", 8, tj, 2, note={"classes": [[1, 2, 3], [4, 5]]}),
            hub_form("tarjan-induced", 8, tj, 2, stay=[1, 3, 4, 5], note={"classes": [[4, 5]]})]


def uncounted_edges() -> List[Graph]:
    out = []
    # 1 <-> 2 by process 0.  Process 1: at 1 only the edge 1 -> 1, at 2 an edge to the hub.  The self-loop
    # enables nothing, so process 1 is disabled in 1 and the SCC is fair.
    out.append(hub_form("self-loop-not-enabled", 3, [(1, 2, 0), (1, 1, 1), (2, 1, 0), (2, 0, 1)], 2,
                        note={"enabled": {1: 1, 2: 3}, "fair": {1, 2}}))
    # the same with process 1 enabled in 1 too (an edge to the hub): its only step "inside" is 1 -> 1,
    # which is no witness, so the SCC is not fair
    out.append(hub_form("self-loop-no-witness", 3, [(1, 2, 0), (1, 1, 1), (1, 0, 1), (2, 1, 0), (2, 0, 1)], 2,
                        note={"enabled": {1: 3, 2: 3}, "fair": set()}))
    # 1 -> 2 (only 2 -> 2) and 1 -> 3 (no edge): both terminal, F = {2, 3}, L = {1, 2, 3}
    out.append(hub_form("terminal-kinds", 4, [(1, 2, 0), (1, 3, 1), (2, 2, 1)], 2,
                        note={"terminal": {2, 3}, "fair": {2, 3}, "live": {1, 2, 3}}))
    # 1 -> 2 twice, by processes 0 and 1; 2 -> 1 by process 2; every process enabled in both states
    par = [(1, 2, 0), (1, 2, 1), (1, 0, 2), (2, 1, 2), (2, 0, 0), (2, 0, 1)]
    out.append(hub_form("parallel-edges", 3, par, 3, note={"enabled": {1: 7, 2: 7}, "fair": {1, 2}}))
    return out


def process_counts() -> List[Graph]:
    """P = 1, 5, 8, three rings each: A takes every process inside; B takes
    process 0 only, the others are enabled in all members but one (fair through
    "disabled somewhere" alone); C takes all but the last process inside, which
    is enabled in every member (it lacks exactly one witness; P > 1 only)."""
    out = []
    for P in (1, 5, 8):
        edges: List[Edge] = []
        A = list(range(1, P + 2))
        edges += _ring(A, lambda k: k % P)
        B = list(range(A[-1] + 1, A[-1] + 4))
        edges += _ring(B, lambda k: 0)
        edges += [(i, 0, p) for i in B[1:] for p in range(1, P)]
        classes, fair = [A, B], set(A) | set(B)
        n = B[-1] + 1
        if P > 1:
            C = list(range(B[-1] + 1, B[-1] + 1 + P))
            edges += _ring(C, lambda k: k % (P - 1))
            edges += [(i, 0, P - 1) for i in C]
            edges += [(i, 0, p) for i in C for p in range(P - 1)]     # and nothing is disabled anywhere
            classes.append(C)
            n = C[-1] + 1
        out.append(hub_form(f"processes-{P}", n, edges, P, note={"classes": classes, "fair": fair}))
    return out


def empty_and_full() -> List[Graph]:
    ring = _ring([1, 2, 3], lambda k: k % 2)
    unfair = _ring([1, 2, 3], lambda k: 0) + _ring([4, 5], lambda k: 0) + [(i, 0, 1) for i in range(1, 6)]
    return [hub_form("stay-empty", 4, ring, 2, stay=[], note={"live": set()}),
            bfs_form("one-state-stay", 1, [], 1, [0], [0], note={"live": {0}, "terminal": {0}}),
            bfs_form("one-state-out", 1, [], 1, [], [0], note={"live": set()}),
            bfs_form("all-terminal", 5, [(1, 1, 0), (3, 3, 1)], 2, range(5), range(5),
                     note={"live": set(range(5)), "terminal": set(range(5))}),
            # S is every state but the hub and no SCC is fair: nothing is live, though WF_vars(Next) keeps all
            hub_form("all-stay-none-fair", 6, unfair, 2, note={"fair": set(), "classes": [[1, 2, 3], [4, 5]]})]


def lasso_shapes() -> List[Graph]:
    out = []
    # a ring of 40 by process 0, every process enabled everywhere (edges to the hub); process p > 0 steps
    # inside at 10 p only (a chord 10 p -> 10 p + 2): P - 1 witness legs and the way back
    P, R = 4, 40
    body = list(range(1, R + 1))
    e = _ring(body, lambda k: 0) + [(i, 0, p) for i in body for p in range(1, P)]
    e += [(10 * p, 10 * p + 2, p) for p in range(1, P)]
    out.append(hub_form("lasso-far-witnesses", R + 1, e, P, lasso_only=True, note={"kind": 1, "through": [(10 * p, 10 * p + 2) for p in range(1, P)]}))
    # 1 -> 2 -> 3 -> 4 -> 1, the last edge the only step of process 1 (enabled everywhere): 1 is the first L
    # state and in F already, and the witness step of process 1 lands on it
    e = [(1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 1, 1)] + [(i, 0, 1) for i in (1, 2, 3)]
    out.append(hub_form("lasso-witness-closes", 5, e, 2, lasso_only=True,
                        note={"kind": 1, "path": [0, 1, 2, 3, 4], "loop": 1}))
    # 1 -> 2 (0), 2 -> 3 (1), 3 -> 1 (0), process 1 enabled everywhere: after the two witness steps the
    # lasso stands on 3, whose direct successor is the cycle's first state
    e = [(1, 2, 0), (2, 3, 1), (3, 1, 0), (1, 0, 1), (3, 0, 1)]
    out.append(hub_form("lasso-return-direct", 4, e, 2, lasso_only=True,
                        note={"kind": 1, "path": [0, 1, 2, 3], "loop": 1}))
    # the first L state reaches a terminal state and a fair SCC in one step: the smaller index wins
    e = [(1, 2, 0), (1, 3, 1), (3, 4, 0), (4, 3, 1)]
    out.append(hub_form("lasso-tie-terminal-first", 5, e, 2, lasso_only=True,
                        note={"kind": 2, "path": [0, 1, 2]}))
    e = [(1, 4, 0), (1, 2, 1), (2, 3, 0), (3, 2, 1)]
    out.append(hub_form("lasso-tie-scc-first", 5, e, 2, lasso_only=True, note={"kind": 1, "loop": 2}))
    # an Init state in L (a prefix of one state), and a prefix of 301 states
    out.append(bfs_form("lasso-prefix-1", 3, [(0, 1, 0), (1, 2, 1), (2, 0, 0)], 2, [0, 1, 2], [0],
                        lasso_only=True, note={"kind": 1, "prefix": 1}))
    tail = 300
    e = [(i, i + 1, 0) for i in range(tail)] + _ring([tail, tail + 1, tail + 2], lambda k: k % 2)
    out.append(bfs_form("lasso-prefix-301", tail + 3, e, 2, [tail, tail + 1, tail + 2], [0],
                        lasso_only=True, note={"kind": 1, "prefix": 301}))
    # WF_vars(Next): the walk from 1 enters the cycle 2 -> 3 -> 4 -> 2, and the walk 1 -> 2 -> 3 ends
    out.append(hub_form("walk-into-cycle", 5, [(1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 2, 0)], 1, next_only=True,
                        note={"kind": 1, "path": [0, 1, 2, 3, 4], "loop": 2}))
    out.append(hub_form("walk-into-terminal", 4, [(1, 2, 0), (2, 3, 0)], 1, next_only=True,
                        note={"kind": 2, "path": [0, 1, 2, 3]}))
    return out


DEGREES = (0, 1, 1, 2, 2, 3, 4, 8)
# (n before the BFS drops what is unreachable, P, seed): the seeds whose instance has an SCC of more than 64
# states and an SCC of more than one state that is not fair (tests/test_live_graphs_host.py asserts both)
RANDOM_CASES: List[Tuple[int, int, int]] = [
    (20000, 5, 1), (20000, 5, 4), (20000, 5, 5), (20000, 8, 1), (20000, 8, 3), (20000, 8, 5),
    (70000, 5, 1), (70000, 5, 4), (70000, 5, 5), (70000, 8, 3), (70000, 8, 7), (70000, 8, 8)]


def random_graph(n: int, P: int, seed: int) -> Graph:
    """Degrees from DEGREES; 90% of the targets within [-40, +60] of the source,
    the rest anywhere; a random process per edge; stay with probability 0.9;
    state 0 the Init state; renumbered by BFS."""
    rnd = random.Random(seed)
    edges: List[Edge] = []
    for i in range(n):
        for _ in range(rnd.choice(DEGREES)):
            j = i + rnd.randint(-40, 60) if rnd.random() < 0.9 else rnd.randrange(n)
            edges.append((i, min(max(j, 0), n - 1), rnd.randrange(P)))
    stay = [i for i in range(n) if rnd.random() < 0.9]
    return bfs_form(f"random-{n}-P{P}-s{seed}", n, edges, P, stay, [0])


def synthetic() -> List[Graph]:
    return (rings() + scc_chains() + straddle() + shared_and_cut() + uncounted_edges() + process_counts() +
            empty_and_full() + lasso_shapes())


def random_cases() -> List[Graph]:
    return [cached_random(*c) for c in RANDOM_CASES]


_random: Dict[Tuple[int, int, int], Graph] = {}


def cached_random(n: int, P: int, seed: int) -> Graph:
    if (n, P, seed) not in _random:
        _random[(n, P, seed)] = random_graph(n, P, seed)
    return _random[(n, P, seed)]


# ------------------------------------------------- the host models' answer, once

@dataclass
class Reference:
    fair: object                 # fair_model.FairVerdict
    next_live: Set[int]          # live_model.eliminate's L (WF_vars(Next); also what the trim leaves)
    terminal: Set[int]
    next_rounds: int
    schedule: object             # fair_model.Schedule


_refs: Dict[str, Reference] = {}


def reference(g: Graph) -> Reference:
    """fair_check, eliminate and the Jacobi schedule of g (cached by name, never modified)."""
    import fair_model
    import live_model
    if g.name not in _refs:
        v = fair_model.fair_check(g.succ, g.procs, g.nproc, g.S, g.level)
        L, terminal, rounds = live_model.eliminate(g.succ, g.S)
        _refs[g.name] = Reference(v, L, terminal, rounds, fair_model.jacobi_schedule(g.succ, g.procs, g.nproc, g.S))
    return _refs[g.name]


# ------------------------------------------------------------- kc_live_selftest

FORE = 8                         # KC_EMIT_FORE
GUARD8, GUARD32 = 0xA5, 0xA5A5A5A5
JUNK8, JUNK32 = 0x5A, 0x5A5A5A5A
RES = ("stay", "stay_terminal", "removed", "rounds", "sccs", "fair_sccs", "fair_states", "live", "live_terminal",
       "scc_launches", "violated", "kind", "prefix", "loop", "len", "code")


@dataclass
class Run:
    rc: int
    res: Dict[str, int]
    alive: np.ndarray
    terminal: np.ndarray
    enabled: np.ndarray
    comp: np.ndarray
    fair: np.ndarray
    path: np.ndarray             # all path_cap entries
    guards_ok: bool


def selftest(lib, g: Graph, fairness: int, path_cap: int = 0, aft: int = 5, words=None, par=None) -> Run:
    """One kc_live_selftest call on g: sections pre-filled with junk between
    guard words; guards_ok = every fore and aft guard came back as sent."""
    import ctypes as C
    deg, edges, eproc, stay, parent, level = words if words is not None else g.words()
    n = len(deg)
    cap = path_cap or (n * (g.nproc + 3) if fairness else n)
    p = np.array(par if par is not None else [n, g.nproc, fairness, path_cap, aft], dtype=np.uint64)
    kinds = [(n, GUARD8, JUNK8)] * 3 + [(n, GUARD32, JUNK32), (n, GUARD8, JUNK8), (cap, GUARD32, JUNK32)]
    secs = []
    for m, gv, jv in kinds:
        secs.append(np.concatenate([np.full(FORE, gv), np.full(m, jv), np.full(aft, gv)]).astype(np.uint64))
    out = np.ascontiguousarray(np.concatenate(secs))
    sent = out.copy()
    res = np.zeros(16, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    keep = [np.ascontiguousarray(x) for x in (deg, edges, eproc, stay, parent, level)]
    rc = lib.kc_live_selftest(ptr(p), len(p), ptr(keep[0]), ptr(keep[1]), len(keep[1]), ptr(keep[2]), ptr(keep[3]),
                              ptr(keep[4]), ptr(keep[5]), ptr(out), len(out), ptr(res), len(res))
    parts, ok, at = [], True, 0
    for m, gv, jv in kinds:
        sec = out[at:at + FORE + m + aft]
        ok = ok and bool((sec[:FORE] == gv).all()) and bool((sec[FORE + m:] == gv).all())
        parts.append(sec[FORE:FORE + m].astype(np.int64))
        at += FORE + m + aft
    if rc != 0:
        ok = ok and bool((out == sent).all())
    r = {k: int(x) for k, x in zip(RES, res)}
    return Run(rc, r, *parts, guards_ok=ok)
