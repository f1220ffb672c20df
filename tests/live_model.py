"""An independent host model of the liveness check (include/kubecheck.h,
"Liveness").

The reachable graph is built from the CPU oracle alone (oracle.successors, Init
states from its level 1); `stay` is written on canonical tuples; the
elimination runs in synchronous (Jacobi) rounds on Python sets.  Nothing here
runs the product's code (csrc/liveness.h, liveness.hip), so kc_live_stay and
the kernels are checked against it.

Not a test module: tests/test_live_host.py and tests/test_gpu_liveness.py use it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

PROPERTIES = ("ReconcileCompletes", "CleansUpProperly", "ClientRestarts", "SomeActorRestarts")
L_CStart, L_PVCStart = 1, 14     # pc values of the canonical tuple (include/kubecheck.h)
PER_PROC = 19                    # tuple words per process


def stay(prop: int, t, nc: int, np_: int) -> bool:
    """stay(t) of property `prop` on a canonical tuple."""
    A = nc + np_
    U = 1 << (A + 2)
    secret = t[0] & ((1 << (U // 2)) - 1)        # apiState's versions of Secret/foo
    if prop == 3:
        return all(t[1 + PER_PROC * a] != (L_CStart if a < nc else L_PVCStart) for a in range(A))
    assert nc == 1
    sr = t[5]
    if prop == 0:
        return bool(sr)
    if prop == 1:
        return (not sr) and secret != 0
    if prop == 2:
        return t[1] != L_CStart
    raise ValueError(prop)


def eliminate(succ: List[List[int]], alive: Set[int]):
    """The elimination on a graph given as successor index lists: (L, terminal
    states, Jacobi rounds with the last, empty one counted).  Edges s -> s are
    dropped: s is terminal if it has no successor other than itself; a round
    removes every alive, non-terminal state with no alive successor other than
    itself, all judged on the set the round started with."""
    terminal = {i for i, out in enumerate(succ) if all(j == i for j in out)}
    alive = set(alive)
    rounds = 0
    while True:
        rounds += 1
        dead = {i for i in alive
                if i not in terminal and not any(j != i and j in alive for j in succ[i])}
        if not dead:
            return alive, terminal, rounds
        alive -= dead


def check_next_lasso(succ, level, S: Set[int], L: Set[int], idx: List[int], prefix_len: int, kind: str,
                     loop_start: int) -> None:
    """The counterexample under WF_vars(Next), as state indices of the graph
    `succ` with BFS levels `level`, is valid: an Init state, steps of the graph,
    a shortest prefix to L (the elimination's result for the stay set S),
    everything from there on inside S and L, then a step back to a state of the
    walk or a state with no successor other than itself."""
    assert kind in ("back-to-state", "stuttering")
    assert len(idx) >= prefix_len >= 1 and level[idx[0]] == 1
    for a, b in zip(idx, idx[1:]):
        assert b in succ[a] and a != b
    assert prefix_len == min(level[i] for i in L)
    assert all(i in S and i in L for i in idx[prefix_len - 1:])
    assert all(i not in L for i in idx[:prefix_len - 1])
    others = [j for j in succ[idx[-1]] if j != idx[-1]]
    if kind == "back-to-state":
        assert prefix_len - 1 <= loop_start < len(idx)
        assert idx[loop_start] in others
    else:
        assert loop_start == -1 and not others


@dataclass
class Verdict:
    stay: Set[int]
    live: Set[int]
    rounds: int
    live_terminal: int
    min_level: Optional[int]     # the smallest BFS level (Init = 1) of a state of L

    @property
    def violated(self) -> bool:
        return bool(self.live)


class Model:
    """The reachable graph of one model configuration (flags as ModelConfig's)."""

    def __init__(self, oracle, nc=1, np=1, ns=1, **flags):
        self.nc, self.np, self.ns = nc, np, ns
        self.oracle = oracle
        self.ocfg = oracle.config(nc, np, ns, **flags)
        init = [tuple(int(x) for x in t) for t in oracle.level_tuples(self.ocfg, 1)]
        self.states: List[Tuple[int, ...]] = []
        self.index: Dict[Tuple[int, ...], int] = {}
        self.level: List[int] = []
        self.succ: List[List[int]] = []            # successor indices, in the oracle's order
        self.actions: List[List[str]] = []         # ... and the action of each
        self.assert_action: Optional[str] = None   # an Assert met: the graph is not complete
        for s in init:
            self._add(s, 1)
        i = 0
        while i < len(self.states):
            lst, fail = oracle.successors(self.ocfg, np_array(self.states[i]))
            if lst is None:
                self.assert_action = fail
                return
            out, acts = [], []
            for a, x in lst:
                x = tuple(int(v) for v in x)
                out.append(self._add(x, self.level[i] + 1))
                acts.append(a)
            self.succ.append(out)
            self.actions.append(acts)
            i += 1
        self.n_init = len(init)
        self.edges = sum(len(o) for o in self.succ)
        self.depth = max(self.level)
        self.self_loops = sum(1 for i, o in enumerate(self.succ) if i in o)

    def _add(self, s, level) -> int:
        j = self.index.get(s)
        if j is None:
            j = len(self.states)
            self.index[s] = j
            self.states.append(s)
            self.level.append(level)
        return j

    def stay(self, prop: int, t) -> bool:
        return stay(prop, t, self.nc, self.np)

    def check(self, prop: int) -> Verdict:
        S = {i for i, t in enumerate(self.states) if self.stay(prop, t)}
        L, terminal, rounds = eliminate(self.succ, S)
        return Verdict(S, L, rounds, len(L & terminal), min((self.level[i] for i in L), default=None))

    def successors_of(self, t):
        """[(action, tuple)] of a reachable state, in the oracle's order."""
        i = self.index[tuple(int(x) for x in t)]
        return [(a, self.states[j]) for a, j in zip(self.actions[i], self.succ[i])]


def np_array(t):
    return np.array(t, dtype=np.uint64)


# the models of the expected-values table: name -> ModelConfig flags
MODELS = {
    "default_101": dict(nc=1, np=0, ns=1),
    "nodeadlock_110": dict(nc=1, np=1, ns=0, check_deadlock=False),
    "nofaults_111": dict(nc=1, np=1, ns=1, can_fail=False, can_timeout=False),
}
_cache: Dict[str, Model] = {}


def model(oracle, name: str) -> Model:
    """The (cached, never modified) graph of one of MODELS."""
    if name not in _cache:
        _cache[name] = Model(oracle, **MODELS[name])
    return _cache[name]
