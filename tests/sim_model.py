"""An independent model of simulation mode (include/kubecheck.h, "Simulation").

The RNG is written out in plain Python integers; successor lists come from the
CPU oracle (oracle.successors) and Init states from its level 1; the invariant
verdicts come from Spec.check_invariants, which tests/test_spec_lowering.py
pins to the oracle state by state.  Nothing here runs the product's walk code
(csrc/simulate.h), so the kernel and kc_sim_replay are checked against it.

Not a test module: tests/test_sim_host.py and tests/test_gpu_simulate.py use it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

M64 = (1 << 64) - 1
KINDS = {"running": 0, "assertion": 1, "invariant": 2, "deadlock": 3, "depth": 4, "terminated": 5}


def mix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def key(seed: int, w: int) -> int:
    return mix(mix(seed) ^ w)


def rand(seed: int, w: int, k: int) -> int:
    return mix(key(seed, w) ^ k)


def pick(r: int, n: int) -> int:
    return (r * n) >> 64


@dataclass
class Walk:
    kind: str                       # a key of KINDS
    states: List[Tuple[int, ...]]   # s_0 .. s_k
    actions: List[Optional[str]]    # the action that led to each state (None for s_0)
    choices: List[int]              # successor index chosen at s_0 .. s_{k-1}
    info: Optional[str] = None      # the failing action / the violated invariant

    @property
    def length(self) -> int:
        return len(self.states)


@dataclass
class Totals:
    walks: List[Walk]
    steps: int = 0
    act_steps: Dict[str, int] = field(default_factory=dict)
    walks_error: int = 0
    walks_depth: int = 0
    walks_terminated: int = 0
    visited: Set[Tuple[int, ...]] = field(default_factory=set)
    error_walk: Optional[int] = None    # the error walk with the smallest (length, walk)


class Model:
    """Walks of one model configuration (flags as ModelConfig's)."""

    def __init__(self, oracle, nc=1, np=1, ns=1, **flags):
        from kubecheck import ModelConfig, Spec

        self.oracle = oracle
        self.check_deadlock = flags.get("check_deadlock", True)
        self.ocfg = oracle.config(nc, np, ns, **flags)
        self.spec = Spec(ModelConfig(nc=nc, np=np, ns=ns, **flags))
        self.init = [tuple(int(x) for x in t) for t in oracle.level_tuples(self.ocfg, 1)]
        self._succ: Dict[Tuple[int, ...], tuple] = {}
        self._inv: Dict[Tuple[int, ...], Optional[str]] = {}

    def successors(self, s):
        r = self._succ.get(s)
        if r is None:
            lst, fail = self.oracle.successors(self.ocfg, np.array(s, dtype=np.uint64))
            r = (None if lst is None else [(a, tuple(int(v) for v in x)) for a, x in lst], fail)
            self._succ[s] = r
        return r

    def invariant(self, s) -> Optional[str]:
        if s not in self._inv:
            self._inv[s] = self.spec.check_invariants(np.array(s, dtype=np.uint64))
        return self._inv[s]

    def walk(self, seed: int, depth: int, w: int) -> Walk:
        s = self.init[pick(rand(seed, w, 0), len(self.init))]
        wk = Walk("running", [s], [None], [])
        k = 0
        while True:
            inv = self.invariant(s)
            if inv is not None:
                wk.kind, wk.info = "invariant", inv
                return wk
            if k + 1 == depth:
                wk.kind = "depth"
                return wk
            succ, fail = self.successors(s)
            if succ is None:
                wk.kind, wk.info = "assertion", fail
                return wk
            if not succ:
                wk.kind = "deadlock" if self.check_deadlock else "terminated"
                return wk
            t = pick(rand(seed, w, k + 1), len(succ))
            a, s = succ[t]
            wk.states.append(s)
            wk.actions.append(a)
            wk.choices.append(t)
            k += 1

    def run(self, seed: int, num_walks: int, depth: int) -> Totals:
        from kubecheck import ACTIONS

        tot = Totals(walks=[self.walk(seed, depth, w) for w in range(num_walks)])
        tot.act_steps = {a: 0 for a in ACTIONS}
        best = None
        for w, wk in enumerate(tot.walks):
            tot.steps += len(wk.choices)
            for a in wk.actions[1:]:
                tot.act_steps[a] += 1
            tot.visited.update(wk.states)
            if wk.kind in ("assertion", "invariant", "deadlock"):
                tot.walks_error += 1
                if best is None or (wk.length, w) < best:
                    best = (wk.length, w)
            elif wk.kind == "depth":
                tot.walks_depth += 1
            else:
                tot.walks_terminated += 1
        tot.error_walk = None if best is None else best[1]
        return tot
