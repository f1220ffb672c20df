"""Host model of user-defined temporal formulas, in the
oracle's tuple space.

TEST INFRASTRUCTURE ONLY.  The graph is live_model.Model's (the CPU oracle's
successors); P and Q are judged with pred.evaluate on canonical tuples; L comes
from live_model.eliminate (WF_vars(Next)) or fair_model.fair_check (per-process
fairness), which take an arbitrary stay set.  Nothing here sees a compiled
program or the packed state.

Not a test module: tests/test_temporal_host.py, tests/test_gpu_temporal.py and
tests/test_tlc_temporal_cli.py use it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Set, Tuple

import fair_model
import live_model
from kubecheck import pred

# the user spellings of the built-in properties: property -> formula
SPELLINGS = {
    "ReconcileCompletes": 'shouldReconcile["Client"] ~> ~shouldReconcile["Client"]',
    "ClientRestarts": '[]<>(pc["Client"] = "CStart")',
    "SomeActorRestarts": r'[]<>((\E c \in Clients : pc[c] = "CStart") \/ (\E p \in Controllers : pc[p] = "PVCStart"))',
}
# SomeActorRestarts on a model without controllers: the quantifier over Controllers has nothing to range over
SPELLING_NO_CONTROLLERS = r'[]<>(\E c \in Clients : pc[c] = "CStart")'

C5_RECONCILED = 'pc["Client"] = "C5" ~> ~shouldReconcile["Client"]'
ALWAYS_RECONCILED = '[]<>(~shouldReconcile["Client"])'
C2_RESTARTS = 'pc["Client"] = "C2" ~> pc["Client"] = "CStart"'
REQUEST_RESTARTS = r'"Client" \in DOMAIN requests ~> pc["Client"] = "CStart"'
C8_STORES = 'pc["Client"] = "C8" ~> Cardinality(apiState) >= 1'
EVENTUALLY_RECONCILED = '<>(~shouldReconcile["Client"])'
EVENTUALLY_CSTART = '<>(pc["Client"] = "CStart")'

# (model, formula, |S|, |S /\ T|, then under WF_vars(Next): |L|, |L /\ T|, prefix_len, first index, Jacobi rounds,
#  then under per-process fairness: |F|, |L|, |L /\ T|, prefix_len, first index); None = holds, no counterexample.
# Computed on the CPU with this module; every test recomputes its row and also asserts the literal.
ROWS = [
    ("nofaults_111", C5_RECONCILED, 7398, 0, (7398, 0, None, None, 1), (5370, 7155, 0, None, None)),
    ("nofaults_111", ALWAYS_RECONCILED, 7398, 7398, (7398, 7398, 1, 1, 1), (5370, 7155, 7155, 1, 1)),
    ("nofaults_111", C2_RESTARTS, 7591, 81, (7591, 81, 24, 422, 1), (160, 6102, 0, None, None)),
    ("nodeadlock_110", REQUEST_RESTARTS, 105, 56, (99, 52, 3, 6, 3), (15, 63, 28, 3, 6)),
    ("default_101", C8_STORES, 33, 1, (30, 1, 6, 20, 2), (24, 30, 1, 6, 20)),
    ("default_101", EVENTUALLY_RECONCILED, 193, 1, (193, 1, 1, 1, 1), (183, 193, 1, 1, 1)),
    ("nodeadlock_110", EVENTUALLY_CSTART, 105, 0, (99, 0, None, None, 3), (15, 63, 0, None, None)),
]


def procs_of_model(name: str) -> Tuple[int, int, int]:
    kw = live_model.MODELS[name]
    return kw["nc"], kw["np"], kw["ns"]


@dataclass
class Verdict:
    form: int
    stay: Set[int]
    trigger: Set[int]
    live: Set[int]
    terminal: Set[int]
    rounds: Optional[int]                      # Jacobi trim rounds (WF_vars(Next) only)
    fair: Optional[fair_model.FairVerdict]     # per-process fairness only

    @property
    def live_trigger(self) -> Set[int]:
        return self.live & self.trigger

    @property
    def violated(self) -> bool:
        return bool(self.live_trigger)

    @property
    def first(self) -> Optional[int]:
        return min(self.live_trigger) if self.live_trigger else None


_sets: Dict[tuple, tuple] = {}


def stay_and_trigger(m, name: str, formula: str):
    """(form, P, Q, S, T) of a formula on live_model.Model m: S = the states where Q is FALSE, T = the states
    where P holds (form 0) or the Init states (form 1)."""
    key = (name, formula)
    if key not in _sets:
        mod = procs_of_model(name)
        form, p_ast, q_ast = pred.parse_temporal(formula, *mod)
        stay = {i for i, t in enumerate(m.states) if not pred.evaluate(q_ast, t, *mod)}
        if form == 0:
            trig = {i for i, t in enumerate(m.states) if pred.evaluate(p_ast, t, *mod)}
        else:
            trig = {i for i in range(len(m.states)) if m.level[i] == 1}
        _sets[key] = (form, p_ast, q_ast, stay, trig)
    return _sets[key]


def check(m, name: str, formula: str, fairness: str) -> Verdict:
    form, _, _, stay, trig = stay_and_trigger(m, name, formula)
    if fairness == "next":
        live, terminal, rounds = live_model.eliminate(m.succ, stay)
        return Verdict(form, stay, trig, live, terminal, rounds, None)
    fv = fair_model.fair_check(m.succ, fair_model.procs_of(m), sum(procs_of_model(name)), stay, m.level)
    return Verdict(form, stay, trig, fv.live, fv.terminal, None, fv)
