"""The liveness checker's graph kernels and host loops (csrc/live_graph.h: the
trim, the SCCs by max-colour push and backward pull, the witness accumulation,
F, the closure to L, the lassos) on made graphs, through kc_live_selftest,
against tests/fair_model.py (Tarjan, F and L by the definition) and
tests/live_model.py (the elimination): the exact alive, terminal, enabled and
fair arrays, the SCC partition, every counter, the verdict, the validity of the
lasso, the guard words, and launch counts within the Jacobi simulation's.

tests/live_graphs.py has the families and says what each is for;
tests/test_live_graphs_host.py checks the generators and the models on the
host."""
import numpy as np
import pytest

import kubecheck

import fair_model
import live_graphs
import live_model
from live_graphs import JUNK8, JUNK32

pytestmark = pytest.mark.gpu

SYNTHETIC = live_graphs.synthetic()
CASES = [(g, f) for g in SYNTHETIC for f in (0, 1) if not (f == 0 and g.lasso_only) and not (f == 1 and g.next_only)]
KIND = {1: "back-to-state", 2: "stuttering"}
NONE = 0xffffffff


def member(n, s):
    out = np.zeros(n, dtype=np.int64)
    out[sorted(s)] = 1
    return out


def check_run(g, fairness, r):
    """Everything kc_live_selftest returned for g against the host models."""
    ref = live_graphs.reference(g)
    want, n, S = ref.fair, g.n, g.S
    res = r.res
    assert r.rc == 0 and res["code"] == 0, kubecheck.load().kc_last_error()
    assert r.guards_ok
    assert (r.terminal == member(n, want.terminal)).all() and want.terminal == ref.terminal
    assert (res["stay"], res["stay_terminal"]) == (len(S), len(S & ref.terminal))
    # the trim: the same under both fairness conditions
    assert res["removed"] == len(S) - len(ref.next_live)
    print(f"{g.name} fairness {fairness}: trim rounds {res['rounds']} (Jacobi {ref.next_rounds}), "
          f"SCC-phase launches {res['scc_launches']} (Jacobi {ref.schedule.launches})")
    assert 1 <= res["rounds"] <= ref.next_rounds
    if fairness == 0:
        live = ref.next_live
        assert (r.alive == member(n, live)).all()
        assert (res["live"], res["live_terminal"]) == (len(live), len(S & ref.terminal))
        assert (res["sccs"], res["fair_sccs"], res["fair_states"], res["scc_launches"]) == (0, 0, 0, 0)
        # the per-process sections are not the WF_vars(Next) run's to touch
        assert (r.enabled == JUNK8).all() and (r.fair == JUNK8).all() and (r.comp == JUNK32).all()
    else:
        live = want.live
        assert (r.alive == member(n, live)).all()
        assert (r.enabled == np.array(want.enabled)).all()
        assert (r.fair == member(n, want.fair)).all()
        # the SCC partition of what the trim left: a label is the largest member of its class (the root at
        # the round that found it), a state that is an SCC of its own carries its index, the rest nothing
        cls = {i: top for c in want.sccs for top in [max(c)] for i in c}
        assert all(set(c) <= ref.next_live for c in want.sccs)
        expect = np.array([cls.get(i, i) if i in ref.next_live else NONE for i in range(n)], dtype=np.int64)
        assert (r.comp == expect).all(), np.flatnonzero(r.comp != expect)[:10]
        assert (res["sccs"], res["fair_sccs"], res["fair_states"]) == (len(want.sccs), len(want.fair_sccs), len(want.fair))
        assert (res["live"], res["live_terminal"]) == (len(live), want.live_terminal)
        assert 1 <= res["scc_launches"] <= ref.schedule.launches
    violated = bool(want.fair) if fairness else bool(live)
    assert res["violated"] == int(violated)
    if not violated:
        assert (res["kind"], res["prefix"], res["loop"], res["len"]) == (0, 0, 0, 0)
        assert (r.path == JUNK32).all()
        return None
    assert res["kind"] in KIND and 1 <= res["prefix"] <= res["len"] <= len(r.path)
    idx = [int(x) for x in r.path[:res["len"]]]
    assert (r.path[res["len"] + 1:] == JUNK32).all()      # (a closing step may stand right behind the lasso)
    kind = KIND[res["kind"]]
    loop = res["loop"] if res["kind"] == 1 else -1
    if fairness:
        fair_model.check_lasso_graph(g.succ, g.procs, g.nproc, g.level, want, idx, res["prefix"], kind, loop)
    else:
        live_model.check_next_lasso(g.succ, g.level, S, live, idx, res["prefix"], kind, loop)
    # the prefix ends in the L state with the smallest index
    assert idx[res["prefix"] - 1] == min(live)
    return idx


@pytest.mark.parametrize("g,fairness", CASES, ids=[f"{g.name}-f{f}" for g, f in CASES])
def test_family(g, fairness):
    lib = kubecheck.load()
    r = live_graphs.selftest(lib, g, fairness)
    idx = check_run(g, fairness, r)
    note = g.note
    if g.lasso_only or g.next_only:
        assert r.res["kind"] == note["kind"]
        if "path" in note:
            assert idx == note["path"]
        if "loop" in note:
            assert r.res["loop"] == note["loop"]
        if "prefix" in note:
            assert r.res["prefix"] == note["prefix"]
        if "through" in note:               # every process's only step inside the SCC is on the cycle
            cyc = idx[r.res["loop"]:]
            steps = set(zip(cyc, cyc[1:] + cyc[:1]))
            assert set(note["through"]) <= steps


@pytest.mark.parametrize("case", live_graphs.RANDOM_CASES,
                         ids=[f"{n}-P{P}-s{s}" for n, P, s in live_graphs.RANDOM_CASES])
@pytest.mark.parametrize("fairness", (0, 1))
def test_random_graph(case, fairness):
    g = live_graphs.cached_random(*case)
    want = live_graphs.reference(g).fair
    # what the seed was kept for
    assert max(len(c) for c in want.sccs) > 64 and len(want.fair_sccs) < len(want.sccs)
    r = live_graphs.selftest(kubecheck.load(), g, fairness)
    check_run(g, fairness, r)


def test_lasso_that_does_not_fit_is_an_error_not_an_overrun():
    lib = kubecheck.load()
    g = next(x for x in SYNTHETIC if x.name == "lasso-far-witnesses")
    r = live_graphs.selftest(lib, g, 1, path_cap=10)
    # a leg's path does not fit: the driver gives up with -EIO, nothing past the buffer is written
    assert r.rc == 0 and r.guards_ok
    assert r.res["code"] == (1 << 32) | 5
    assert b"does not fit" in lib.kc_last_error()
    want = live_graphs.reference(g).fair
    assert (r.alive == member(g.n, want.live)).all() and r.res["fair_states"] == len(want.fair)
    # ... and a prefix that does not fit
    g = next(x for x in SYNTHETIC if x.name == "lasso-prefix-301")
    r = live_graphs.selftest(lib, g, 1, path_cap=300)
    assert r.rc == 0 and r.guards_ok and r.res["code"] == 5 and (r.path == JUNK32).all()
    assert b"no counterexample from state 300" in lib.kc_last_error()
    r = live_graphs.selftest(lib, g, 1, path_cap=304)
    assert r.rc == 0 and r.guards_ok and r.res["code"] == 0 and (r.res["prefix"], r.res["kind"]) == (301, 1)


def test_no_aft_guards():
    # aft = 0: each section ends where the kernels' array ends
    g = SYNTHETIC[0]
    r = live_graphs.selftest(kubecheck.load(), g, 1, aft=0)
    assert r.rc == 0 and r.guards_ok and r.res["code"] == 0
    check_run(g, 1, r)
