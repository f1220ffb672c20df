"""Per-process weak fairness without a GPU: kc_live_step_process against the
independent model (tests/fair_model.py) on every edge of the three small
graphs, the model's SCC / F / L functions on hand-made graphs, the fairness
argument and the grown structs of the C ABI, and the command line's option."""
import ctypes as C

import numpy as np
import pytest

import kubecheck
from kubecheck import ModelConfig, Spec, _lib, tlc

import fair_model
import live_model


@pytest.mark.parametrize("name", list(live_model.MODELS))
def test_step_process_matches_model(oracle, name):
    m = live_model.model(oracle, name)
    assert m.self_loops == 0 and m.assert_action is None
    sp = Spec(ModelConfig(**live_model.MODELS[name]))
    nproc = m.nc + m.np + m.ns
    seen = set()
    for i, s in enumerate(m.states):
        succ, fail = sp.successors(np.array(s, dtype=np.uint64))
        assert fail is None and len(succ) == len(m.succ[i])
        got_edges = []
        for k, (action, t) in enumerate(succ):
            t = tuple(int(x) for x in t)
            want = fair_model.edge_process(m, s, action, t)
            assert sp.step_process(s, k) == want, (i, k, action)
            got_edges.append((action, t))
            seen.add(want)
        assert sorted(got_edges) == sorted(m.successors_of(s))
        # past the last successor
        with pytest.raises(kubecheck.KubecheckError) as e:
            sp.step_process(s, len(succ))
        assert e.value.code == -22
    assert seen == set(range(nproc))          # every process steps somewhere


def test_step_process_errors(oracle):
    lib = kubecheck.load()
    assert lib.kc_live_step_process(None, None, 0) == -22
    sp = Spec(ModelConfig())
    t = sp.init()[0]
    with pytest.raises(kubecheck.KubecheckError):
        sp.step_process(t, -1)
    bad = t.copy()
    bad[0] = 1 << 40
    with pytest.raises(kubecheck.KubecheckError):
        sp.step_process(bad, 0)
    # a state whose Next raises an Assert has no successors to name
    m = live_model.Model(oracle, nc=2, np=0, ns=1)
    assert m.assert_action == "C4"
    sp2 = Spec(ModelConfig(nc=2, np=0))
    failing = [s for s in m.states if sp2.successors(np.array(s, dtype=np.uint64))[0] is None]
    assert failing
    with pytest.raises(kubecheck.KubecheckError):
        sp2.step_process(failing[0], 0)


def test_fairness_argument_checks():
    lib = kubecheck.load()
    h = C.c_void_p()
    c = ModelConfig().to_c()
    for f in (-1, 2, 7):
        l = _lib.KcLiveConfig(0, 0, f)
        assert lib.kc_live_create(C.byref(c), C.byref(l), C.byref(h)) == -22, f
        assert b"fairness" in lib.kc_last_error() and not h.value
    # two positional arguments still mean WF_vars(Next)
    assert _lib.KcLiveConfig(1, 64).fairness == 0
    assert kubecheck.FAIRNESS == ("next", "process")
    with pytest.raises(ValueError, match="fairness"):
        kubecheck.LivenessChecker(ModelConfig(), "ReconcileCompletes", fairness="strong")
    assert lib.kc_live_edge_procs(None, None, None, None, 0) == -22


def test_struct_layouts_grow_by_appending():
    names = [f[0] for f in _lib.KcLiveConfig._fields_]
    assert names == ["property", "max_states", "fairness"]
    names = [f[0] for f in _lib.KcLiveResult._fields_]
    assert names[-5:] == ["sccs", "fair_sccs", "fair_states", "scc_rounds", "scc_ms"]
    assert names[-8:-5] == ["seconds", "build_ms", "trim_ms"]
    # (tests/test_live_host.py::test_struct_layouts_match_header compares every offset with the header)
    r = kubecheck.LiveResult(
        property="ReconcileCompletes", states=3, edges=3, init=1, depth=3, stay_states=2, live_states=2,
        live_terminal=0, rounds=1, error=None, error_action=None, error_self=-1, violated=True,
        kind="back-to-state", prefix_len=2, trace_len=3, loop_start=1, seconds=0.0, build_ms=0.0, trim_ms=0.0)
    assert (r.fairness, r.sccs, r.fair_sccs, r.fair_states, r.scc_rounds, r.scc_ms) == ("next", 0, 0, 0, 0, 0.0)


def test_cli_fairness_option():
    a = tlc.parse_args(["-config", "x.cfg", "MC"])
    assert a.fairness == "next"
    a = tlc.parse_args(["-fairness", "process", "-config", "x.cfg", "MC"])
    assert a.fairness == "process" and not a.simulate
    assert tlc.parse_args(["-fairness", "next", "MC"]).fairness == "next"
    with pytest.raises(SystemExit):
        tlc.parse_args(["-fairness", "strong", "MC"])
    for argv in (["-simulate", "-fairness", "process", "MC"], ["-fairness", "next", "-simulate", "num=4", "MC"]):
        with pytest.raises(tlc.CfgError, match="fairness"):
            tlc.parse_args(argv)
    assert tlc.parse_args(["-simulate", "MC"]).fairness == "next"
    # the 2192 line says which fairness was assumed
    nxt = tlc.live_start_message("ReconcileCompletes", "next", 207, 0.0)
    prc = tlc.live_start_message("ReconcileCompletes", "process", 207, 0.0)
    assert nxt.startswith("Checking temporal property ReconcileCompletes under WF_vars(Next) for")
    assert prc.startswith("Checking temporal property ReconcileCompletes under weak fairness of every process for")
    assert "207 total distinct states" in prc


# ---- hand-made graphs through the model's SCC, F and L

def _check(succ, procs, nproc, S):
    return fair_model.fair_check(succ, procs, nproc, set(S))


def test_tarjan():
    #  0 -> 1 -> 2 -> 0 ; 2 -> 3 ; 3 -> 4 -> 3 ; 5 alone ; 6 -> 6
    succ = [[1], [2], [0, 3], [4], [3], [], [6]]
    got = sorted(sorted(c) for c in fair_model.tarjan(succ, set(range(7))))
    assert got == [[0, 1, 2], [3, 4], [5], [6]]
    # induced on a subset the cycle through 1 is cut
    got = sorted(sorted(c) for c in fair_model.tarjan(succ, {0, 2, 3, 4}))
    assert got == [[0], [2], [3, 4]]


def test_self_loop_only_state():
    # 0 -> 1 (process 0); 1 -> 1 (process 1) only: 1 is terminal, no SCC, F = {1}, L = {0, 1}
    v = _check([[1], [1]], [[0], [1]], 2, {0, 1})
    assert v.terminal == {1} and v.enabled == [1, 0]
    assert v.sccs == [] and v.fair == {1} and v.live == {0, 1} and v.violated and v.live_terminal == 1
    # outside S the terminal state does not count
    v = _check([[1], [1]], [[0], [1]], 2, {0})
    assert v.fair == set() and v.live == set() and not v.violated


def test_cycle_that_starves_an_enabled_process_is_not_fair():
    # 0 <-> 1 by process 0; process 1 could leave from either state (to 2, outside S) and never does
    succ = [[1, 2], [0, 2], [2]]
    procs = [[0, 1], [0, 1], [1]]
    v = _check(succ, procs, 2, {0, 1})
    assert [sorted(c) for c in v.sccs] == [[0, 1]]
    assert v.fair_sccs == [] and v.fair == set() and v.live == set() and not v.violated
    # WF_vars(Next) alone keeps the cycle
    L, _, _ = live_model.eliminate(succ, {0, 1})
    assert L == {0, 1}


def test_same_cycle_with_the_process_disabled_in_one_state_is_fair():
    # as above, but state 1 has no process-1 step: process 1 is not continuously enabled
    succ = [[1, 2], [0], [2]]
    procs = [[0, 1], [0], [1]]
    v = _check(succ, procs, 2, {0, 1})
    assert [sorted(c) for c in v.fair_sccs] == [[0, 1]]
    assert v.fair == {0, 1} and v.live == {0, 1} and v.violated and v.live_terminal == 0
    # ... and fair too if instead process 1 takes a step inside the cycle
    v = _check([[1, 2], [0, 2], [2]], [[0, 1], [1, 1], [1]], 2, {0, 1})
    assert v.fair == {0, 1}


def test_fair_sub_cycle_inside_a_larger_scc():
    # SCC {0, 1, 2, 3}: 0 <-> 1 by process 0 starves process 1 (enabled in both: 0 -> 2, 1 -> 2), but the
    # SCC as a whole holds the process-1 edges 0 -> 2, 1 -> 2 and 3 -> 0; the maximal SCC decides: fair.
    # 4 -> 0 leads in (L), 5 is reachable from 3 but outside S.
    succ = [[1, 2], [0, 2], [3], [0, 5], [0], [5]]
    procs = [[0, 1], [0, 1], [0], [1, 0], [0], [0]]
    v = _check(succ, procs, 2, {0, 1, 2, 3, 4})
    assert [sorted(c) for c in v.sccs] == [[0, 1, 2, 3]]
    assert [sorted(c) for c in v.fair_sccs] == [[0, 1, 2, 3]]
    assert v.fair == {0, 1, 2, 3} and v.live == {0, 1, 2, 3, 4} and v.live_terminal == 0
    # cut the way back (3 outside S): what is left of the SCC is the starving cycle alone
    v = _check(succ, procs, 2, {0, 1, 2, 4})
    assert [sorted(c) for c in v.sccs] == [[0, 1]] and v.fair == set() and v.live == set()
