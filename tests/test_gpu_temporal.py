"""User-defined temporal formulas on the GPU against the host
model of tests/temporal_model.py (the graph from the CPU oracle, P and Q by
pred.evaluate, L by live_model.eliminate or fair_model.fair_check).

First the user spellings of the built-in properties: every result field but
the timings and the names, and the counterexample, equal the built-in run's.
(States are compared as tuples, never by discovery index: within a level wider
than a wave the index a state gets depends on which wave's atomicAdd comes
first, so two runs may number nofaults_111's states differently.  The walk
under WF_vars(Next) depends on its first state and the successor order alone;
the legs under per-process fairness pick the smallest index of a level, so on
nofaults_111 their traces are validated, not compared.)
Then the table of trigger rows, whose literals were computed with the model on
the CPU (tests/test_temporal_host.py recomputes them); every test recomputes
its row with the model as well.  Then the refusals of the C interface."""
import dataclasses

import pytest

import kubecheck
from kubecheck import LivenessChecker, ModelConfig, pred

import fair_model
import live_model
import temporal_model as tm

pytestmark = pytest.mark.gpu

# rounds and scc_rounds count launches of kernels that update in place (a stale read costs rounds only), so two
# runs of one property may differ in them: bounded below, as tests/test_gpu_liveness.py and test_gpu_fairness.py do
NOT_COMPARED = ("property", "formula", "seconds", "build_ms", "trim_ms", "scc_ms", "trigger_stay", "trigger_live",
                "rounds", "scc_rounds")
# where the numbering varies the legs may end in another state of the level: a terminal one or one of a fair SCC
TRACE_FIELDS = ("trace", "trace_actions", "trace_text", "trace_len", "loop_start", "kind")
# the built-in properties and the models they are defined and tabulated on (tests/test_gpu_liveness.py)
BUILTIN_ROWS = [(m, p) for p in tm.SPELLINGS for m in live_model.MODELS]


@pytest.mark.parametrize("fairness", ["next", "process"])
@pytest.mark.parametrize("name,pname", BUILTIN_ROWS, ids=[f"{m}-{p}" for m, p in BUILTIN_ROWS])
def test_user_spelling_of_a_builtin_is_the_builtin_run(oracle, name, pname, fairness):
    cfg = ModelConfig(**live_model.MODELS[name])
    formula = tm.SPELLINGS[pname]
    if pname == "SomeActorRestarts" and cfg.np == 0:
        formula = tm.SPELLING_NO_CONTROLLERS
    with LivenessChecker(cfg, pname, fairness=fairness) as lc:
        want = lc.run()
        want_alive = alive_set(lc)
    with LivenessChecker(cfg, formula=formula, name="Mine", fairness=fairness) as lc:
        got = lc.run()
        got_alive = alive_set(lc)
    assert (got.property, got.formula, want.formula) == ("Mine", formula, None)
    a, b = dataclasses.asdict(got), dataclasses.asdict(want)
    by_index = name == "nofaults_111" and fairness == "process"     # (the module docstring)
    for k in NOT_COMPARED + (TRACE_FIELDS if by_index else ()):
        del a[k], b[k]
    assert a == b                                  # the trace among them: same first state, same lasso kernels
    for r in (got, want):
        assert r.rounds >= 1 and (r.scc_rounds >= 1) == (fairness == "process")
    assert got_alive == want_alive and len(got_alive) == got.states
    if by_index and got.violated:
        m = live_model.model(oracle, name)
        v = tm.check(m, name, formula, fairness)
        check_counterexample(m, name, formula, v, got, fairness)
    assert (want.trigger_stay, want.trigger_live) == (0, 0)
    # T = S for ReconcileCompletes and every state for the other two: S and L lie inside it
    assert (got.trigger_stay, got.trigger_live) == (got.stay_states, got.live_states)
    assert got.violated == (got.trigger_live > 0)


def alive_set(lc):
    """{(tuple, in L)} of the last run."""
    tuples, alive = lc.alive()
    return {(tuple(int(x) for x in t), bool(a)) for t, a in zip(tuples, alive)}


def check_counterexample(m, name, formula, v, r, fairness):
    mod = tm.procs_of_model(name)
    form, p_ast, q_ast, _, _ = tm.stay_and_trigger(m, name, formula)
    assert r.kind in ("back-to-state", "stuttering")
    assert r.trace_len == len(r.trace) == len(r.trace_actions) >= r.prefix_len >= 1
    trace = [tuple(t) for t in r.trace]
    idx = [m.index[t] for t in trace]
    assert m.level[idx[0]] == 1 and r.trace_actions[0] is None                      # an Init state
    for k in range(1, len(trace)):
        assert (r.trace_actions[k], trace[k]) in m.successors_of(trace[k - 1]), k   # a real successor
    # the prefix: a shortest one to a state of L /\ T on the first level that has one (which of that level's
    # states has the smallest discovery index is the device's numbering; the model's is v.first)
    first = idx[r.prefix_len - 1]
    assert first in v.live_trigger and r.prefix_len == m.level[first] == m.level[v.first]
    if form == 0:
        assert pred.evaluate(p_ast, trace[r.prefix_len - 1], *mod)
    else:
        assert m.level[first] == 1
    assert first in v.live
    assert all(i not in v.live_trigger for i in idx[:r.prefix_len - 1])
    for k in range(r.prefix_len - 1, len(trace)):
        assert not pred.evaluate(q_ast, trace[k], *mod), k                           # ~Q from there on
        assert idx[k] in v.live, k
    others = [j for j in m.succ[idx[-1]] if j != idx[-1]]
    if r.kind == "back-to-state":
        assert r.prefix_len - 1 <= r.loop_start < r.trace_len
        assert idx[r.loop_start] in others
    else:
        assert r.loop_start == -1 and not others
    if fairness == "process":
        # the lasso from the trigger state on, by the definition: the graph's levels and the verdict as seen from
        # that state (it is the lasso's "Init" state, and the prefix to it has one state)
        level = list(m.level)
        level[first] = 1
        want = dataclasses.replace(v.fair, min_level=1)
        cut = r.prefix_len - 1
        fair_model.check_lasso_graph(m.succ, fair_model.procs_of(m), sum(mod), level, want, idx[cut:], 1, r.kind,
                                     r.loop_start - cut if r.loop_start >= 0 else -1)


@pytest.mark.parametrize("fairness", ["next", "process"])
@pytest.mark.parametrize("row", tm.ROWS, ids=[f"{r[0]}-{k}" for k, r in enumerate(tm.ROWS)])
def test_trigger_row(oracle, row, fairness):
    name, formula, n_stay, n_trig_stay, nxt, proc = row
    m = live_model.model(oracle, name)
    v = tm.check(m, name, formula, fairness)
    # the literals against the model
    first = v.first
    prefix = None if first is None else m.level[first]
    assert (len(v.stay), len(v.stay & v.trigger)) == (n_stay, n_trig_stay)
    if fairness == "next":
        assert (len(v.live), len(v.live_trigger), prefix, first, v.rounds) == nxt
    else:
        assert (len(v.fair.fair), len(v.live), len(v.live_trigger), prefix, first) == proc

    with LivenessChecker(ModelConfig(**live_model.MODELS[name]), formula=formula, name="Row", fairness=fairness) as lc:
        r = lc.run()
        got = alive_set(lc)
    print(f"{name} {formula} [{fairness}]: rounds {r.rounds}, build {r.build_ms:.2f} ms, trim {r.trim_ms:.2f} ms, "
          f"|S| {r.stay_states} |L| {r.live_states} |S/\\T| {r.trigger_stay} |L/\\T| {r.trigger_live}")
    assert r.error is None and (r.property, r.formula, r.fairness) == ("Row", formula, fairness)
    assert (r.states, r.edges, r.depth, r.init) == (len(m.states), m.edges, m.depth, m.n_init)
    assert (r.stay_states, r.live_states) == (len(v.stay), len(v.live))
    assert r.live_terminal == len(v.live & v.terminal)
    assert (r.trigger_stay, r.trigger_live) == (len(v.stay & v.trigger), len(v.live_trigger))
    assert r.violated == v.violated == (r.trigger_live > 0)
    if fairness == "next":
        assert 1 <= r.rounds <= v.rounds
    else:
        assert (r.sccs, r.fair_sccs, r.fair_states) == (len(v.fair.sccs), len(v.fair.fair_sccs), len(v.fair.fair))
    # the exact alive set
    assert len(got) == len(m.states)
    assert got == {(t, i in v.live) for i, t in enumerate(m.states)}
    if v.violated:
        check_counterexample(m, name, formula, v, r, fairness)
    else:
        assert (r.kind, r.prefix_len, r.trace_len, r.loop_start, r.trace) == (None, 0, 0, -1, [])


def test_a_handle_takes_formula_after_formula(oracle):
    """One handle, set_formula twice: each run is its own formula's (the program and the trigger bytes are replaced)."""
    name = "nodeadlock_110"
    m = live_model.model(oracle, name)
    with LivenessChecker(ModelConfig(**live_model.MODELS[name]), formula=tm.REQUEST_RESTARTS, name="A") as lc:
        a = lc.run()
        lc.set_formula(tm.EVENTUALLY_CSTART, "B")
        b = lc.run()
        lc.set_formula(tm.REQUEST_RESTARTS, "A")
        a2 = lc.run()
    va, vb = tm.check(m, name, tm.REQUEST_RESTARTS, "next"), tm.check(m, name, tm.EVENTUALLY_CSTART, "next")
    assert (a.violated, a.trigger_live, a.prefix_len) == (True, len(va.live_trigger), 3)
    assert (b.property, b.violated, b.live_states, b.trigger_live, b.trace) == ("B", False, len(vb.live), 0, [])
    assert (a2.trace, a2.trigger_stay, a2.trigger_live) == (a.trace, a.trigger_stay, a.trigger_live)


def test_refusals_are_einval():
    cfg = ModelConfig(**live_model.MODELS["default_101"])
    form, prog = pred.compile_temporal(tm.C8_STORES, 1, 0, 1)
    # property = -1 and no formula: a handle never lacks its formula
    with pytest.raises(kubecheck.KubecheckError) as e:
        LivenessChecker(cfg, property=-1)
    assert e.value.code == -22 and "kc_live_create_formula" in str(e.value)
    # one END, three ENDs, a bad form, a field outside the state, no instruction: at create and at set_formula
    one = pred.compile_invariants(["Cardinality(apiState) >= 1"], 1, 0, 1)
    three = pred.compile_invariants(["TRUE", "FALSE", 'pc["Client"] = "C8"'], 1, 0, 1)
    wide = [pred.P_PUSH, 1, pred.P_END, 0, pred.P_LEAF_CONST | (prog.W << 8) | (1 << 22), 0, pred.P_END | (1 << 8), 0]
    bad = ((0, one, "exactly two"), (0, three, "exactly two"), (2, prog, "form"), (-1, prog, "form"),
           (0, wide, "field outside the state"), (0, [], "1 to 128 instructions"))
    for f, p, why in bad:
        with pytest.raises(kubecheck.KubecheckError) as e:
            LivenessChecker(cfg, program=(f, p))
        assert e.value.code == -22 and why in str(e.value), why
    with LivenessChecker(cfg, program=(form, prog), name="Stores") as lc:
        first = lc.run()
        for f, p, why in bad:
            with pytest.raises(kubecheck.KubecheckError) as e:
                lc.set_program(f, p)
            assert e.value.code == -22 and why in str(e.value), why
        again = lc.run()                              # ... and the handle keeps the formula it had
        assert (first.property, first.trigger_live, first.trace) == ("Stores", 1, again.trace) and first.violated
    # a formula on a handle created with a built-in property
    with LivenessChecker(cfg, "ClientRestarts") as lc:
        with pytest.raises(kubecheck.KubecheckError) as e:
            lc.set_program(form, prog)
        assert e.value.code == -22 and "built-in property" in str(e.value)
        assert lc.run().property == "ClientRestarts"
    # a user formula needs no single client: two clients, where properties 0-2 are refused
    with pytest.raises(kubecheck.KubecheckError):
        LivenessChecker(ModelConfig(nc=2, np=0), "ClientRestarts")
    with LivenessChecker(ModelConfig(nc=2, np=0), formula='<>(pc["Client2"] = "C5")') as lc:
        r = lc.run()
    assert (r.error, r.error_action) == ("assertion", "C4")     # (this model's build meets an Assert: no verdict)
