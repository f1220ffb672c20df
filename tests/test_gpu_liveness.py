"""Liveness checking on the GPU against the independent host model of
tests/live_model.py (the graph from the CPU oracle, stay on canonical tuples,
Jacobi elimination on Python sets): the graph's size, |S|, |L|, the verdict,
the exact alive set and the validity of the counterexample, one test per row
of the expected-values table; then the capacity limit, an Assert during the
build and the command line.

The table's literals were computed with the model on the CPU; every test
recomputes them with the model and also asserts the literal."""
import os
import re
import subprocess
import sys

import pytest

import kubecheck
from kubecheck import LivenessChecker, ModelConfig, PROPERTIES

import live_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_OF = {"nofaults_111": "model1_fail0_timeout0"}

# (model, property, (states, edges, depth), |S|, |L|, Jacobi rounds, terminal in L, min level of L)
# None = the table leaves the cell empty; the model's value is still compared
TABLE = [
    ("default_101", "ReconcileCompletes", (207, 378, 34), 193, 193, 1, 0, 1),
    ("default_101", "CleansUpProperly", (207, 378, 34), 0, 0, None, None, None),
    ("default_101", "ClientRestarts", (207, 378, 34), 173, 0, 15, None, None),
    ("nodeadlock_110", "ReconcileCompletes", (140, 479, 15), 91, 91, None, 2, 1),
    ("nodeadlock_110", "ClientRestarts", (140, 479, 15), 105, 99, 3, 3, 2),
    ("nodeadlock_110", "SomeActorRestarts", (140, 479, 15), 75, 27, 5, 3, None),
    ("nofaults_111", "ReconcileCompletes", (8203, 17018, 109), 7398, 7398, None, None, 1),
    ("nofaults_111", "CleansUpProperly", (8203, 17018, 109), 427, 427, None, None, 25),
    ("nofaults_111", "ClientRestarts", (8203, 17018, 109), 7591, 7591, None, None, None),
    ("nofaults_111", "SomeActorRestarts", (8203, 17018, 109), 6545, 0, 25, None, None),
]


def check_counterexample(m, prop, want, r):
    """The counterexample is valid (its identity is the device's choice)."""
    assert r.kind in ("back-to-state", "stuttering")
    assert r.trace_len == len(r.trace) == len(r.trace_actions) >= r.prefix_len >= 1
    trace = [tuple(t) for t in r.trace]
    assert m.level[m.index[trace[0]]] == 1 and r.trace_actions[0] is None       # an Init state
    for k in range(1, len(trace)):
        assert (r.trace_actions[k], trace[k]) in m.successors_of(trace[k - 1]), k
    assert r.prefix_len == want.min_level
    for k in range(r.prefix_len - 1, len(trace)):
        assert m.stay(prop, trace[k]), k
        assert m.index[trace[k]] in want.live, k
    # a shortest prefix: nothing before its end is in L
    assert all(m.index[t] not in want.live for t in trace[:r.prefix_len - 1])
    others = [t for _, t in m.successors_of(trace[-1]) if t != trace[-1]]
    if r.kind == "back-to-state":
        assert r.prefix_len - 1 <= r.loop_start < r.trace_len
        assert trace[r.loop_start] in others
    else:
        assert r.loop_start == -1 and not others
    assert re.findall(r"^State (\d+):$", r.trace_text, flags=re.M) == [str(k + 1) for k in range(r.trace_len)]


@pytest.mark.parametrize("name,pname,graph,n_stay,n_live,jacobi,n_term,min_level", TABLE,
                         ids=[f"{t[0]}-{t[1]}" for t in TABLE])
def test_table_row(oracle, fixtures, name, pname, graph, n_stay, n_live, jacobi, n_term, min_level):
    m = live_model.model(oracle, name)
    prop = PROPERTIES.index(pname)
    want = m.check(prop)
    # the literals against the model
    assert (len(m.states), m.edges, m.depth) == graph
    assert (len(want.stay), len(want.live)) == (n_stay, n_live)
    assert jacobi in (None, want.rounds) and n_term in (None, want.live_terminal)
    assert min_level in (None, want.min_level)

    with LivenessChecker(ModelConfig(**live_model.MODELS[name]), pname) as lc:
        r = lc.run()
        tuples, alive = lc.alive()
    print(f"{name} {pname}: rounds {r.rounds} (Jacobi {want.rounds}), build {r.build_ms:.2f} ms, "
          f"trim {r.trim_ms:.2f} ms")
    assert r.error is None and r.property == pname
    assert (r.states, r.edges, r.depth, r.init) == (len(m.states), m.edges, m.depth, m.n_init)
    if name in FIXTURE_OF:
        fx = fixtures[FIXTURE_OF[name]]
        assert (r.states, r.edges, r.depth) == (fx["distinct"], fx["generated"] - fx["init"], fx["depth"])
    assert (r.stay_states, r.live_states, r.live_terminal) == (len(want.stay), len(want.live), want.live_terminal)
    assert r.violated == want.violated
    assert 1 <= r.rounds <= want.rounds
    # the exact alive set
    got = {(tuple(int(x) for x in t), bool(a)) for t, a in zip(tuples, alive)}
    assert len(got) == len(tuples) == len(m.states)
    assert got == {(t, i in want.live) for i, t in enumerate(m.states)}
    if want.violated:
        check_counterexample(m, prop, want, r)
    else:
        assert (r.kind, r.prefix_len, r.trace_len, r.loop_start, r.trace) == (None, 0, 0, -1, [])


def test_capacity_is_enomem_then_a_fresh_handle_succeeds(oracle):
    cfg = ModelConfig(**live_model.MODELS["nofaults_111"])
    with LivenessChecker(cfg, "CleansUpProperly", max_states=4096) as lc:
        with pytest.raises(kubecheck.KubecheckError) as e:
            lc.run()
        assert e.value.code == -12 and "max_states = 4096" in str(e.value)
        with pytest.raises(kubecheck.KubecheckError):
            lc.alive()                   # no completed run
    with LivenessChecker(cfg, "CleansUpProperly") as lc:
        r = lc.run()
    assert (r.states, r.edges, r.live_states, r.violated) == (8203, 17018, 427, True)
    # the smallest capacity that holds the graph
    with LivenessChecker(cfg, "CleansUpProperly", max_states=8203) as lc:
        assert lc.run().live_states == 427
    with LivenessChecker(cfg, "CleansUpProperly", max_states=8202) as lc:
        with pytest.raises(kubecheck.KubecheckError) as e:
            lc.run()
        assert e.value.code == -12


def test_assert_during_build_gives_no_verdict(oracle):
    m = live_model.Model(oracle, nc=2, np=0, ns=1)
    assert m.assert_action == "C4"
    with LivenessChecker(ModelConfig(nc=2, np=0), "SomeActorRestarts") as lc:
        r = lc.run()
    assert (r.error, r.error_action) == ("assertion", "C4") and r.error_self in (0, 1)
    assert (r.violated, r.kind, r.trace_len, r.live_states, r.rounds) == (False, None, 0, 0, 0)


def _cli(cfg_name):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tla-kubernetes_amd"))
    p = subprocess.run([sys.executable, "-m", "kubecheck.tlc", "-tool", "-config",
                        os.path.join(ROOT, "models", cfg_name), "MC"],
                       capture_output=True, text=True, env=env, timeout=300)
    codes = [int(c) for c in re.findall(r"@!@!@STARTMSG (\d+):\d+ @!@!@", p.stdout)]
    return p, codes


def test_cli_liveness_cfg():
    p, codes = _cli("Liveness.cfg")
    assert p.returncode == 13, p.stderr
    plain, plain_codes = _cli("Model_1.cfg")
    assert plain.returncode == 0, plain.stderr
    assert 2116 not in plain_codes and 2192 not in plain_codes
    # the BFS block is the one of the plain run; its 2186 closes the output
    assert "577736 states generated, 163408 distinct states found, 0 states left on queue." in p.stdout
    assert "The depth of the complete state graph search is 124." in p.stdout
    assert "No error has been found" in p.stdout
    assert codes[:len(plain_codes) - 1] == plain_codes[:-1] and codes[-1] == plain_codes[-1] == 2186
    tail = codes[len(plain_codes) - 1:-1]
    # the first property is violated and ends the run
    assert tail[:3] == [2192, 2116, 2264] and codes.count(2116) == 1 and codes.count(2192) == 1
    assert "Checking temporal property ReconcileCompletes" in p.stdout
    assert set(tail[3:-1]) == {2217} and tail[-1] in (2122, 2218)
    n = len(tail) - 4
    last = re.search(r"STARTMSG (2122|2218):4 @!@!@\n(\d+): (Back to state (\d+)|Stuttering)\n", p.stdout)
    assert last and int(last.group(2)) == n + 1
    if last.group(4):
        assert 1 <= int(last.group(4)) <= n
