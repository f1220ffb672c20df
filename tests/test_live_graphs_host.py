"""The made graphs of tests/live_graphs.py and the graph-generic host models
without a GPU: every family instance obeys kc_live_selftest's input rules,
fair_check's SCCs equal a brute-force decomposition by reachability matrix, the
Jacobi simulation of the launch schedule ends with fair_check's F and L and
eliminate's rounds, the random instances have the structure they were chosen
for, and kc_live_selftest answers -EINVAL to each kind of bad input."""
import numpy as np
import pytest

import kubecheck

import fair_model
import live_graphs
import live_model

SYNTHETIC = live_graphs.synthetic()
IDS = [g.name for g in SYNTHETIC]


def test_names_are_unique():
    assert len(set(IDS)) == len(IDS)
    assert len({c for c in live_graphs.RANDOM_CASES}) == len(live_graphs.RANDOM_CASES) == 12


@pytest.mark.parametrize("g", SYNTHETIC, ids=IDS)
def test_family_instance_is_valid_input(g):
    live_graphs.validate(g)


def brute_sccs(succ, S):
    """The SCCs of more than one state of the subgraph S induces, by the
    transitive closure of its adjacency matrix (self-loops dropped)."""
    nodes = sorted(S)
    at = {v: k for k, v in enumerate(nodes)}
    m = len(nodes)
    R = np.zeros((m, m), dtype=bool)
    for v in nodes:
        for w in succ[v]:
            if w in at and w != v:
                R[at[v], at[w]] = True
    for k in range(m):                       # Warshall
        R |= np.outer(R[:, k], R[k, :])
    both = R & R.T
    seen, out = set(), []
    for k in range(m):
        if k in seen or not both[k, k]:
            continue
        comp = {k} | set(np.flatnonzero(both[k]).tolist())
        seen |= comp
        out.append(sorted(nodes[j] for j in comp))
    return sorted(out)


@pytest.mark.parametrize("g", [g for g in SYNTHETIC if g.n <= 64], ids=[g.name for g in SYNTHETIC if g.n <= 64])
def test_sccs_equal_brute_force(g):
    want = live_graphs.reference(g).fair
    assert sorted(sorted(c) for c in want.sccs) == brute_sccs(g.succ, g.S)
    if "classes" in g.note:
        assert sorted(sorted(c) for c in want.sccs) == sorted(g.note["classes"])


@pytest.mark.parametrize("g", SYNTHETIC, ids=IDS)
def test_jacobi_schedule_ends_with_the_models_answer(g):
    ref = live_graphs.reference(g)
    s = ref.schedule
    assert s.fair == ref.fair.fair and s.live == ref.fair.live
    assert s.trim_rounds == ref.next_rounds
    assert 1 <= s.launches <= 4096
    # the labels: the largest member of each class, NONE outside what the trim leaves
    cls = {i: top for c in ref.fair.sccs for top in [max(c)] for i in c}
    for i in range(g.n):
        assert s.comp[i] == (cls.get(i, i) if i in ref.next_live else fair_model.NONE)
    # what each case was built to show
    for key, got in (("fair", ref.fair.fair), ("live", ref.fair.live), ("terminal", ref.fair.terminal & g.S)):
        if key in g.note:
            assert got == g.note[key], key
    if "enabled" in g.note:
        assert {i: ref.fair.enabled[i] for i in g.note["enabled"]} == g.note["enabled"]
    if "outer" in g.note:
        assert s.outer_rounds == g.note["outer"] and len(ref.fair.sccs) == g.note["sccs"]
    assert ref.fair.live <= ref.next_live          # per-process fairness only ever removes behaviours


@pytest.mark.parametrize("case", live_graphs.RANDOM_CASES, ids=[f"{n}-P{P}-s{s}" for n, P, s in live_graphs.RANDOM_CASES])
def test_random_instance(case):
    g = live_graphs.cached_random(*case)
    live_graphs.validate(g)
    assert g.n > case[0] * 0.8 and g.nproc == case[1]
    ref = live_graphs.reference(g)
    # chosen for: an SCC of more than 64 states, and one of more than one state that is not fair
    assert max(len(c) for c in ref.fair.sccs) > 64 and len(ref.fair.fair_sccs) < len(ref.fair.sccs)
    s = ref.schedule
    assert s.fair == ref.fair.fair and s.live == ref.fair.live and s.trim_rounds == ref.next_rounds
    assert 1 <= s.launches <= 4096


def test_check_lasso_graph_rejects_a_cycle_without_a_witness():
    g = next(x for x in SYNTHETIC if x.name == "lasso-witness-closes")
    want = live_graphs.reference(g).fair
    fair_model.check_lasso_graph(g.succ, g.procs, g.nproc, g.level, want, [0, 1, 2, 3, 4], 2, "back-to-state", 1)
    with pytest.raises(AssertionError):      # not a step of the graph
        fair_model.check_lasso_graph(g.succ, g.procs, g.nproc, g.level, want, [0, 1, 3, 4], 2, "back-to-state", 1)
    h = next(x for x in SYNTHETIC if x.name == "lasso-far-witnesses")
    want = live_graphs.reference(h).fair
    ring = [0] + list(range(1, 41))
    with pytest.raises(AssertionError):      # the plain ring never takes a step of processes 1 .. 3
        fair_model.check_lasso_graph(h.succ, h.procs, h.nproc, h.level, want, ring, 2, "back-to-state", 1)
    w = next(x for x in SYNTHETIC if x.name == "walk-into-cycle")
    ref = live_graphs.reference(w)
    live_model.check_next_lasso(w.succ, w.level, w.S, ref.next_live, [0, 1, 2, 3, 4], 2, "back-to-state", 2)
    with pytest.raises(AssertionError):      # 4 has no edge to 1
        live_model.check_next_lasso(w.succ, w.level, w.S, ref.next_live, [0, 1, 2, 3, 4], 2, "back-to-state", 1)


@pytest.mark.parametrize("name", list(live_model.MODELS))
def test_edge_process_by_pc_equals_the_models_rule(oracle, name):
    """The rule tests/test_gpu_fairness.py applies to Model_1's exported graph
    (no action names there) names the same process as fair_model.edge_process
    on every edge of the small models."""
    m = live_model.model(oracle, name)
    src = [i for i in range(len(m.states)) for _ in m.succ[i]]
    dst = [j for i in range(len(m.states)) for j in m.succ[i]]
    want = [p for row in fair_model.procs_of(m) for p in row]
    assert len(want) == m.edges
    got = fair_model.edge_process_by_pc(np.array(m.states, dtype=np.uint64), src, dst, m.nc + m.np)
    assert got.tolist() == want
    assert m.ns == 1 or m.nc + m.np not in want     # (without a server nothing is the server's step)


# ---- kc_live_selftest's input rules: one bad input per rule, -EINVAL with or without a GPU

def _bad_inputs():
    g = live_graphs.hub_form("bad-base", 5, [(1, 2, 0), (2, 3, 1), (3, 1, 0), (3, 4, 1)], 2)
    n = g.n

    def words(**kw):
        w = dict(zip(("deg", "edges", "eproc", "stay", "parent", "level"), (x.copy() for x in g.words())))
        for k, (i, v) in kw.items():
            w[k][i] = v
        return tuple(w.values())

    good = [n, 2, 1, 0, 5]
    yield "n-zero", words(), [0, 2, 1, 0, 5]
    yield "P-zero", words(), [n, 0, 1, 0, 5]
    yield "P-nine", words(), [n, 9, 1, 0, 5]
    yield "fairness-two", words(), [n, 2, 2, 0, 5]
    yield "path-cap-below-n-under-next", words(), [n, 2, 0, n - 1, 5]
    yield "par-short", words(), good[:4]
    yield "target-not-a-state", words(edges=(0, n)), good
    yield "process-not-below-P", words(eproc=(0, 2)), good
    yield "degrees-sum-above-ne", words(deg=(1, 2)), good
    yield "degrees-sum-below-ne", words(deg=(3, 1)), good
    yield "stay-two", words(stay=(1, 2)), good
    yield "level-starts-at-2", words(level=(0, 2)), good
    yield "level-falls", words(level=(2, 3)), good
    yield "init-with-parent", words(parent=(0, 0)), good
    yield "parent-not-smaller", words(parent=(2, 2)), good
    yield "parent-on-wrong-level", words(parent=(2, 1)), good
    yield "no-edge-from-parent", words(level=(4, 3), parent=(4, 1)), good
    yield "level-1-after-level-2-parentless", words(level=(4, 1)), good


BAD = list(_bad_inputs())


@pytest.mark.parametrize("name,words,par", BAD, ids=[b[0] for b in BAD])
def test_selftest_rejects_bad_input(name, words, par):
    lib = kubecheck.load()
    g = live_graphs.hub_form("bad-base", 5, [(1, 2, 0), (2, 3, 1), (3, 1, 0), (3, 4, 1)], 2)
    r = live_graphs.selftest(lib, g, 1, words=words, par=par)
    assert r.rc == -22, lib.kc_last_error()
    assert b"kc_live_selftest" in lib.kc_last_error() and r.guards_ok


def test_selftest_good_input_needs_a_gpu_or_runs():
    lib = kubecheck.load()
    g = live_graphs.hub_form("bad-base", 5, [(1, 2, 0), (2, 3, 1), (3, 1, 0), (3, 4, 1)], 2)
    for fairness in (0, 1):
        r = live_graphs.selftest(lib, g, fairness)
        assert r.rc == (0 if kubecheck.device_count() > 0 else -19), lib.kc_last_error()
    # ne < 2^31 and the section sizes are checked before any device call too
    assert lib.kc_live_selftest(None, 0, None, None, 0, None, None, None, None, None, 0, None, 0) == -22
    r = live_graphs.selftest(lib, g, 1, path_cap=3)               # a path buffer the lasso will not fit
    assert r.rc == (0 if kubecheck.device_count() > 0 else -19)
    r = live_graphs.selftest(lib, g, 1, par=[g.n, 2, 1, 3, 5])    # ... and out not sized for it
    assert r.rc == -22
