"""Simulation mode on the GPU against the independent model of
tests/sim_model.py (the RNG in plain Python, successors from the CPU oracle):
every walk's end, length and final state, the totals, the reported error and
its replayed trace.  Expected values are computed by the model in the test.

distinct_visited counts 63-bit fingerprints and the model counts exact states;
at these sizes (under 1e5 states) the chance that the two differ by a
fingerprint collision is about n^2 / 2^64 ~ 1e-9."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kubecheck
from kubecheck import ModelConfig, Simulator

import sim_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS = ("assertion", "invariant", "deadlock")


def _key(flags):
    return tuple(sorted(flags.items()))


@functools.lru_cache(maxsize=None)
def _model(key):
    import pyoracle

    pyoracle.lib()
    return sim_model.Model(pyoracle, **dict(key))


@functools.lru_cache(maxsize=None)
def _expected(key, seed, num_walks, depth):
    """The model's run, computed once per case and shared (never modified)."""
    return _model(key).run(seed, num_walks, depth)


def expected(flags, seed, num_walks, depth):
    return _expected(_key(flags), seed, num_walks, depth)


def run_gpu(flags, seed, num_walks, depth, **kw):
    with Simulator(ModelConfig(**flags), seed=seed, num_walks=num_walks, depth=depth, **kw) as sim:
        res = sim.run()
        kind, length, final = sim.walks()
    return res, kind, length, final


def check_walks(want, kind, length, final):
    assert len(kind) == len(want.walks)
    assert [int(k) for k in kind] == [sim_model.KINDS[w.kind] for w in want.walks]
    assert [int(n) for n in length] == [w.length for w in want.walks]
    exp = np.array([w.states[-1] for w in want.walks], dtype=np.uint64)
    bad = np.nonzero((final != exp).any(axis=1))[0]
    assert bad.size == 0, f"final states differ for walks {bad[:8]}"


def check_totals(want, res, distinct=False):
    assert res.steps == want.steps
    assert res.act_steps == want.act_steps
    assert (res.walks_error, res.walks_depth, res.walks_terminated) == \
        (want.walks_error, want.walks_depth, want.walks_terminated)
    if distinct:
        assert res.distinct_visited == len(want.visited)


def check_error(want, res):
    if want.error_walk is None:
        assert res.error is None and res.trace_len == 0 and res.trace == []
        return
    wk = want.walks[want.error_walk]
    assert res.error == wk.kind
    assert res.error_walk == want.error_walk and res.trace_len == wk.length
    if wk.kind == "assertion":
        assert res.error_action == wk.info and res.error_invariant is None
    elif wk.kind == "invariant":
        assert res.error_invariant == wk.info and res.error_action is None
    else:
        assert res.error_action is None and res.error_invariant is None


def check_trace(flags, want, res):
    """The replayed trace of the reported walk, validated through the oracle
    alone: an oracle Init state, then the oracle successor at the model's chosen
    index at every step, and a last state that shows the error."""
    model = _model(_key(flags))
    wk = want.walks[res.error_walk]
    trace = [tuple(s) for s in res.trace]
    assert len(trace) == res.trace_len == wk.length
    assert trace[0] in model.init
    assert res.trace_actions[0] is None
    for i, t in enumerate(wk.choices):
        succ, fail = model.successors(trace[i])
        assert fail is None and model.invariant(trace[i]) is None
        assert succ[t] == (res.trace_actions[i + 1], trace[i + 1])
    succ, fail = model.successors(trace[-1])
    if res.error == "assertion":
        assert succ is None and fail == res.error_action
    elif res.error == "deadlock":
        assert succ == [] and model.invariant(trace[-1]) is None
    else:
        assert model.invariant(trace[-1]) == res.error_invariant
    assert re.findall(r"^State (\d+):$", res.trace_text, flags=re.M) == [str(i + 1) for i in range(len(trace))]


# ---- 1. Model_1, 1024 walks x depth 128, seed 1, count_distinct
def test_model1_walks_and_totals():
    want = expected({}, 1, 1024, 128)
    res, kind, length, final = run_gpu({}, 1, 1024, 128, count_distinct=True)
    print("steps", res.steps, "distinct", res.distinct_visited, "kernel_ms", res.kernel_ms)
    check_walks(want, kind, length, final)
    check_totals(want, res, distinct=True)
    assert want.steps == 1024 * 127 and want.walks_error == 0     # the case: no walk of Model_1 errs
    check_error(want, res)
    assert res.launches == 4 and res.kernel_ms > 0 and res.seconds > 0


# ---- 2. launch-geometry invariance
@pytest.mark.parametrize("spl", [1, 7, 0])
def test_steps_per_launch_does_not_change_the_result(spl):
    want = expected({}, 1, 1024, 128)
    res, kind, length, final = run_gpu({}, 1, 1024, 128, count_distinct=True, steps_per_launch=spl)
    check_walks(want, kind, length, final)
    check_totals(want, res, distinct=True)
    check_error(want, res)
    assert res.launches == {1: 128, 7: 19, 0: 4}[spl]


@pytest.mark.parametrize("num_walks", [1, 257, 1000])
def test_ragged_walk_counts(num_walks):
    # a single lane, a ragged last wave, a ragged last workgroup
    want = expected({}, 1, num_walks, 128)
    res, kind, length, final = run_gpu({}, 1, num_walks, 128, count_distinct=True)
    check_walks(want, kind, length, final)
    check_totals(want, res, distinct=True)
    # a walk does not depend on how many walks there are
    full = expected({}, 1, 1024, 128)
    assert [w.states[-1] for w in want.walks] == [w.states[-1] for w in full.walks[:num_walks]]


# ---- 3. errors
ERROR_CASES = [
    (dict(nc=2), 512, 64, "assertion", "C4"),
    (dict(variant=2), 512, 128, "invariant", "OnlyOneVersion"),
    (dict(variant=1, invariants=7), 512, 128, "invariant", "NoLostUpdate"),
    (dict(np=2, variant=1, invariants=7), 512, 128, "invariant", "NoLostUpdate"),
    (dict(variant=4), 512, 64, "invariant", "TypeOK"),
    (dict(variant=5), 64, 8, "invariant", "OnlyOneVersion"),
    (dict(ns=0), 256, 32, "deadlock", None),
]


@pytest.mark.parametrize("flags,num_walks,depth,kind,info", ERROR_CASES, ids=[str(c[0]) for c in ERROR_CASES])
def test_errors(flags, num_walks, depth, kind, info):
    want = expected(flags, 1, num_walks, depth)
    assert want.walks_error >= 1                       # the case's condition: the model found an error walk
    assert want.walks[want.error_walk].kind == kind and want.walks[want.error_walk].info == info
    if flags == dict(variant=5):                       # Init violates OnlyOneVersion: every walk errs at once
        assert all(w.kind == "invariant" and w.length == 1 for w in want.walks)
    res, kinds, length, final = run_gpu(flags, 1, num_walks, depth, count_distinct=True)
    print(flags, "error walks", res.walks_error, "reported", res.error_walk, "len", res.trace_len)
    check_walks(want, kinds, length, final)
    check_totals(want, res, distinct=True)
    check_error(want, res)
    check_trace(flags, want, res)


def test_no_deadlock_check_means_termination():
    flags = dict(ns=0, check_deadlock=False)
    want = expected(flags, 1, 256, 32)
    assert want.walks_error == 0 and want.walks_terminated >= 1
    res, kinds, length, final = run_gpu(flags, 1, 256, 32)
    check_walks(want, kinds, length, final)
    check_totals(want, res)
    check_error(want, res)
    assert res.distinct_visited == 0                   # not counted unless asked


# ---- 4. stop_on_error
def test_stop_on_error_reports_the_same_error():
    flags = dict(nc=2)
    want = expected(flags, 1, 512, 64)
    with Simulator(ModelConfig(**flags), seed=1, num_walks=512, depth=64, stop_on_error=True,
                   steps_per_launch=8) as sim:
        res = sim.run()
        kinds, length, _ = sim.walks()
        running = sim.trace(int(np.nonzero(kinds == 0)[0][0]))   # a walk stopped early still replays
    check_error(want, res)
    check_trace(flags, want, res)
    assert res.steps <= want.steps
    # the walks advance in lock-step: launches of 8 steps until the shortest error (14 states) is met
    first = want.walks[want.error_walk].length
    assert res.launches == -(-first // 8)
    assert int(length.max()) == 8 * res.launches + 1 and len(running[0]) == int(length.max())
    full = run_gpu(flags, 1, 512, 64)[0]
    assert (full.error, full.error_walk, full.trace_len, full.trace) == \
        (res.error, res.error_walk, res.trace_len, res.trace)


# ---- 5. seed
def test_seed_changes_the_walks():
    want = expected({}, 2, 128, 64)
    res, kind, length, final = run_gpu({}, 2, 128, 64, count_distinct=True)
    check_walks(want, kind, length, final)
    check_totals(want, res, distinct=True)
    other = expected({}, 1, 128, 64)
    assert any(a.states[-1] != b.states[-1] for a, b in zip(want.walks, other.walks))


# ---- 6. wider states
def test_np2_walks_and_distinct():
    flags = dict(np=2)
    want = expected(flags, 1, 1024, 128)
    res, kind, length, final = run_gpu(flags, 1, 1024, 128, count_distinct=True)
    check_walks(want, kind, length, final)
    check_totals(want, res, distinct=True)
    check_error(want, res)


@pytest.mark.parametrize("flags", [dict(nc=2, np=2), dict(np=3)], ids=str)
def test_four_actor_models(flags):
    # four actors: more state words and the second objs word
    want = expected(flags, 1, 256, 32)
    res, kind, length, final = run_gpu(flags, 1, 256, 32, count_distinct=True)
    check_walks(want, kind, length, final)
    check_totals(want, res, distinct=True)
    check_error(want, res)
    if res.error is not None:
        check_trace(flags, want, res)


# ---- a second run of one Simulator starts afresh
def test_rerun_is_identical():
    with Simulator(ModelConfig(nc=2), seed=1, num_walks=512, depth=64, count_distinct=True) as sim:
        a, b = sim.run(), sim.run()
    assert (a.steps, a.act_steps, a.walks_error, a.distinct_visited, a.error_walk, a.trace) == \
        (b.steps, b.act_steps, b.walks_error, b.distinct_visited, b.error_walk, b.trace)
    check_totals(expected(dict(nc=2), 1, 512, 64), b, distinct=True)


# ---- 7. CLI end to end
def test_cli_simulate_reports_assertion_trace():
    want = expected(dict(nc=2), 1, 512, 64)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tla-kubernetes_amd"))
    p = subprocess.run([sys.executable, "-m", "kubecheck.tlc", "-tool", "-simulate", "num=512", "-depth", "64",
                        "-seed", "1", "-nc", "2", "-config", os.path.join(ROOT, "models", "Model_1.cfg"), "MC"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 12, p.stderr
    assert "Assert evaluated to FALSE (action C4)" in p.stdout
    assert p.stdout.count("STARTMSG 2217:4") == want.walks[want.error_walk].length
    assert "seed 1" in p.stdout and "512 behaviors" in p.stdout and "64 states" in p.stdout
