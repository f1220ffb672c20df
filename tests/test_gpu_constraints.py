"""Constraints (kc_model_config.constraint_stored, constraint_inflight,
action_constraints) on the GPU: the device hook against the host's
kc_spec_in_model, the engine against the host model's fixtures
(tests/con_model.py, tests/golden/constraint_fixtures.json) in both claim
modes on the narrow path and on the chunked wide path (deferred and
materialising), FIFO level sets, rule 5 (no deadlock by cuts), rule 4 (the
invariants of a discarded successor), the untouched defaults, and the refused
combinations."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import con_model
import kubecheck
import pyoracle
from kubecheck import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "constraint_fixtures.json")))
ROWS = {rid: (model, kw) for rid, model, kw in con_model.ROWS}


def model_kw(model, kw):
    nc, np_, ns = model
    return dict(nc=nc, np=np_, ns=ns, constraint_stored=kw.get("stored_max", -1),
                constraint_inflight=kw.get("inflight_max", -1),
                action_constraints=1 if kw.get("serve_clients_first") else 0)


def run(**kw):
    with kubecheck.ModelChecker(kubecheck.ModelConfig(**kw)) as mc:
        assert mc.instantiation == "constraints"
        return mc.run()


def host_answers(sp, S, X, acts):
    u64 = C.POINTER(C.c_uint64)
    return np.array([sp._lib.kc_spec_in_model(C.byref(sp._c), S[i].ctypes.data_as(u64), X[i].ctypes.data_as(u64),
                                              int(acts[i])) for i in range(len(acts))], dtype=np.int32)


# ------------------------------------------------------------ the device hook
_pairs = {}


def np2_pairs():
    """Every (parent, successor, action) of the (1,2,1) StoredAtMost1 +
    ServeClientsFirst run (48,050), computed once."""
    if not _pairs:
        chunks = []
        model, kw = ROWS["np2_stored1_serve"]
        con_model.run(*model, on_pairs=lambda *c: chunks.append(c), **kw)
        for k, name in enumerate(("S", "X", "acts", "cuts")):
            _pairs[name] = np.concatenate([c[k] for c in chunks])
    return _pairs


def test_device_hook_equals_host_np2_every_pair():
    p = np2_pairs()
    assert len(p["acts"]) == 48050 - 2
    sp = kubecheck.Spec(kubecheck.ModelConfig(**model_kw(*ROWS["np2_stored1_serve"])))
    got = sp.con_selftest(p["S"], p["X"], p["acts"])
    assert np.array_equal(got, host_answers(sp, p["S"], p["X"], p["acts"]))
    assert np.array_equal(got, p["cuts"])
    assert (int((got == 1).sum()), int((got == 2).sum())) == (363, 220)


def test_device_hook_equals_host_model1_every_pair():
    model, kw = ROWS["model1_inflight1"]
    sp = kubecheck.Spec(kubecheck.ModelConfig(**model_kw(model, kw)))
    n = [0, 0]

    def on_pairs(S, X, acts, cuts):
        got = sp.con_selftest(S, X, acts)
        assert np.array_equal(got, host_answers(sp, S, X, acts))
        assert np.array_equal(got, cuts)
        n[0] += len(acts)
        n[1] += int((got == 1).sum())

    con_model.run(*model, on_pairs=on_pairs, pair_chunk=1 << 16, **kw)
    assert n == [575716 - 2, 6442]


def test_device_hook_at_the_bounds():
    """Pairs whose successor holds exactly k and k + 1 objects / pending
    requests, for every k the (1,2,1) run's pairs reach, under the bound k;
    among them pairs where the pending actor is the last one (its list mask is
    in the second objs word of the packed state)."""
    p = np2_pairs()
    X = p["X"]
    A = range(3)
    st = np.array([con_model.stored(x) for x in X])
    pend = np.array([len(con_model.pending_requests(x, A)) + len(con_model.pending_lists(x, A)) for x in X])
    last = np.array([2 in con_model.pending_lists(x, A) or 2 in con_model.pending_requests(x, A) for x in X])
    assert st.max() >= 2 and pend.max() >= 2 and last.any()
    assert any(2 in con_model.pending_lists(x, A) for x in X[last])
    for field, vals in (("constraint_stored", st), ("constraint_inflight", pend)):
        for k in range(0, int(vals.max())):
            idx = np.concatenate([np.flatnonzero(vals == k)[:300], np.flatnonzero(vals == k + 1)[:300],
                                  np.flatnonzero(last & (vals == k))[:100], np.flatnonzero(last & (vals == k + 1))[:100]])
            sp = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2, ns=1, **{field: k}))
            got = sp.con_selftest(p["S"][idx], X[idx], p["acts"][idx])
            assert np.array_equal(got, host_answers(sp, p["S"][idx], X[idx], p["acts"][idx]))
            assert np.array_equal(got, (vals[idx] > k).astype(np.int32))
            assert set(got.tolist()) == {0, 1}


# The other two models built with constraints, capped: the device hook on
# every pair, and the engine in both claim modes, against the host model.
OTHER_MODELS = [((2, 1, 1), dict(stored_max=1, inflight_max=2, serve_clients_first=True), 10),
                ((1, 3, 1), dict(stored_max=1, inflight_max=2, serve_clients_first=True), 12)]


@pytest.mark.parametrize("model,kw,max_levels", OTHER_MODELS)
def test_other_models_hook_and_engine(model, kw, max_levels):
    sp = kubecheck.Spec(kubecheck.ModelConfig(**model_kw(model, kw)))
    chunks = []
    want = con_model.run(*model, max_levels=max_levels, on_pairs=lambda *c: chunks.append(c), **kw)
    S, X, acts, cuts = (np.concatenate([c[k] for c in chunks]) for k in range(4))
    got = sp.con_selftest(S, X, acts)
    assert np.array_equal(got, cuts) and np.array_equal(got, host_answers(sp, S, X, acts))
    assert want["error"] is None and want["cut_state"] > 0 and want["cut_action"] > 0
    for first_claim in (False, True):
        r = run(first_claim=first_claim, max_levels=max_levels, **model_kw(model, kw))
        assert r.error is None and not r.complete
        assert (r.generated, r.distinct, r.depth) == (want["generated"], want["distinct"], want["depth"])
        assert r.level_width == want["level_width"] and r.act_gen == want["act_gen"]
        assert (r.cut_state, r.cut_action) == (want["cut_state"], want["cut_action"])
        if not first_claim:
            assert r.act_dist == want["act_dist"]


# -------------------------------------------------------- engine vs fixtures
def check_row(r, fx, first_claim):
    assert r.error is None and r.complete
    assert (r.generated, r.distinct, r.depth) == (fx["generated"], fx["distinct"], fx["depth"])
    assert r.level_width == fx["level_width"]
    assert (r.cut_state, r.cut_action) == (fx["cut_state"], fx["cut_action"])
    assert r.act_gen == fx["act_gen"]
    if first_claim:
        assert sum(r.act_dist.values()) == sum(fx["act_dist"].values())
    else:
        assert r.act_dist == fx["act_dist"]
    # the new-states-per-parent histogram: every distinct state was expanded,
    # and only the in-model new states are counted (no parent of these runs
    # reaches the last, open-ended bin)
    assert sum(r.outdeg_hist) == r.distinct and r.outdeg_hist[15] == 0
    assert sum(i * n for i, n in enumerate(r.outdeg_hist)) == r.distinct - r.init


@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("rid", sorted(ROWS))
def test_engine_equals_fixture(rid, first_claim):
    r = run(first_claim=first_claim, **model_kw(*ROWS[rid]))
    check_row(r, FIX["rows"][rid], first_claim)
    if ROWS[rid][0] == (1, 1, 1):
        assert r.narrow_levels == r.depth          # Model_1 runs wholly on narrow levels


@pytest.mark.parametrize("defer", ["1", "0"])
@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("rid", ["np2_stored1", "model1_inflight1", "np2_stored1_serve"])
def test_engine_wide_chunked_equals_fixture(monkeypatch, rid, first_claim, defer):
    # chunk_states turns the narrow kernel off: every level runs the wide
    # k_claim, the widest in several chunks (663 / 3,937 parents in chunks of
    # 256), on the deferred frontier or with the materialising emit
    monkeypatch.setenv("KC_DEFER", defer)
    r = run(first_claim=first_claim, chunk_states=256, **model_kw(*ROWS[rid]))
    check_row(r, FIX["rows"][rid], first_claim)
    assert r.narrow_levels == 0 and r.levels_chunks > r.depth
    assert (r.deferred_states > 0) == (defer == "1")
    assert r.claim_mode == ("first" if first_claim else "minimum")


# ------------------------------------------------------------ FIFO level sets
@pytest.mark.parametrize("chunk_states", [0, 256])
def test_fifo_levels_equal_host_model(chunk_states):
    rid = con_model.LEVELS_ROW
    model, kw = ROWS[rid]
    levels = sorted(int(L) for L in FIX["rows"][rid]["levels"])
    want = con_model.run(*model, keep_levels=levels, **kw)["levels"]
    with kubecheck.ModelChecker(kubecheck.ModelConfig(chunk_states=chunk_states, **model_kw(model, kw))) as mc:
        for L in levels:
            mc.capture_level(L)
            r = mc.run()
            assert r.error is None and r.distinct == FIX["rows"][rid]["distinct"]
            got = mc.level_tuples(L)
            assert got.shape == want[L].shape and got.tobytes() == want[L].tobytes(), L
            assert con_model._sha(got) == FIX["rows"][rid]["levels"][str(L)]["sha256"]


# ------------------------------------------------------------------ rule 5
@pytest.mark.parametrize("chunk_states", [0, 256])
def test_frontier_dying_by_cuts_is_no_deadlock(chunk_states):
    r = run(check_deadlock=True, chunk_states=chunk_states, **model_kw(*ROWS["model1_inflight0"]))
    assert r.error is None and r.complete and r.queue_left == 0
    check_row(r, FIX["rows"]["model1_inflight0"], False)


# ------------------------------------------------------------------ rule 4
@pytest.mark.parametrize("defer", ["1", "0"])
@pytest.mark.parametrize("chunk_states", [0, 256])
@pytest.mark.parametrize("first_claim", [False, True])
def test_invariant_of_a_discarded_successor(monkeypatch, first_claim, chunk_states, defer):
    """Seeded variant 2 under StoredAtMost2 (the smallest bound with a
    violation, see the fixture's note): the violating state holds three
    objects, so it is outside the constraint and only the check made where it
    is discarded can find it."""
    monkeypatch.setenv("KC_DEFER", defer)
    fx = FIX["rule4"]
    nc, np_, ns = fx["model"]
    r = run(nc=nc, np=np_, ns=ns, variant=fx["variant"], constraint_stored=fx["stored_max"],
            first_claim=first_claim, chunk_states=chunk_states)
    assert r.error == "invariant" and r.error_invariant == "OnlyOneVersion"
    assert r.trace_len == fx["trace_len"] == len(r.trace) and r.error_level == fx["trace_len"]
    st = [con_model.stored(np.array(t, dtype=np.uint64)) for t in r.trace]
    assert max(st[:-1]) <= fx["stored_max"] < st[-1]
    cfg = pyoracle.config(nc, np_, ns, variant=fx["variant"])
    init = [t.tobytes() for t in pyoracle.level_tuples(cfg, 1)]
    assert np.array(r.trace[0], dtype=np.uint64).tobytes() in init
    for a, b in zip(r.trace, r.trace[1:]):
        succ, _ = pyoracle.successors(cfg, np.array(a, dtype=np.uint64))
        assert np.array(b, dtype=np.uint64).tobytes() in [x.tobytes() for _, x in succ]
    assert con_model.violated(np.array(r.trace[-1], dtype=np.uint64), nc, np_) == 1
    if not first_claim:
        assert [list(map(int, t)) for t in r.trace] == fx["trace"]


def test_invariant_of_a_discarded_init_state():
    # variant 5's Init store holds two Secret versions: under StoredAtMost1
    # both Init states are outside the constraint, and still checked
    want = con_model.run(1, 1, 1, variant=5, stored_max=1)
    assert want["error"]["invariant"] == 1 and want["error"]["trace_len"] == 1
    assert want["distinct"] == 0
    r = run(variant=5, constraint_stored=1)
    assert r.error == "invariant" and r.error_invariant == "OnlyOneVersion"
    assert (r.trace_len, r.error_level, r.distinct, r.init) == (1, 1, 0, 2)
    assert np.array(r.trace[0], dtype=np.uint64).tobytes() == want["error"]["trace"][0].tobytes()
    # under StoredAtMost2 the same Init states are inside the model: the
    # violation is reported as without a constraint, the kept Init states counted
    want = con_model.run(1, 1, 1, variant=5, stored_max=2)
    assert want["error"]["trace_len"] == 1 and want["distinct"] == 2
    r = run(variant=5, constraint_stored=2)
    plain = kubecheck.ModelChecker(kubecheck.ModelConfig(variant=5))
    with plain:
        p = plain.run()
    assert r.error == p.error == "invariant" and r.error_invariant == p.error_invariant == "OnlyOneVersion"
    assert (r.trace_len, r.error_level, r.distinct, r.init, r.depth, r.level_width) == \
        (p.trace_len, p.error_level, p.distinct, p.init, p.depth, p.level_width) == (1, 1, 2, 2, 1, [2])
    assert r.trace == p.trace and (r.cut_state, r.cut_action) == (0, 0)
    # no invariant to violate: both are discarded and the run is over
    r = run(variant=5, constraint_stored=1, invariants=0)
    assert r.error is None and r.complete
    assert (r.generated, r.distinct, r.depth, r.cut_state, r.level_width) == (2, 0, 0, 2, [])


# ---------------------------------------------------------------- defaults
def test_defaults_run_the_plain_instantiation():
    with kubecheck.ModelChecker(kubecheck.ModelConfig()) as mc:
        assert mc.instantiation == "plain"
        r = mc.run()
    assert (r.generated, r.distinct, r.depth) == (577736, 163408, 124)
    assert (r.cut_state, r.cut_action) == (0, 0) and r.error is None
    with kubecheck.ModelChecker(kubecheck.ModelConfig(np=2, symmetry="controllers", max_levels=3)) as mc:
        assert mc.instantiation == "symmetry"


# --------------------------------------------------------- the command line
def test_cli_constraint_cfg(tmp_path):
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tla-kubernetes_amd"))
    cmd = [sys.executable, "-m", "kubecheck.tlc", "-tool", "-config"]
    p = subprocess.run(cmd + [os.path.join(ROOT, "models", "Constraint.cfg")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    fx = FIX["rows"]["model1_inflight1"]
    assert f"{fx['generated']} states generated, {fx['distinct']} distinct states found, 0 states left on queue." in p.stdout
    assert f"The depth of the complete state graph search is {fx['depth']}." in p.stdout
    banner = p.stdout.split("@!@!@STARTMSG 2187:0 @!@!@\n")[1].split("\n")[0]
    assert banner.endswith(f"Constraints: InFlightAtMost1 ({fx['cut_state']} generated states discarded by a state "
                           "constraint, 0 by an action constraint).")
    # a refused combination: exit 1 with the reason, nothing run
    p = subprocess.run(cmd + [os.path.join(ROOT, "models", "Constraint.cfg"), "-coverage"], capture_output=True,
                       text=True, env=env, timeout=300)
    assert p.returncode == 1 and p.stdout == ""
    assert p.stderr.startswith("Error: CONSTRAINT / ACTION_CONSTRAINT (InFlightAtMost1) with -coverage") and \
        "Traceback" not in p.stderr


# ---------------------------------------------------------------- refusals
CON = dict(constraint_stored=1)


@pytest.mark.parametrize("kw,needle", [
    (dict(np=2, symmetry="controllers", **CON), "symmetry"),
    (dict(seen_hbm_bytes=1 << 26, **CON), "seen_hbm_bytes"),
    (dict(frontier_hbm_bytes=1 << 26, **CON), "frontier_hbm_bytes"),
    (dict(trace_host=True, **CON), "trace_host"),
    (dict(nc=2, np=2, **CON), "with constraints"),
    (dict(constraint_inflight=0, np=2, symmetry=2), "symmetry"),
    (dict(action_constraints=1, seen_hbm_bytes=1 << 26), "seen_hbm_bytes"),
])
def test_engine_create_refusals(kw, needle):
    with pytest.raises(kubecheck.KubecheckError) as e:
        kubecheck.ModelChecker(kubecheck.ModelConfig(**kw))
    assert e.value.code == -22 and needle in str(e.value)


def test_engine_create_refuses_unknown_action_bits():
    c = kubecheck.ModelConfig().to_c()
    c.action_constraints = 2
    h = C.c_void_p()
    assert kubecheck.load().kc_engine_create(C.byref(c), C.byref(h)) == -22
    assert b"action_constraints" in kubecheck.load().kc_last_error()


def test_coverage_and_checkpoint_refusals(tmp_path):
    with kubecheck.ModelChecker(kubecheck.ModelConfig(max_levels=5, **CON)) as mc:
        for call in (lambda: mc.set_coverage(True), lambda: mc.set_checkpoint(str(tmp_path), every_levels=2),
                     lambda: mc.recover(str(tmp_path))):
            with pytest.raises(kubecheck.KubecheckError) as e:
                call()
            assert e.value.code == -22 and "constraints" in str(e.value)
        r = mc.run()
        assert r.error is None and not r.complete and r.queue_left > 0
        with pytest.raises(kubecheck.KubecheckError) as e:
            mc.checkpoint(str(tmp_path))
        assert e.value.code == -22 and "constraints" in str(e.value)


@pytest.mark.parametrize("con", [CON, dict(constraint_inflight=2), dict(action_constraints=1)])
def test_other_entry_points_refuse(con):
    lib = kubecheck.load()
    cfg = kubecheck.ModelConfig(**con)
    c = cfg.to_c()
    h = C.c_void_p()
    assert lib.kc_shard_create(C.byref(c), 0, 1, C.byref(h)) == -22
    assert b"constraints" in lib.kc_last_error() and not h.value
    with pytest.raises(kubecheck.KubecheckError) as e:
        kubecheck.Simulator(cfg, seed=1, num_walks=4, depth=4)
    assert e.value.code == -22 and "constraints" in str(e.value)
    with pytest.raises(kubecheck.KubecheckError) as e:
        kubecheck.LivenessChecker(cfg, "ReconcileCompletes")
    assert e.value.code == -22 and "constraints" in str(e.value)
