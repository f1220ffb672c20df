"""User-defined invariants end to end on the GPU: the engine
hook against the host model's fixtures (tests/golden/pred_fixtures.json,
written by tools/make_pred_golden.py from tests/pred_model.py), in both claim
modes, on narrow and wide levels, with several chunks, switched off again, and
every refusal."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kubecheck
from kubecheck import KubecheckError, ModelChecker, ModelConfig, pred

import pred_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def rows():
    with open(os.path.join(GOLDEN, "pred_fixtures.json")) as f:
        return json.load(f)["rows"]


def run_row(fx, **extra):
    nc, np_, ns = fx["model"]
    kw = dict(fx["run"])
    kw.update(extra)
    with ModelChecker(ModelConfig(nc=nc, np=np_, ns=ns, **kw), invariants=fx["user"]) as mc:
        return mc.run()


def check_counts(r, fx):
    assert (r.generated, r.distinct, r.depth, r.init) == (fx["generated"], fx["distinct"], fx["depth"], fx["init"])
    assert r.level_width == fx["level_width"]
    assert [u.name for u in r.user_invariants] == list(fx["user"])
    assert {u.name: u.violations for u in r.user_invariants} == fx["violations"]
    assert all(u.states_evaluated == fx["states_evaluated"] for u in r.user_invariants)


def check_violation(r, fx, oracle, deterministic):
    nc, np_, ns = fx["model"]
    assert r.error == "invariant" and r.error_invariant == fx["name"]
    assert r.error_level == fx["err_level"] and r.trace_len == fx["trace_len"] == fx["err_level"]
    assert not r.complete
    check_counts(r, fx)
    # a real behaviour that ends in a violating state
    ast = pred.parse(fx["user"][fx["name"]], nc, np_, ns)
    assert not pred.evaluate(ast, r.trace[-1], nc, np_, ns)
    for k in range(fx["k"]):
        assert pred.evaluate(pred.parse(list(fx["user"].values())[k], nc, np_, ns), r.trace[-1], nc, np_, ns)
    kw = {k: v for k, v in fx["run"].items() if k in ("can_fail", "can_timeout", "variant")}
    cfg = oracle.config(nc, np_, ns, **kw)
    init = [list(map(int, t)) for t in oracle.level_tuples(cfg, 1)]
    assert r.trace[0] in init
    for s, x in zip(r.trace, r.trace[1:]):
        succ, _ = oracle.successors(cfg, np.array(s, dtype=np.uint64))
        assert x in [list(map(int, t)) for _, t in succ]
    if deterministic:
        assert r.trace == fx["trace"]


@pytest.mark.parametrize("first_claim", [False, True])
def test_model1_invariants_that_hold(rows, fixtures, first_claim):
    fx = rows["model1_holds"]
    r = run_row(fx, first_claim=first_claim)
    assert r.error is None and r.complete
    assert (r.generated, r.distinct, r.depth) == (577736, 163408, 124)
    check_counts(r, fx)
    plain = fixtures["model1"]
    assert r.level_width == plain["level_width"] and r.act_gen == plain["act_gen"] and r.act_dist == plain["act_dist"]
    assert r.user_invariants[0].states_evaluated == 163408


VIOLATED_M1 = ["model1_store1", "model1_c4", "model1_c5", "model1_pvcdone", "model1_onepending", "model1_two",
               "c101_c5"]


@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("rid", VIOLATED_M1)
def test_model1_violated(rows, oracle, rid, first_claim):
    fx = rows[rid]
    assert fx["verdict"] == "violated"
    r = run_row(fx, first_claim=first_claim)
    check_violation(r, fx, oracle, deterministic=not first_claim)


@pytest.mark.parametrize("rid", ["model1_store1", "model1_onepending", "model1_pvcdone"])
def test_model1_violated_on_the_wide_path(rows, oracle, rid):
    """chunk_states switches the narrow kernel off: the same levels through launch_chunk / close_level, in chunks."""
    fx = rows[rid]
    r = run_row(fx, chunk_states=256)
    assert r.narrow_levels == 0
    check_violation(r, fx, oracle, deterministic=True)


@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("rid,level,builtin", [("variant2_oov", 22, "variant2"), ("variant5_oov", 1, "variant5")])
def test_parity_with_built_in_only_one_version(rows, fixtures, oracle, rid, level, builtin, first_claim):
    fx = rows[rid]
    assert fx["err_level"] == level
    r = run_row(fx, first_claim=first_claim)
    check_violation(r, fx, oracle, deterministic=not first_claim)
    assert r.trace_len == fixtures[builtin]["trace_len"]
    if not first_claim:
        assert r.trace == fixtures[builtin]["trace"]


@pytest.mark.parametrize("extra", [dict(), dict(first_claim=True), dict(chunk_states=256)])
def test_violation_comes_before_what_its_level_finds(rows, fixtures, oracle, extra):
    """Level 21 of variant 2 holds a violating state and its expansion finds the OnlyOneVersion violation of level 22."""
    fx = rows["variant2_precedence"]
    assert fx["err_level"] == fixtures["variant2"]["err_level"] - 1
    r = run_row(fx, **extra)
    check_violation(r, fx, oracle, deterministic=not extra.get("first_claim"))
    with ModelChecker(ModelConfig(variant=2, **extra)) as mc:          # without it: the built-in error, one level on
        b = mc.run()
    assert b.error_invariant == "OnlyOneVersion" and b.error_level == fx["err_level"] + 1


@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("rid,level,width,bad", [("np2_bothdone", 25, 8801, 2), ("np2_c5_bothdone", 34, 96320, 6)])
def test_np2_wide_levels(rows, oracle, rid, level, width, bad, first_claim):
    fx = rows[rid]
    assert fx["err_level"] == level and fx["level_width"][level - 1] == width
    assert list(fx["violations"].values()) == [bad]
    r = run_row(fx, first_claim=first_claim)
    check_violation(r, fx, oracle, deterministic=not first_claim)
    with ModelChecker(ModelConfig(np=2, max_levels=level + 1, first_claim=first_claim)) as mc:
        plain = mc.run()
    assert r.defer_fallback == plain.defer_fallback


def test_np2_level_in_several_chunks(rows, oracle):
    fx = rows["np2_c5_bothdone"]
    r = run_row(fx, chunk_states=16384)
    assert r.levels_chunks > r.depth + 4             # level 34 alone spans six chunks
    check_violation(r, fx, oracle, deterministic=True)
    with ModelChecker(ModelConfig(np=2, max_levels=35, chunk_states=16384)) as mc:
        plain = mc.run()
    assert r.defer_fallback == plain.defer_fallback


def test_np2_holding_invariant_on_40_levels(fixtures):
    fx = fixtures["np2_40levels"]
    with ModelChecker(ModelConfig(np=2, max_levels=40), invariants={"Holds": pred_model.NP2_HOLDS}) as mc:
        r = mc.run()
    assert r.error is None
    assert (r.distinct, r.generated) == (1716684, 6898316) == (fx["distinct"], fx["generated"])
    assert r.level_width == fx["level_width"] and r.act_gen == fx["act_gen"]
    u, = r.user_invariants
    assert u.violations == 0 and u.states_evaluated == sum(fx["level_width"][:39])


def test_switching_off(rows, fixtures):
    fx = rows["model1_c5"]
    lib = kubecheck.load()
    with ModelChecker(ModelConfig(), invariants=fx["user"]) as mc:
        assert mc.run().error_invariant == "NeverC5"
        mc.set_invariants(None)
        r = mc.run()
        plain = fixtures["model1"]
        assert r.error is None and r.user_invariants == []
        assert (r.generated, r.distinct, r.depth) == (plain["generated"], plain["distinct"], plain["depth"])
        assert r.level_width == plain["level_width"] and r.act_gen == plain["act_gen"]
        out = (C.c_uint64 * 9)()
        assert lib.kc_engine_invariant_stats(mc._h, out, 9) == -22
        assert b"kc_engine_set_invariants" in lib.kc_last_error()
        mc.set_invariants(fx["user"])                # and on again
        assert mc.run().error_level == fx["err_level"]


def test_no_trace_without_keep_trace(rows):
    fx = rows["model1_c5"]
    r = run_row(fx, keep_trace=False)
    assert r.error_invariant == "NeverC5" and r.error_level == fx["err_level"] and r.trace_len == 0


INV = {"X": "Cardinality(apiState) <= 2"}


@pytest.mark.parametrize("cfg,word", [
    (dict(nc=2, symmetry="clients"), "symmetry"),
    (dict(constraint_stored=1), "constraint discards"),
    (dict(action_properties="NoBlindUpdate"), "action properties"),
    (dict(seen_hbm_bytes=1 << 26), "seen_hbm_bytes"),
    (dict(frontier_hbm_bytes=1 << 26), "frontier_hbm_bytes"),
    (dict(trace_host=True), "trace_host"),
])
def test_refused_by_configuration(cfg, word):
    with ModelChecker(ModelConfig(**cfg)) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.set_invariants(INV)
        assert e.value.code == -22 and word in str(e.value)
        assert mc.run().user_invariants == []


def test_refused_with_coverage_both_ways():
    with ModelChecker(ModelConfig(), coverage=True) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.set_invariants(INV)
        assert e.value.code == -22 and "coverage" in str(e.value)
    with ModelChecker(ModelConfig(), invariants=INV) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.set_coverage(True)
        assert e.value.code == -22 and "user invariants" in str(e.value)


def test_refused_with_checkpoint_and_recover(tmp_path):
    with ModelChecker(ModelConfig(), invariants=INV) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.set_checkpoint(str(tmp_path), every_levels=10)
        assert e.value.code == -22 and "user invariants" in str(e.value)
        with pytest.raises(KubecheckError) as e:
            mc.recover(str(tmp_path))
        assert e.value.code == -22 and "user invariants" in str(e.value)
    with ModelChecker(ModelConfig()) as mc:
        mc.set_checkpoint(str(tmp_path), every_levels=10)
        with pytest.raises(KubecheckError) as e:
            mc.set_invariants(INV)
        assert e.value.code == -22 and "checkpoint" in str(e.value)


def test_bad_program_is_refused():
    lib = kubecheck.load()
    with ModelChecker(ModelConfig()) as mc:
        bad = (C.c_uint64 * 2)(pred.P_AND, 0)
        assert lib.kc_engine_set_invariants(mc._h, bad, 1) == -22
        assert b"128 instructions" in lib.kc_last_error()
        assert mc.run().error is None


def test_reach_cfg_message_stream(capsys):
    """models/Reach.cfg through the command line: the violated user invariant prints what a built-in one prints."""
    from kubecheck import tlc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rc = tlc.main(["-config", os.path.join(root, "models", "Reach.cfg"), "-defs", os.path.join(root, "models", "Reach.tla"),
                   "MC"])
    out = capsys.readouterr().out
    assert rc == 12
    assert "Invariant ClientNeverDone is violated." in out and "The behavior up to this point is:" in out
    assert out.count("/\\ pc = (") == 8 and '"Client" :> "C5"' in out       # level 8: a behaviour of 8 states
