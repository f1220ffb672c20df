"""The table-driven label lowering on the GPU: k_claim's per-actor generated
counters, the rebuild's action of a run-time slot, the select-only plan and
its Assert position, on the wide deferred path, where all of them run.

Model_1 is narrower than the narrow-kernel threshold, so chunk_states forces
its levels onto the wide path (k_claim with the deferred rebuild); 512
parents per chunk also gives the widest levels several chunks."""
import pytest

from kubecheck import ModelChecker, ModelConfig

pytestmark = pytest.mark.gpu

CHUNK = 512


def run(**kw):
    with ModelChecker(ModelConfig(**kw)) as mc:
        return mc.run()


@pytest.mark.parametrize("first_claim", [False, True])
def test_model1_wide_deferred(fixtures, mcout, first_claim):
    fx = fixtures["model1"]
    r = run(chunk_states=CHUNK, first_claim=first_claim)
    assert r.claim_mode == ("first" if first_claim else "minimum")
    assert r.deferred_states > 0 and not r.defer_fallback and r.narrow_levels == 0
    assert r.complete and r.error is None
    assert (r.generated, r.distinct, r.depth) == (577736, 163408, 124)
    assert r.level_width == fx["level_width"]
    assert r.act_gen == fx["act_gen"] == mcout["act_gen"]
    if first_claim:
        assert sum(r.act_dist.values()) + r.init == r.distinct
    else:
        assert r.act_dist == fx["act_dist"]          # the rebuild's action of every new state


def test_two_clients_first_claim(oracle, fixtures):
    """Two actors of one kind: the per-actor merge of the generated counters."""
    fx = fixtures["nc2"]
    r = run(nc=2, chunk_states=CHUNK, first_claim=True)
    assert (r.error, r.error_action, r.error_level) == ("assertion", "C4", fx["err_level"])
    assert r.level_width == fx["level_width"] and r.trace_len == fx["trace_len"]
    # the levels before the Assert, against the oracle stopped at the same level
    levels = fx["err_level"] - 1
    ref = oracle.run(oracle.config(2, 1, 1, max_levels=levels))
    r = run(nc=2, chunk_states=CHUNK, first_claim=True, max_levels=levels)
    assert r.deferred_states > 0 and r.error is None
    assert r.level_width == ref["level_width"] == fx["level_width"][:levels]
    assert (r.generated, r.distinct) == (ref["generated"], ref["distinct"])
    assert r.act_gen == ref["act_gen"]


def test_two_controllers_first_claim(fixtures):
    """NP=2 (the benchmark's model), its first 40 levels; the fixture is the oracle's run."""
    fx = fixtures["np2_40levels"]
    r = run(np=2, max_levels=40, first_claim=True)
    assert r.claim_mode == "first" and r.deferred_states > 0 and not r.defer_fallback
    assert (r.generated, r.distinct, r.depth) == (fx["generated"], fx["distinct"], fx["depth"])
    assert r.level_width == fx["level_width"]
    assert r.act_gen == fx["act_gen"]
    assert sum(r.act_dist.values()) + r.init == r.distinct


@pytest.mark.parametrize("key,variant,error,what", [("variant3", 3, "assertion", "C2"),
                                                    ("variant2", 2, "invariant", "OnlyOneVersion")])
def test_seeded_errors_wide_deferred(fixtures, key, variant, error, what):
    """The C2 Assert (the plan's fail_pos and fail_slot) and the invariant bug
    on the wide deferred path: the fixture's level and trace length."""
    fx = fixtures[key]
    r = run(variant=variant, chunk_states=CHUNK)
    assert r.error == error and not r.complete
    assert (r.error_action if error == "assertion" else r.error_invariant) == what
    assert (r.error_level, r.trace_len) == (fx["err_level"], fx["trace_len"])
    assert [list(map(int, t)) for t in r.trace] == fx["trace"]
