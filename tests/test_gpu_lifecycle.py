"""Construction and destruction of the engine and the sharded stages.

Every buffer of EngineT and ShardT is owned by a DeviceArray / PinnedArray
member (csrc/engine_util.h) and freed when the checker closes; the seen-set
tier (csrc/engine_spill.h SeenSpill) owns its arena.  What no other test
does: build, run and close the same configuration several times in one
process, and close a checker whose setup stopped half-way (the seen-set
budget check fails after the hot table and the arena are allocated).

Every case is Model_1 (163,408 states, 124 levels); every run must give the
golden counts and level widths (tests/golden/oracle_fixtures.json, model1).
Nothing here looks at the device's free memory: the machines are shared."""
import pytest

from kubecheck import KubecheckError, ModelChecker, ModelConfig
from kubecheck.distributed import NativeShardedChecker

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
ROUNDS = 6


def _golden(fixtures):
    fx = fixtures["model1"]
    assert (fx["distinct"], fx["generated"], fx["depth"]) == (163408, 577736, 124)
    return (fx["distinct"], fx["generated"], fx["depth"], list(fx["level_width"]))


def _engine(**kw):
    with ModelChecker(ModelConfig(**kw)) as mc:
        r = mc.run()
    return (r.distinct, r.generated, r.depth, list(r.level_width))


def _sharded(**kw):
    mc = NativeShardedChecker(ModelConfig(**kw), emulate=2)
    try:
        r = mc.run()
    finally:
        mc.close()
    return (r["distinct"], r["generated"], r["depth"], list(r["level_width"]))


@pytest.mark.parametrize("name", ["default", "first_claim", "trace_host", "seen_spill", "seen_and_frontier_spill"])
def test_engine_build_run_close_repeated(fixtures, tmp_path, name):
    kw = {
        "default": {},
        "first_claim": dict(first_claim=True),
        "trace_host": dict(trace_host=True),
        "seen_spill": dict(seen_hbm_bytes=4 * MiB),
        # (small segments and a directory, so that the queue really spills
        # past its two budgets, as tests/test_gpu_seenspill.py runs it)
        "seen_and_frontier_spill": dict(seen_hbm_bytes=4 * MiB, frontier_hbm_bytes=48 * KiB,
                                        frontier_host_bytes=64 * KiB, frontier_segment_states=384,
                                        spill_dir=str(tmp_path)),
    }[name]
    want = _golden(fixtures)
    for k in range(ROUNDS):
        assert _engine(**kw) == want, f"round {k}"


@pytest.mark.parametrize("kw", [{}, dict(seen_hbm_bytes=4 * MiB)], ids=["default", "seen_spill"])
def test_sharded_build_run_close_repeated(fixtures, kw):
    want = _golden(fixtures)
    for k in range(ROUNDS):
        assert _sharded(**kw) == want, f"round {k}"


def test_close_after_failed_seen_setup(fixtures):
    # the budget check fails after the hot table and the arena exist; the
    # checker is closed with them, and the next one runs clean
    with pytest.raises(KubecheckError) as e:
        _engine(seen_hbm_bytes=1 * MiB)
    assert "too small" in str(e.value)
    assert _engine() == _golden(fixtures)
