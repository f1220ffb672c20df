"""Construction and destruction of everything in the library that owns a
device, pinned, stream or event handle.

Every such handle is a member of its holder (csrc/owned.h: DeviceArray,
PinnedArray, OwnedStream, OwnedEvent) and is released when the holder closes;
the seen-set tier (csrc/engine_spill.h SeenSpill) owns its arena.  What no
other test does: build, run and close the same configuration several times
in one process, and close a holder whose setup or run stopped half-way (the
seen-set budget check fails after the hot table and the arena are allocated;
a liveness graph overflows its buffers; an FPSet names a device that is not
there).

The checker cases are Model_1 (163,408 states, 124 levels); every run must
give the golden counts and level widths (tests/golden/oracle_fixtures.json,
model1).  The plugin cases (FPSet, StateQueue, Simulator, LivenessChecker,
the cold tier through its selftest harness) must give the same answers on
every round.  Nothing here looks at the device's free memory: the machines
are shared."""
import os

import numpy as np
import pytest
import torch

import cold_model as cm
from kubecheck import FPSet, KubecheckError, LivenessChecker, ModelChecker, ModelConfig, Simulator, StateQueue
from kubecheck.distributed import NativeShardedChecker
from test_gpu_coldset import Both, full_check, split

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


# ------------------------------------------------------------------ the plugins
STRESS_SEED = 0x5EED0000


def test_fpset_create_use_close_repeated():
    # 1,000 puts, checkFPs (four temporaries), stress (three events), close;
    # and a set that starts at 96 slots and takes 4,096 puts 256 at a time.
    # DevFpset::reserve grows past 3/4 load to land at <= 1/2, doubling from
    # 12 buckets: 768, 1,536, 3,072 and 6,144 slots, four rehashes
    fps = np.arange(1, 4097, dtype=np.uint64) * np.uint64(7919)
    for k in range(ROUNDS):
        with FPSet(1 << 14) as s:
            assert not s.put_batch(fps[:1000]).any(), f"round {k}"
            assert s.put_batch(fps[:1000]).all()
            s.checkFPs()
            assert s.min_gap == 7919
            ti, tl, found = s.stress(STRESS_SEED, 4096, 1024, 4096)
            # (the stress stream is a bijection's: distinct, and none is a small multiple of 7919)
            assert (s.size(), found) == (1000 + 4096, 2048) and ti > 0 and tl > 0
        with FPSet(64) as s:
            caps = [s.capacity()]
            for at in range(0, 4096, 256):
                assert not s.put_batch(fps[at:at + 256]).any(), f"round {k}"
                caps.append(s.capacity())
            assert sorted(set(caps)) == [96, 768, 1536, 3072, 6144]
            assert s.size() == 4096 and s.contains_batch(fps).all()
            assert not s.contains_batch(fps + np.uint64(1)).any()


def test_fpset_bad_device_then_a_fresh_one():
    with pytest.raises(KubecheckError) as e:
        FPSet(device=10 ** 6)
    assert e.value.code == -22 and "bad device" in str(e.value)
    with FPSet() as s:
        assert not s.put_batch(np.array([3, 5], dtype=np.uint64)).any() and s.size() == 2


def test_state_queue_spill_and_close_repeated(tmp_path):
    # tests/test_gpu_squeue.py::test_fifo_through_all_tiers' queue: 3 segments
    # of HBM, 4 of host RAM, the rest in files; 12 segments go in
    W, SEG = 6, 1000
    seg_b = SEG * W * 8
    a = (np.arange(12 * SEG, dtype=np.uint64)[:, None] * np.uint64(W) + np.arange(W, dtype=np.uint64)[None, :])
    for k in range(ROUNDS):
        q = StateQueue(W, device=0, segment_states=SEG, hbm_bytes=3 * seg_b, host_bytes=4 * seg_b,
                       spill_dir=str(tmp_path))
        for at in range(0, len(a), 1500):
            q.enqueue(a[at:at + 1500])
        st = q.stats()
        assert st["spilled_host_bytes"] > 0 and st["spilled_disk_bytes"] > 0, f"round {k}"
        assert len(os.listdir(tmp_path)) > 0
        # the older half to the host (read from whatever tier holds it), the
        # rest through HBM (host and file segments are loaded back)
        half = len(a) // 2
        assert np.array_equal(q.dequeue(half), a[:half]), f"round {k}"
        out = torch.zeros((len(a) - half, W), dtype=torch.int64, device="cuda")
        assert q.dequeue_dev(out, len(out)) == len(out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), a[half:]), f"round {k}"
        assert q.size() == 0 and q.stats()["reloaded_bytes"] > 0
        q.close()
        assert os.listdir(tmp_path) == []


def _sim(**kw):
    with Simulator(ModelConfig(), seed=1, num_walks=256, depth=32, **kw) as sim:
        r = sim.run()
    return (r.steps, r.act_steps, r.walks_error, r.walks_depth, r.walks_terminated, r.distinct_visited, r.error,
            r.launches, r.fpset_slots)


@pytest.mark.parametrize("count_distinct", [False, True])
def test_simulator_build_run_close_repeated(count_distinct):
    first = _sim(count_distinct=count_distinct)
    assert first[0] == 256 * 31 and (first[5] > 0) == count_distinct      # no walk of Model_1 ends early
    for k in range(1, ROUNDS):
        assert _sim(count_distinct=count_distinct) == first, f"round {k}"


def _live(fairness, **kw):
    # (which lasso the device reports is its choice: the counts are not)
    with LivenessChecker(ModelConfig(), "ReconcileCompletes", fairness=fairness, **kw) as lc:
        r = lc.run()
    return (r.states, r.edges, r.init, r.depth, r.stay_states, r.live_states, r.live_terminal, r.violated,
            r.sccs, r.fair_sccs, r.fair_states)


@pytest.mark.parametrize("fairness", ["next", "process"])
def test_liveness_build_run_close_repeated(fairness):
    first = _live(fairness)
    assert first[:5] == (163408, 577734, 2, 124, 150856) and first[7]
    assert (first[8] > 0) == (fairness == "process")
    for k in range(1, ROUNDS):
        assert _live(fairness) == first, f"round {k}"


@pytest.mark.parametrize("fairness", ["next", "process"])
def test_liveness_close_after_overflow(fairness):
    with pytest.raises(KubecheckError) as e:
        _live(fairness, max_states=4096)
    assert e.value.code == -12 and "max_states = 4096" in str(e.value)
    assert _live(fairness)[0] == 163408


def _cold(tmp_path, case):
    r = cm.rng(53)
    if case == "merge":        # tests/test_gpu_coldset.py::test_tiering: exactly 2/3, one merge
        parts = split(cm.shape_keys("uniform", 40_000, r), (3000, 2000), r)
        b = Both(cache_keys=1)
    else:                      # ...::test_file_tier: one run of two windows, read through the staging buffers
        parts = [cm.shape_keys("uniform", 65, r)]
        b = Both(spill_dir=tmp_path, host_bytes=8, window_keys=64, cache_keys=0)
    with b:
        for p in parts:
            b.add(p)
        full_check(b, np.sort(np.concatenate(parts)), r, slices=False)
        s = b.check_stats()
    assert os.listdir(tmp_path) == []
    return s


@pytest.mark.parametrize("case", ["merge", "file"])
def test_cold_tier_build_use_close_repeated(tmp_path, case):
    first = _cold(tmp_path, case)
    assert (first["merges"], first["runs_disk"]) == ((1, 0) if case == "merge" else (0, 1))
    assert case == "merge" or first["disk_read"] > 0
    for k in range(1, ROUNDS):
        assert _cold(tmp_path, case) == first, f"round {k}"
