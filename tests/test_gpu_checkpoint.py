"""Checkpoint and recover on the GPU (kc_engine_checkpoint / _recover /
_set_checkpoint): a run cut at a level top, written out, and taken up by a new
engine reports what the uninterrupted run reports.  The reference is always
the uninterrupted run of the same config and the oracle's fixtures, and the
file is read back through the independent reader of tests/ckpt_model.py."""
import os

import numpy as np
import pytest

import ckpt_model as cm
import kubecheck
from kubecheck import KubecheckError, ModelChecker, ModelConfig, checkpoint_info

pytestmark = pytest.mark.gpu

CUMULATIVE = ("init", "generated", "distinct", "depth", "level_width", "act_gen", "act_dist", "outdeg_hist",
              "peak_frontier", "complete", "error")


def run(**kw):
    with ModelChecker(ModelConfig(**kw)) as mc:
        return mc.run()


def write_at(d, stop, stage_bytes=0, **kw):
    """Run to the top of level `stop`, checkpoint into d; the stopped run's result."""
    with ModelChecker(ModelConfig(max_levels=stop, **kw)) as mc:
        r = mc.run()
        assert r.error is None and r.queue_left > 0 and not r.complete and r.depth == stop
        if stage_bytes:
            mc.set_checkpoint(None, stage_bytes=stage_bytes)
        mc.checkpoint(str(d))
    return r


def resume(d, stage_bytes=0, fps=False, **kw):
    """A new engine, recover from d, run; (result, check_fps min gap or None)."""
    with ModelChecker(ModelConfig(**kw)) as mc:
        if stage_bytes:
            mc.set_checkpoint(None, stage_bytes=stage_bytes)
        mc.recover(str(d))
        r = mc.run()
        return (r, mc.check_fps()[0]) if fps else r


def same(a, b, keys=CUMULATIVE):
    for k in keys:
        assert getattr(a, k) == getattr(b, k), k
    assert a.collision_optimistic == b.collision_optimistic


@pytest.fixture(scope="module")
def model1():
    with ModelChecker(ModelConfig()) as mc:
        r = mc.run()
        return r, mc.check_fps()[0]


# ---- Model_1, deterministic: stopped at its first, a middle and its last level
@pytest.mark.parametrize("stop", [1, 30, 124])
def test_model1_stopped_and_recovered(tmp_path, model1, fixtures, mcout, stop):
    whole, gap = model1
    fx = fixtures["model1"]
    part = write_at(tmp_path, stop)
    assert part.level_width == fx["level_width"][:stop]
    r, rgap = resume(tmp_path, fps=True)
    assert (r.init, r.generated, r.distinct, r.queue_left, r.depth) == (
        mcout["init"], mcout["generated"], mcout["distinct"], mcout["queue_left"], mcout["depth"])
    assert r.complete and r.error is None and r.depth == 124
    assert r.level_width == fx["level_width"] and r.act_gen == fx["act_gen"] == mcout["act_gen"]
    assert r.act_dist == fx["act_dist"]
    assert r.outdeg_hist == whole.outdeg_hist == fx["outdeg_hist"]
    same(r, whole)
    assert rgap == gap                      # the seen-set is the same set
    # (stop = 124: the recovered run expands the last level, which yields nothing new)


def test_file_against_the_oracle(tmp_path, oracle, fixtures):
    fx = fixtures["model1"]
    write_at(tmp_path, 30)
    ck = cm.read(tmp_path)
    sp = kubecheck.Spec(ModelConfig())
    cfg = oracle.config()
    levels = [oracle.level_tuples(cfg, L) for L in range(1, 31)]
    assert [len(x) for x in levels] == fx["level_width"][:30]
    # FRONTIER: level 30's states, packed, in the oracle's (FIFO) order
    want = [int(w) for t in levels[29] for w in sp.pack(t)]
    assert ck.frontier == want
    # FPS: the fingerprints of levels 1..30, as a set
    fps = {sp.fingerprint(t) for lv in levels for t in lv}
    assert len(ck.fps) == len(fps) == sum(fx["level_width"][:30]) and set(ck.fps) == fps
    # the header's counts: the fixture's prefix sums
    assert ck.level == ck.nlevels == 30 and ck.level_width == fx["level_width"][:30]
    assert ck.n == fx["level_width"][29] and ck.level_gidx == sum(fx["level_width"][:29])
    assert ck.distinct == sum(fx["level_width"][:30]) and ck.init == fx["init"]
    # (the widest level so far: the narrow path counts the level it stops at, the wide path does not)
    assert ck.peak_frontier in (max(fx["level_width"][:29]), max(fx["level_width"][:30]))
    assert ck.state_words == sp.state_words and ck.keep_trace == 1 and ck.claim_mode == 0
    assert (ck.nc, ck.np, ck.ns, ck.variant, ck.invariants, ck.symmetry) == (1, 1, 1, 0, 3, 0)
    # cand: the frontier's successors, by the oracle
    assert ck.cand == sum(len(oracle.successors(cfg, t)[0]) for t in levels[29])
    # the trace file: Init states have no parent, every other parent is in the level before
    starts = np.cumsum([0] + fx["level_width"][:30])
    assert ck.parent[:2] == [cm.M64] * 2
    for L in range(1, 30):
        assert all(starts[L - 1] <= p < starts[L] for p in ck.parent[starts[L]:starts[L + 1]]), L
    # and the library's own reader agrees with the independent one
    info = checkpoint_info(str(tmp_path))
    assert (info.level, info.n, info.cand, info.distinct) == (ck.level, ck.n, ck.cand, ck.distinct)
    assert info.sections["FPS"]["bytes"] == 8 * len(fps)


def test_two_hops_equal_one_run(tmp_path, model1):
    whole, gap = model1
    write_at(tmp_path, 20)
    with ModelChecker(ModelConfig(max_levels=70)) as mc:
        mc.recover(str(tmp_path))
        mid = mc.run()
        assert mid.depth == 70 and mid.queue_left > 0 and mid.level_width == whole.level_width[:70]
        mc.checkpoint(str(tmp_path))
        assert checkpoint_info(str(tmp_path)).level == 70
        # a later run without a new recover() starts from Init as always
        again = mc.run()
        assert again.depth == 70 and again.level_width == mid.level_width and again.generated == mid.generated
    r, rgap = resume(tmp_path, fps=True)
    same(r, whole)
    assert rgap == gap


# ---- wide paths: multi-chunk levels and rehash, and single-chunk wide levels
# on the deferred and the materialising frontier; recovered with other chunks
# and once into a large table
@pytest.mark.parametrize("defer", ["1", "0"])
@pytest.mark.parametrize("wkw,rkw", [(dict(chunk_states=256, fpset_slots=64), dict(chunk_states=1 << 20)),
                                      (dict(chunk_states=1 << 20), dict(chunk_states=256, fpset_slots=64)),
                                      (dict(chunk_states=1 << 20), dict(chunk_states=512, fpset_slots=1 << 22)),
                                      (dict(chunk_states=256, fpset_slots=64), dict())])
def test_wide_paths(tmp_path, model1, monkeypatch, defer, wkw, rkw):
    monkeypatch.setenv("KC_DEFER", defer)
    whole, gap = model1
    part = write_at(tmp_path, 40, **wkw)
    assert part.level_width == whole.level_width[:40]
    r, rgap = resume(tmp_path, fps=True, **rkw)
    same(r, whole)
    assert rgap == gap
    if rkw.get("fpset_slots", 0) >= 1 << 22:
        assert r.fpset_slots == 1 << 22
    elif rkw.get("fpset_slots") == 64:
        assert r.fpset_slots > 64


# ---- a naturally wide model: NP=2 cut at level 30 (35,224 states, the next
# level 45,945; wider than the narrow path takes since level 25), continued to 40
def test_np2_wide_levels_and_small_stage(tmp_path, fixtures):
    fx = fixtures["np2_40levels"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    part = write_at(a, 30, np=2)
    assert part.level_width == fx["level_width"][:30] and part.level_width[29] == 35224
    r = resume(a, np=2, max_levels=40)
    assert r.level_width == fx["level_width"] and r.act_gen == fx["act_gen"] and r.act_dist == fx["act_dist"]
    assert r.generated == fx["generated"] and r.distinct == fx["distinct"] and not r.complete
    # 4-KiB staging buffers: the FPS section crosses many windows and both buffers
    write_at(b, 30, stage_bytes=4096, np=2)
    assert os.path.getsize(cm.path(a)) == os.path.getsize(cm.path(b))
    ca, cb = cm.read(a), cm.read(b)
    assert len(ca.fps) == sum(fx["level_width"][:30]) and set(ca.fps) == set(cb.fps) and len(set(cb.fps)) == len(cb.fps)
    assert ca.frontier == cb.frontier and ca.parent == cb.parent and ca.ord == cb.ord
    assert (ca.level_width, ca.act_gen, ca.act_dist, ca.outdeg) == (cb.level_width, cb.act_gen, cb.act_dist, cb.outdeg)
    r = resume(b, stage_bytes=4096, np=2, max_levels=40)
    assert r.level_width == fx["level_width"] and r.act_gen == fx["act_gen"] and r.act_dist == fx["act_dist"]


# ---- across claim modes: the seen-set travels as bare fingerprints
@pytest.mark.parametrize("w_first,r_first", [(False, True), (True, False)])
def test_np2_across_claim_modes(tmp_path, fixtures, w_first, r_first):
    fx = fixtures["np2_40levels"]
    part = write_at(tmp_path, 30, np=2, first_claim=w_first)
    assert part.claim_mode == ("first" if w_first else "minimum")
    assert checkpoint_info(str(tmp_path)).claim_mode == part.claim_mode
    r = resume(tmp_path, np=2, max_levels=40, first_claim=r_first)
    assert r.claim_mode == ("first" if r_first else "minimum")
    assert (r.distinct, r.generated) == (fx["distinct"], fx["generated"])
    assert r.level_width == fx["level_width"] and r.act_gen == fx["act_gen"]
    assert sum(r.act_dist.values()) + r.init == r.distinct


def test_model1_first_claim_to_first_claim(tmp_path, model1):
    whole, gap = model1
    write_at(tmp_path, 40, chunk_states=1 << 20, first_claim=True)
    r, rgap = resume(tmp_path, fps=True, chunk_states=1 << 20, first_claim=True)
    assert r.claim_mode == "first" and r.complete
    same(r, whole, keys=("init", "generated", "distinct", "depth", "level_width", "act_gen", "peak_frontier"))
    assert sum(r.act_dist.values()) + r.init == r.distinct
    assert rgap == gap


# ---- errors after a recovery: the fixture's trace, state for state
ERRORS = [("nc2", dict(nc=2), 5, "assertion"), ("variant2", dict(variant=2), 11, "invariant"),
          ("ns0", dict(ns=0), 2, "deadlock"),
          ("np2_variant1_lost_update", dict(np=2, variant=1, invariants=7), 12, "invariant")]


@pytest.mark.parametrize("chunk", [0, 1 << 20])
@pytest.mark.parametrize("key,kw,stop,kind", ERRORS)
def test_errors_after_recovery(tmp_path, fixtures, key, kw, stop, kind, chunk):
    fx = fixtures[key]
    write_at(tmp_path, stop, chunk_states=chunk, **kw)
    r = resume(tmp_path, chunk_states=chunk, **kw)
    assert r.error == kind
    assert (r.error_level, r.trace_len) == (fx.get("err_level") or fx["trace_len"], fx["trace_len"])
    assert [list(map(int, t)) for t in r.trace] == fx["trace"]
    k = min(len(r.level_width), len(fx["level_width"]))
    assert k >= stop and r.level_width[:k] == fx["level_width"][:k]
    if fx.get("err_action"):
        assert r.error_action == fx["err_action"] and r.error_self == fx["err_self"]


def test_first_claim_error_after_recovery(tmp_path, fixtures, oracle):
    fx = fixtures["variant3"]
    write_at(tmp_path, 12, chunk_states=1 << 20, variant=3, first_claim=True)
    r = resume(tmp_path, chunk_states=1 << 20, variant=3, first_claim=True)
    assert r.error == "assertion" and (r.error_level, r.trace_len) == (fx["err_level"], fx["trace_len"])
    cfg = oracle.config(variant=3)
    trace = [list(map(int, t)) for t in r.trace]
    assert tuple(trace[0]) in {tuple(map(int, t)) for t in oracle.level_tuples(cfg, 1)}
    for a, b in zip(trace, trace[1:]):
        assert any(list(map(int, x)) == b for _, x in oracle.successors(cfg, a)[0])


# ---- run()'s own checkpoints
@pytest.mark.parametrize("chunk", [0, 1 << 20])
def test_periodic_checkpoints(tmp_path, model1, chunk):
    whole, gap = model1
    with ModelChecker(ModelConfig(chunk_states=chunk)) as mc:
        mc.set_checkpoint(str(tmp_path), every_levels=10)
        r = mc.run()
        same(r, whole)                       # materialising at the checkpoint levels changes no count
        assert mc.check_fps()[0] == gap
        # off again: the next run writes nothing
        os.remove(cm.path(tmp_path))
        mc.set_checkpoint(None)
        same(mc.run(), whole)
        assert not os.path.exists(cm.path(tmp_path))
        mc.set_checkpoint(str(tmp_path), every_levels=10)
        mc.run()
    info = checkpoint_info(str(tmp_path))
    assert info.level == 121 and info.n == whole.level_width[120]
    assert not os.path.exists(cm.path(tmp_path) + ".tmp")
    ck = cm.read(tmp_path)
    assert ck.level_width == whole.level_width[:121]
    r, rgap = resume(tmp_path, fps=True, chunk_states=chunk)
    same(r, whole)
    assert rgap == gap
    # a recovered run counts its periods from the recovered level: 121 + 2 = 123
    with ModelChecker(ModelConfig(chunk_states=chunk)) as mc:
        mc.recover(str(tmp_path))
        mc.set_checkpoint(str(tmp_path), every_levels=2)
        same(mc.run(), whole)
    assert checkpoint_info(str(tmp_path)).level == 123


def test_checkpoint_by_time(tmp_path, model1):
    whole, _ = model1
    # every level on the wide path, so the host sees every level top; due at each
    with ModelChecker(ModelConfig(chunk_states=1 << 20)) as mc:
        mc.set_checkpoint(str(tmp_path), every_seconds=1e-9)
        same(mc.run(), whole)
    assert checkpoint_info(str(tmp_path)).level == 124
    same(resume(tmp_path), whole)


# ---- keep_trace = False
def test_without_trace(tmp_path, model1):
    whole, gap = model1
    write_at(tmp_path, 30, keep_trace=False)
    info = checkpoint_info(str(tmp_path))
    assert not info.keep_trace and set(info.sections) == {"COUNTERS", "FRONTIER", "FPS"}
    assert cm.read(tmp_path).parent is None
    r, rgap = resume(tmp_path, fps=True, keep_trace=False)
    same(r, whole)
    assert rgap == gap
    with ModelChecker(ModelConfig(keep_trace=True)) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.recover(str(tmp_path))
        assert e.value.code == -22 and "keep_trace" in str(e.value)
        same(mc.run(), whole)               # nothing was armed
    # the reverse is fine: the trace sections are skipped
    write_at(tmp_path, 30, keep_trace=True)
    same(resume(tmp_path, keep_trace=False), whole)


# ---- symmetry: the effective mask is part of the model's identity
def test_symmetry(tmp_path):
    kw = dict(np=2, symmetry="controllers")
    whole = run(max_levels=40, **kw)
    part = write_at(tmp_path, 30, **kw)
    assert part.level_width == whole.level_width[:30]
    assert checkpoint_info(str(tmp_path)).symmetry == 2
    r = resume(tmp_path, max_levels=40, **kw)
    same(r, whole, keys=("init", "generated", "distinct", "depth", "level_width", "act_gen", "act_dist",
                         "outdeg_hist", "peak_frontier"))
    with ModelChecker(ModelConfig(np=2)) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.recover(str(tmp_path))
        assert e.value.code == -22 and "symmetry = 2" in str(e.value)


# ---- refusals
def test_refusals(tmp_path):
    d = str(tmp_path)
    with ModelChecker(ModelConfig()) as mc:
        # nothing to checkpoint: no run yet, a complete run
        with pytest.raises(KubecheckError) as e:
            mc.checkpoint(d)
        assert e.value.code == -22 and "did not stop at max_levels" in str(e.value)
        mc.run()
        with pytest.raises(KubecheckError) as e:
            mc.checkpoint(d)
        assert e.value.code == -22
        with pytest.raises(KubecheckError) as e:
            mc.recover(d)
        assert e.value.code == -2           # no file
        with pytest.raises(KubecheckError) as e:
            mc.set_checkpoint(d, every_levels=5, stage_bytes=100)
        assert e.value.code == -22 and "stage_bytes" in str(e.value)
    # a run that ended in an error leaves nothing to checkpoint
    with ModelChecker(ModelConfig(nc=2, max_levels=20)) as mc:
        assert mc.run().error == "assertion"
        with pytest.raises(KubecheckError) as e:
            mc.checkpoint(d)
        assert e.value.code == -22
    write_at(tmp_path, 10)
    # another model: the first differing field is named
    for kw, what in ((dict(nc=2), "nc = 1"), (dict(variant=2), "variant = 0"), (dict(can_fail=False), "can_fail = 1"),
                     (dict(invariants=1), "invariants = 3"), (dict(check_deadlock=False), "check_deadlock = 1")):
        with ModelChecker(ModelConfig(**kw)) as mc:
            with pytest.raises(KubecheckError) as e:
                mc.recover(d)
            assert e.value.code == -22 and what in str(e.value), kw
    # the spill tiers, the host trace and coverage
    for kw in (dict(seen_hbm_bytes=4 << 20), dict(frontier_hbm_bytes=32 << 10, frontier_segment_states=256),
               dict(trace_host=True)):
        with ModelChecker(ModelConfig(max_levels=10, **kw)) as mc:
            mc.run()
            for call in (lambda: mc.checkpoint(d), lambda: mc.recover(d),
                         lambda: mc.set_checkpoint(d, every_levels=3)):
                with pytest.raises(KubecheckError) as e:
                    call()
                assert e.value.code == -22 and "seen_hbm_bytes, frontier_hbm_bytes or trace_host" in str(e.value)
    with ModelChecker(ModelConfig(max_levels=10), coverage=True) as mc:
        mc.run()
        for call in (lambda: mc.checkpoint(d), lambda: mc.recover(d), lambda: mc.set_checkpoint(d, every_levels=3)):
            with pytest.raises(KubecheckError) as e:
                call()
            assert e.value.code == -22 and "coverage" in str(e.value)
    with ModelChecker(ModelConfig()) as mc:
        mc.set_checkpoint(d, every_levels=3)
        with pytest.raises(KubecheckError) as e:
            mc.set_coverage(True)
        assert e.value.code == -22 and "checkpoint" in str(e.value)
    # a damaged file: -EIO at recover(), and the engine still runs from Init
    image = bytearray(open(cm.path(d), "rb").read())
    image[len(image) // 2] ^= 0x10
    open(cm.path(d), "wb").write(bytes(image))
    with ModelChecker(ModelConfig(max_levels=12)) as mc:
        with pytest.raises(KubecheckError) as e:
            mc.recover(d)
        assert e.value.code == -5
        assert mc.run().depth == 12


# ---- the command line: -checkpointlevels / -metadir, then -recover
def test_cli_checkpoint_and_recover(tmp_path, capsys, mcout):
    from kubecheck import tlc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = os.path.join(root, "models", "Model_1.cfg")
    meta = str(tmp_path / "meta")
    assert tlc.main(["-tool", "-nocheckfps", "-config", cfg, "-checkpointlevels", "50", "-metadir", meta, "MC"]) == 0
    out = capsys.readouterr().out
    assert "@!@!@STARTMSG 2195" in out and f"Checkpointing of run {meta}" in out and "@!@!@STARTMSG 2196" in out
    assert "2197" not in out and "Finished computing initial states: 2 distinct" in out
    assert checkpoint_info(meta).level == 101
    assert tlc.main(["-tool", "-nocheckfps", "-config", cfg, "-recover", meta, "MC"]) == 0
    out = capsys.readouterr().out
    info = checkpoint_info(meta)
    assert f"Starting recovery from checkpoint {meta}/" in out
    assert f"Recovery completed. {info.distinct} states examined. {info.n} states on queue." in out
    assert "Computing initial states" not in out and "2195" not in out
    assert f"{mcout['generated']} states generated, {mcout['distinct']} distinct states found, 0 states left" in out
    assert f"The depth of the complete state graph search is {mcout['depth']}." in out
    # no checkpoint there: an error, not a run from Init
    assert tlc.main(["-config", cfg, "-recover", str(tmp_path / "none"), "MC"]) == 1
    assert "Error" in capsys.readouterr().err
