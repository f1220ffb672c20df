"""claim_model.py against a brute-force reading of the oracle, and the host-side
validation of kc_claim_selftest (no GPU: bad input answers -EINVAL before any
device is looked for, good input -ENODEV on a machine without one)."""
import errno

import numpy as np
import pytest

import claim_model as cm
import emit_model as em
import kubecheck

U64 = np.uint64


def level_setup(oracle, np_, lv):
    ocfg = oracle.config(np_=np_)
    spec = kubecheck.Spec(kubecheck.ModelConfig(np=np_))
    older = {}
    for k in range(1, lv + 1):
        for t in oracle.level_tuples(ocfg, k):
            older[t.tobytes()] = k
    return spec, cm.Frontier(spec, oracle.level_tuples(ocfg, lv)), older, oracle.level_tuples(ocfg, lv + 1)


@pytest.mark.parametrize("np_,lv", [(1, 22), (1, 41), (2, 12)])
def test_exact_model_is_the_oracles_next_level(oracle, np_, lv):
    """With every earlier state pre-loaded, the copies the model calls new are
    the oracle's next level, each at its first discoverer in BFS order."""
    spec, fr, older, nxt = level_setup(oracle, np_, lv)
    for own in (False, True):
        fp = spec.fingerprint_own if own else spec.fingerprint
        preload = {fp(np.frombuffer(t, dtype=U64)): cm.make_claim(k, 7) for t, k in older.items()}
        assert len(preload) == len(older)
        world = 3 if own else 1
        masks = [0] * fr.n
        for rank in range(world):
            m, final, probes = cm.exact(fr, preload, lv + 1, base=0, rank=rank, world=world)
            assert all(a & b == 0 for a, b in zip(masks, m))
            masks = [a | b for a, b in zip(masks, m)]
            assert set(final) - set(preload) == {fr.parent(i).succ[t][3 if own else 2]
                                                 for i, w in enumerate(m) for t in em.bits(w)}
        level = em.SpecLevel(spec, np.array([p.tuple for p in fr.block]))
        want = em.first_discoverer_masks(level, set(older))
        assert masks == want
        assert sum(cm.popcount(w) for w in masks) == len(nxt)
        new = {fr.parent(i).succ[t][1].tobytes() for i, w in enumerate(masks) for t in em.bits(w)}
        assert new == {t.tobytes() for t in nxt}
        cm.check_first(fr, set(preload), masks, own)          # the exact answer is one of the first-claim answers


def test_model_claims_bases_and_same_level_preloads(oracle):
    """A same-level claim of a smaller key stays and wins; a larger one (another
    rank's) is displaced; the key carries base."""
    spec, fr, _, _ = level_setup(oracle, 1, 22)
    fps = sorted(fr.fps())
    small = {fps[0]: cm.make_claim(9, 3 << 8 | 1)}                         # parent 3 < base
    large = {fps[1]: cm.make_claim(9, 1 << cm.RANK_SHIFT | 5)}
    mask, final, _ = cm.exact(fr, {**small, **large}, 9, base=1000)
    assert final[fps[0]] == small[fps[0]]
    i, t = next((i, t) for i, t, fp, _ in fr.copies() if fp == fps[1])
    assert final[fps[1]] == cm.make_claim(9, (1000 + i) << 8 | t) and (mask[i] >> t) & 1
    assert not any((mask[i] >> t) & 1 for i, t, fp, _ in fr.copies() if fp == fps[0])
    assert sum(cm.popcount(w) for w in mask) == len(fps) - 1


def test_model_err_key_and_act_gen(oracle, fixtures):
    ocfg = oracle.config(variant=3)
    ref = oracle.run(ocfg)
    assert ref["err_kind"] == 1 and ref["err_level"] == fixtures["variant3"]["err_level"]
    spec = kubecheck.Spec(kubecheck.ModelConfig(variant=3))
    fr = cm.Frontier(spec, oracle.level_tuples(ocfg, ref["err_level"]))
    bad = [i for i in range(fr.n) if fr.parent(i).fail_pos is not None]
    assert bad
    p = fr.parent(bad[0])
    assert fr.err_key(10, 1) == (10 + bad[0]) << 16 | p.fail_pos << 8 | 1
    assert len(p.succ) == p.fail_pos and fr.err_key(10, 0) == fr.err_key(10, 1)
    assert sum(fr.act_gen()) == fr.total()


# ------------------------------------------------------------------ validation
def call(oracle, kind=cm.K_EXACT, np_=1, **kw):
    cfg = kubecheck.ModelConfig(np=np_)
    spec = kubecheck.Spec(cfg)
    tuples = oracle.level_tuples(oracle.config(np_=np_), 12)
    fr = cm.Frontier(spec, tuples)
    kw.setdefault("nslots", 2 * (fr.total() + 1))
    if kw.get("flags", 0) & cm.PF_DEFER:
        kw.setdefault("prev", fr)
        return cm.selftest(kind, cfg, **kw)[0]
    return cm.selftest(kind, cfg, fr, **kw)[0]


def test_harness_validates_on_the_host(oracle):
    ok = {0, -errno.ENODEV} if kubecheck.device_count() else {-errno.ENODEV}
    assert call(oracle) in ok
    assert call(oracle, kind=cm.K_SHARD, world=3, rank=2, stage_cap=100) in ok
    assert call(oracle, kind=cm.K_FIRST_C8, flags=cm.PF_CSUM) in ok
    assert call(oracle, flags=cm.PF_DEFER, links=[(0, 0), (1, 0)]) in ok
    EINVAL = -errno.EINVAL
    spec = kubecheck.Spec(kubecheck.ModelConfig())
    fr = cm.Frontier(spec, oracle.level_tuples(oracle.config(), 12))
    bad = fr.packed().copy()
    bad[1] = cm.M64                                   # an out-of-domain parent
    assert cm.selftest(cm.K_EXACT, spec.cfg, packed=bad, nslots=4096)[0] == EINVAL
    assert call(oracle, flags=cm.PF_DEFER, links=[(0, 0), (fr.n, 0)]) == EINVAL          # a link past nprev
    nsucc = len(fr.parent(0).succ)
    assert call(oracle, flags=cm.PF_DEFER, links=[(0, nsucc - 1)]) in ok
    assert call(oracle, flags=cm.PF_DEFER, links=[(0, nsucc)]) == EINVAL                 # a position past the count
    assert call(oracle, nslots=fr.total()) == EINVAL                                     # no free slot left
    assert call(oracle, nslots=fr.total() + 1) in ok
    full = np.zeros(2 * (fr.total() + 4), dtype=U64)
    full[0:8:2] = [11, 12, 13, 14]
    assert call(oracle, nslots=fr.total() + 4, table=full) == EINVAL                     # ... with what is stored
    assert call(oracle, kind=cm.K_SHARD, world=3, rank=3) == EINVAL                      # rank >= world
    assert call(oracle, kind=cm.K_SHARD, world=9, rank=0) == EINVAL
    assert call(oracle, kind=cm.K_SHARD, world=1, rank=0) == EINVAL
    assert call(oracle, kind=cm.K_FIRST_C8, nslots=2 * fr.total() + 3) == EINVAL         # odd compact table
    assert call(oracle, kind=cm.K_FIRST_C8, nslots=2 * fr.total() + 4) in ok
    assert call(oracle, kind=7) == EINVAL
    assert call(oracle, level=0) == EINVAL
    assert call(oracle, flags=cm.PF_CSUM) == EINVAL                                      # csum: first-claim only
    assert call(oracle, kind=cm.K_SHARD, world=2, rank=0, base=256) == EINVAL
    stray = np.zeros(2 * 4096, dtype=U64)
    stray[5] = 1                                                                         # a claim word, no fp
    assert call(oracle, nslots=4096, table=stray) == EINVAL
