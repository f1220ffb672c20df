"""The engine's own probe loops (k_claim's pipelined group, k_nfinish, the
sharded narrow kernel, the settle passes) on a seen-set whose size is chosen,
not defaulted: ModelConfig.fpset_slots sets nslots directly, it need not be a
power of two, and a table that never grows holds a slot set that does not
depend on the insertion order, so the host model's table (probe_model.py) is
the run's table.

The size is searched by the model for one at which Model_1's fingerprints
are carried across the table's end (table_edge_search.find_size).  For the
163,408 Model_1 fingerprints NO size does that: slots are monotone in the
remixed fingerprint fp * G mod 2^64, the table's end is the top of that space
at every size, and the four largest remixed fingerprints lie 0.64, 1.12, 1.84
and 2.76 mean spacings below 2^64 — at the <= 1/3 load a table that does not
grow must keep, 1.9 slots or more apart.  The sizes of one window are not
independent draws.  test_no_size_carries_model1_across_the_end pins that
finding (the model's count at every even size of the window, engine and each
rank at R = 3), so the day a fingerprint set does reach the end the runs below
use that size.  The probe loops AT the end are pinned by test_gpu_probe.py on
the primitives; what the runs here pin is every engine path on a
non-power-of-two table that never grows: exact counts, fpset_slots == N and
the exact minimum gap of the stored fingerprint set."""
import numpy as np
import pytest

import kubecheck
import table_edge_search as tes
from kubecheck import ModelChecker, ModelConfig, Spec
from kubecheck.distributed import NativeShardedChecker

pytestmark = pytest.mark.gpu

BASE = (1 << 20) + 2          # the first even size past the default 2^20 (not a power of two)
# a narrow run reserves room for 2^20 new states (engine.hip run_narrow), so a
# table below 3 * (2^20 + 163,408) slots is grown 4x before the first level
BASE_NARROW = (1 << 22) + 2
R = 3


def sharded_fps(fps, packed):
    """The sharded path's fingerprints (kubeapi_spec.h fingerprint<1>): the low
    59 bits are the fold, the top 4 a hash of apiState (word 0) and the
    listRequests objs word folded to 32 bits (Model_1: word 3)."""
    w0, w = packed[:, 0], packed[:, 3]
    v = (w ^ (w >> np.uint64(32))) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        z = w0 * np.uint64(0x9e3779b97f4a7c15) + v
        z ^= z >> np.uint64(31)
        z *= np.uint64(0xbf58476d1ce4e5b9)
    h = (fps & np.uint64((1 << 59) - 1)) | ((z >> np.uint64(60)) << np.uint64(59))
    h[h == 0] = 1
    return h


@pytest.fixture(scope="module")
def m1(oracle, fixtures):
    """Model_1's fingerprints computed on the CPU: the oracle's states of every
    level through the lowered spec's fingerprint (no GPU)."""
    fx = fixtures["model1"]
    cfg, spec = oracle.config(), Spec(ModelConfig())
    tuples = np.concatenate([oracle.level_tuples(cfg, lv) for lv in range(1, fx["depth"] + 1)])
    fps = np.array([spec.fingerprint(t) for t in tuples], dtype=np.uint64)
    assert len(fps) == len(set(fps.tolist())) == fx["distinct"] == 163408
    packed = np.array([spec.pack(t) for t in tuples], dtype=np.uint64)
    assert packed.shape[1] == 4
    f1 = sharded_fps(fps, packed)
    lib = kubecheck.load()
    owner = np.array([lib.kc_shard_owner(int(f), R) for f in f1])
    s = np.sort(fps)
    sizes = {}
    for compact in (False, True):
        for who, sets, base in (("engine", [fps], BASE), ("engine_narrow", [fps], BASE_NARROW),
                                ("sharded", [f1[owner == r] for r in range(R)], BASE)):
            n, c = tes.find_size(sets, compact, base=base)
            sizes[compact, who] = (n or base, c, base, sets)
    return dict(fps=fps, f1=f1, owner=owner, gap=int(np.min(s[1:] - s[:-1])), sizes=sizes, fx=fx)


def test_no_size_carries_model1_across_the_end(m1):
    # (see the module docstring) the model's count of fingerprints carried
    # across N - 1 -> 0, over every even size of the window, exact for the
    # size the runs use
    for (compact, who), (n, c, base, sets) in m1["sizes"].items():
        assert c is None and n == base, (compact, who, n, c)
        full = [np.sort(tes.remix(f)) for f in sets]
        assert [tes.carried(r, n, compact) for r in full] == [0] * len(sets)
        # the largest remixed fingerprint's home is short of the last slot (pair)
        assert all(int(tes.homes(r[-1:], n, compact)[0]) < n - 2 for r in full)
    # the model's carry count is the host table's, on a set small enough to build it
    rng = tes.pm.rng(5)
    for compact, kind in ((False, "wide"), (True, "compact")):
        fps = tes.pm.craft(62 if compact else 63, 64, kind, 5, rng) + tes.pm.craft(60, 64, kind, 3, rng) + \
            [rng.getrandbits(63) | 1 for _ in range(12)]
        t = tes.model_table(fps, 64, kind)
        c = tes.carried(np.sort(tes.remix(fps)), 64, compact)
        assert c >= 4 and {i for i in range(c)} <= t.occupied()


MODES = {"minimum": (dict(), None, False), "first_compact": (dict(first_claim=True), "1", True),
         "first_16B": (dict(first_claim=True), "0", False)}
PATHS = {"narrow": dict(), "wide": dict(chunk_states=1 << 20), "wide_chunks": dict(chunk_states=512)}


def _exact(r, m1, first):
    fx = m1["fx"]
    assert r.complete and r.error is None
    assert (r.distinct, r.generated, r.depth) == (fx["distinct"], fx["generated"], fx["depth"])
    assert r.level_width == fx["level_width"] and r.act_gen == fx["act_gen"]
    if first:
        assert sum(r.act_dist.values()) + r.init == r.distinct
    else:
        assert r.act_dist == fx["act_dist"]


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_engine_chosen_table_size(m1, monkeypatch, mode, path):
    kw, compact_env, compact = MODES[mode]
    if compact_env is not None:
        monkeypatch.setenv("KC_CLAIM_COMPACT", compact_env)
    n = m1["sizes"][compact, "engine_narrow" if path == "narrow" else "engine"][0]
    with ModelChecker(ModelConfig(fpset_slots=n, **kw, **PATHS[path])) as mc:
        r = mc.run()
        gap, _ = mc.check_fps()
    assert r.fpset_slots == n                      # no rehash: the model's table is the run's
    assert r.claim_mode == ("first" if kw else "minimum")
    _exact(r, m1, bool(kw))
    assert gap == m1["gap"]                        # the table holds exactly this fingerprint set


@pytest.mark.parametrize("snarrow", ["1", "0"])
@pytest.mark.parametrize("first", [False, True])
def test_sharded_chosen_table_size(m1, monkeypatch, first, snarrow):
    monkeypatch.setenv("KC_SNARROW", snarrow)
    n = m1["sizes"][first, "sharded"][0]
    fx = m1["fx"]
    mc = NativeShardedChecker(ModelConfig(fpset_slots=n, first_claim=first), emulate=R)
    try:
        r = mc.run()
        ranks = [mc.shard_result(i) for i in range(R)]
    finally:
        mc.close()
    assert r["claim_mode"] == ("first" if first else "minimum")
    assert r["complete"] and r["error"] is None and r["level_width"] == fx["level_width"]
    assert (r["distinct"], r["generated"], r["depth"]) == (fx["distinct"], fx["generated"], fx["depth"])
    assert r["act_gen"] == fx["act_gen"] and sum(r["act_dist"].values()) + r["init"] == r["distinct"]
    assert [k["fpset_slots"] for k in ranks] == [n] * R        # no rank's table grew
    # every rank stored exactly the fingerprints the model says it owns
    assert [k["distinct"] for k in ranks] == [int((m1["owner"] == i).sum()) for i in range(R)]


# --- growth on the compact table from a tiny size (the first-claim twin of
# test_multi_chunk_and_rehash_paths): every table from 64 slots up is filled
# past 1/3 and rehashed
@pytest.mark.parametrize("compact", ["1", "0"])
@pytest.mark.parametrize("path", ["narrow", "wide_chunks"])
def test_first_claim_growth_from_64_slots(m1, monkeypatch, path, compact):
    monkeypatch.setenv("KC_CLAIM_COMPACT", compact)
    kw = dict(chunk_states=256) if path == "wide_chunks" else {}
    with ModelChecker(ModelConfig(fpset_slots=64, first_claim=True, **kw)) as mc:
        r = mc.run()
        gap, _ = mc.check_fps()
    assert r.claim_mode == "first" and r.fpset_slots > 64
    _exact(r, m1, True)
    assert gap == m1["gap"]
