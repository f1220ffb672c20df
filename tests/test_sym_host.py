"""Symmetry reduction on the host (no GPU): the fixtures against the oracle and
the host model (tests/sym_model.py), the spec's symmetry, kc_spec_permute and
kc_spec_fingerprint_sym against the model, cfg parsing and the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kubecheck
import pyoracle
import sym_model
from kubecheck import _lib, tlc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "sym_fixtures.json")))

# the cases re-derived live: (model, symmetry, levels)
LIVE = {
    "121_ml30": ((1, 2, 1), "controllers", 30),
    "211_c4": ((2, 1, 1), "clients", 10),
    "131_ml14": ((1, 3, 1), "controllers", 14),
}


class Case:
    """Every level of one live case: the oracle's states, per level."""

    def __init__(self, name):
        self.model, self.sym, self.nlev = LIVE[name]
        self.nc, self.np_, self.ns = self.model
        self.mask = sym_model.MASKS[self.sym]
        self.cfg = pyoracle.config(*self.model, max_levels=self.nlev)
        self.levels = [pyoracle.level_tuples(self.cfg, lv) for lv in range(1, self.nlev + 1)]
        self.group = sym_model.group(self.nc, self.np_, self.mask)
        self.spec = kubecheck.Spec(kubecheck.ModelConfig(nc=self.nc, np=self.np_, ns=self.ns, symmetry=self.sym))


@pytest.fixture(scope="module", params=list(LIVE))
def case(request):
    return Case(request.param)


def _key(rows):
    return [r.tobytes() for r in np.ascontiguousarray(rows)]


# ------------------------------------------------------------------ fixtures
def test_fixture_matches_live_model(case, request):
    name = request.node.callspec.params["case"]
    fx = FIX[name]["before_error"] if "before_error" in FIX[name] else FIX[name]
    widths = [len(sym_model.orbit_reps(t, case.nc, case.np_, case.mask)) for t in case.levels]
    assert widths == fx["level_width"]
    assert [len(t) for t in case.levels] == fx["states_width"]
    assert sum(widths) == fx["distinct"]


def test_fixture_matches_the_measured_table():
    # (states, orbits) measured independently when the feature was proposed
    table = {"121_ml22": (19270, 10201), "121_ml30": (149618, 75914), "121_ml36": (699193, 351116),
             "121_ml40_nofaults": (66194, 33288), "131_ml14": (22880, 5056)}
    for name, (states, orbits) in table.items():
        assert (FIX[name]["states"], FIX[name]["distinct"]) == (states, orbits), name
    assert FIX["121_ml30"]["level_width"][-4:] == [7841, 10324, 13524, 17683]
    assert FIX["121_ml36"]["level_width"][-4:] == [38100, 48228, 60572, 75465]
    e = FIX["121_v1_nolostupdate"]
    assert (e["error"]["err_kind"], e["error"]["err_invariant"], e["error"]["err_level"]) == (2, 2, 25)
    assert (e["error"]["states"], e["before_error"]["distinct"]) == (33714, 16154)
    e = FIX["211_c4"]
    assert (e["error"]["err_kind"], e["error"]["err_action"], e["error"]["err_level"]) == (1, "C4", 10)
    assert (e["error"]["states"], e["before_error"]["distinct"]) == (3845, 1851)
    # the symmetric widths pass the narrow path's 8192 at level 28
    w = FIX["121_ml34"]["level_width"]
    assert w[26] <= 8192 < w[27]
    # generated: the oracle's own count where the group is trivial
    ref = pyoracle.run(pyoracle.config(1, 2, 1, max_levels=12))
    assert sym_model.expected(pyoracle.config(1, 2, 1, max_levels=12), 1)["generated"] == ref["generated"] == 10555


# ------------------------------------------------------- the spec is symmetric
def _check_symmetric(cfg, levels, nc, np_, group):
    """successors(pi.s) == pi.successors(s) as sets, for every s of every
    level and every pi; every level is closed under the group."""
    for t in levels:
        succ, flat, bounds = {}, [], [0]
        for s in t:
            out, fail = pyoracle.successors(cfg, s)
            rows = [x for _, x in out] if out is not None else []
            succ[s.tobytes()] = (frozenset(x.tobytes() for x in rows), fail)
            flat.extend(rows)
            bounds.append(len(flat))
        flat = np.array(flat, dtype=np.uint64).reshape(-1, t.shape[1])
        for perm in group[1:]:
            pt = _key(sym_model.permute(t, perm, nc, np_))
            pf = _key(sym_model.permute(flat, perm, nc, np_)) if len(flat) else []
            for i, s in enumerate(t):
                assert pt[i] in succ, "a level is not closed under the group"
                want, fail = succ[pt[i]]
                assert fail == succ[s.tobytes()][1]
                assert frozenset(pf[bounds[i]:bounds[i + 1]]) == want


def test_spec_is_symmetric(case):
    _check_symmetric(case.cfg, case.levels, case.nc, case.np_, case.group)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
def test_variants_are_symmetric_under_controllers(variant):
    cfg = pyoracle.config(1, 2, 1, max_levels=14, variant=variant, invariants=7 if variant == 1 else 3)
    n = len(pyoracle.run(cfg)["level_width"])
    levels = [pyoracle.level_tuples(cfg, lv) for lv in range(1, n + 1)]
    _check_symmetric(cfg, levels, 1, 2, sym_model.group(1, 2, 2))


def test_variant5_init_and_its_refusal():
    # variant 5's Init store names actor 0 in a version vector: closed under
    # the controllers' group of (1,2,1), not under the clients' of (2,1,1)
    init = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2, variant=5)).init()
    assert np.array_equal(init, pyoracle.level_tuples(pyoracle.config(1, 2, 1, variant=5, max_levels=1), 1))
    for perm in sym_model.group(1, 2, 2):
        assert set(_key(sym_model.permute(init, perm, 1, 2))) == set(_key(init))
    init = kubecheck.Spec(kubecheck.ModelConfig(nc=2, np=1, variant=5)).init()
    assert set(_key(sym_model.permute(init, (1, 0, 2), 2, 1))) != set(_key(init))
    lib = kubecheck.load()
    h = C.c_void_p()
    c = kubecheck.ModelConfig(nc=2, np=1, variant=5, symmetry="clients").to_c()
    assert lib.kc_engine_create(C.byref(c), C.byref(h)) == -22
    assert b"variant 5" in lib.kc_last_error()


# ------------------------------------------------------------ kc_spec_permute
def test_spec_permute_matches_model(case):
    for perm in case.group:
        for t in case.levels:
            want = sym_model.permute(t, perm, case.nc, case.np_)
            for i, s in enumerate(t):
                assert np.array_equal(case.spec.permute(s, perm), want[i])


def test_spec_permute_refuses_bad_perms():
    sp = kubecheck.Spec(kubecheck.ModelConfig(nc=2, np=2))
    s = sp.init()[1]
    assert np.array_equal(sp.permute(s, (0, 1, 2, 3)), s)
    for perm in [(2, 1, 0, 3), (0, 1, 2, 2), (0, 1, 2, 4), (-1, 1, 2, 3), (1, 2, 3, 0)]:
        with pytest.raises(kubecheck.KubecheckError) as e:
            sp.permute(s, perm)
        assert e.value.code == -22 and "permutation" in str(e.value)


# ---------------------------------------------------- kc_spec_fingerprint_sym
def test_fingerprint_sym_is_the_orbits(case):
    plain = kubecheck.Spec(kubecheck.ModelConfig(nc=case.nc, np=case.np_, ns=case.ns))
    for t in case.levels:
        fps = {k: case.spec.fingerprint_sym(s) for k, s in zip(_key(t), t)}
        # one value per orbit, the minimum of the plain fingerprints over it
        assert len(set(fps.values())) == len(sym_model.orbit_reps(t, case.nc, case.np_, case.mask))
        orbit_min = {k: plain.fingerprint(s) for k, s in zip(_key(t), t)}
        for perm in case.group[1:]:
            for k, pk in zip(_key(t), _key(sym_model.permute(t, perm, case.nc, case.np_))):
                assert fps[pk] == fps[k]
                orbit_min[k] = min(orbit_min[k], plain.fingerprint(np.frombuffer(pk, dtype=np.uint64)))
        assert orbit_min == fps


def test_fingerprint_sym_off_and_trivial_group():
    t = pyoracle.level_tuples(pyoracle.config(1, 2, 1, max_levels=16), 16)
    plain = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2))
    off = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2, symmetry=0))
    trivial = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2, symmetry="clients"))
    on = kubecheck.Spec(kubecheck.ModelConfig(nc=1, np=2, symmetry="actors"))
    differs = 0
    for s in t:
        fp = plain.fingerprint(s)
        assert off.fingerprint_sym(s) == fp and trivial.fingerprint_sym(s) == fp
        differs += on.fingerprint_sym(s) != fp
    assert 0 < differs < len(t)


# ------------------------------------------------------ parsing and refusals
def test_model_config_symmetry_reaches_c():
    MC = kubecheck.ModelConfig
    assert MC().to_c().symmetry == 0
    assert [MC(symmetry=s).to_c().symmetry for s in (0, "clients", "controllers", "actors", 1, 2, 3)] == \
        [0, 1, 2, 3, 1, 2, 3]
    for bad in ("servers", 4, -1):
        with pytest.raises(ValueError):
            MC(symmetry=bad).to_c()
    c = _lib.KcModelConfig()
    c.symmetry = 3
    kubecheck.load().kc_model_config_default(C.byref(c))
    assert c.symmetry == 0


def test_cfg_symmetry_keyword():
    text = open(os.path.join(ROOT, "models", "Symmetry.cfg")).read()
    cfg = tlc.parse_cfg(text)
    assert cfg["symmetry"] == "SymControllers"
    assert tlc.check_from_cfg(cfg) == ({"can_fail": True, "can_timeout": True, "invariants": 3,
                                        "symmetry": "controllers"}, [])
    for name, sym in (("SymClients", "clients"), ("SymActors", "actors")):
        assert tlc.model_from_cfg(tlc.parse_cfg(text.replace("SymControllers", name)))["symmetry"] == sym
    # nothing changes without the keyword
    plain = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Model_1.cfg")).read())
    assert plain["symmetry"] is None and "symmetry" not in tlc.model_from_cfg(plain)
    with pytest.raises(tlc.CfgError):
        tlc.parse_cfg(text.replace("SymControllers", "Permutations(Controllers)"))
    with pytest.raises(tlc.CfgError):
        tlc.parse_cfg(text + "SYMMETRY SymClients\n")
    with pytest.raises(tlc.CfgError, match="PROPERTY"):
        tlc.check_from_cfg(tlc.parse_cfg(text + "PROPERTY ReconcileCompletes\n"))
    with pytest.raises(tlc.CfgError, match="-simulate"):
        tlc.check_from_cfg(cfg, simulate=True)


def test_banner_names_the_symmetry_set():
    r = kubecheck.CheckResult.__new__(kubecheck.CheckResult)
    r.__dict__.update(init=2, distinct=2, generated=2, error=None, depth=1, queue_left=0, outdeg_hist=[],
                      act_dist={a: 0 for a in tlc.ACTION_SPANS}, act_gen={a: 0 for a in tlc.ACTION_SPANS})
    on = dict((c, b) for c, _, b in tlc.messages(r, 0.0, 1.0, symmetry="SymControllers"))
    off = dict((c, b) for c, _, b in tlc.messages(r, 0.0, 1.0))
    assert on[2187].endswith("Symmetry set: SymControllers.") and "Symmetry" not in off[2187]
    assert on[2187].startswith(off[2187])


def test_refused_where_symmetry_is_unsound_or_unsupported():
    lib = kubecheck.load()
    h = C.c_void_p()
    c = kubecheck.ModelConfig(nc=1, np=2, symmetry="controllers").to_c()
    live = _lib.KcLiveConfig(0, 0, 0)
    assert lib.kc_live_create(C.byref(c), C.byref(live), C.byref(h)) == -22
    assert b"symmetry" in lib.kc_last_error() and b"unsound" in lib.kc_last_error()
    assert lib.kc_shard_create(C.byref(c), 0, 1, C.byref(h)) == -22
    assert b"symmetry" in lib.kc_last_error() and b"owner projection" in lib.kc_last_error()
    sim = _lib.KcSimConfig(1, 64, 10, 0, 0, 1)
    assert lib.kc_sim_create(C.byref(c), C.byref(sim), C.byref(h)) == -22
    assert b"symmetry" in lib.kc_last_error()
    # the Python entry points raise
    with pytest.raises(kubecheck.KubecheckError, match="symmetry"):
        kubecheck.LivenessChecker(kubecheck.ModelConfig(nc=1, np=2, symmetry="controllers"))
    with pytest.raises(kubecheck.KubecheckError, match="symmetry"):
        kubecheck.Simulator(kubecheck.ModelConfig(nc=1, np=2, symmetry="controllers"), num_walks=64)
    # the engine: a mask outside 0..3
    c = kubecheck.ModelConfig(nc=1, np=2).to_c()
    c.symmetry = 4
    assert lib.kc_engine_create(C.byref(c), C.byref(h)) == -22
    assert b"symmetry" in lib.kc_last_error()
