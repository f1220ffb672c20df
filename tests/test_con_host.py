"""Constraints (TLC's CONSTRAINT / ACTION_CONSTRAINT) without a GPU: the cfg
keywords and the refused combinations, the ModelConfig fields down to the C
struct, the host predicate kc_spec_in_model against the host model
(tests/con_model.py) on every (parent, successor) pair of two constrained
runs, and the fixture file recomputed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import con_model
import kubecheck
from kubecheck import _lib, tlc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "constraint_fixtures.json")))
HEAD = "CONSTANT REQUESTS_CAN_FAIL = TRUE\nCONSTANT REQUESTS_CAN_TIMEOUT = TRUE\nINVARIANT TypeOK OnlyOneVersion\n"
BASE = {"can_fail": True, "can_timeout": True, "invariants": 3}


# ------------------------------------------------------------------ the cfg
def test_constraint_cfg_file():
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Constraint.cfg")).read())
    assert cfg["constraints"] == ["InFlightAtMost1"] and cfg["action_constraints"] == []
    assert tlc.model_from_cfg(cfg) == dict(BASE, constraint_inflight=1)
    assert tlc.check_from_cfg(cfg) == (dict(BASE, constraint_inflight=1), [])
    c = kubecheck.ModelConfig(**tlc.model_from_cfg(cfg)).to_c()
    assert (c.constraint_stored, c.constraint_inflight, c.action_constraints) == (-1, 1, 0)


@pytest.mark.parametrize("text,want", [
    ("CONSTRAINT StoredAtMost1", dict(constraint_stored=1)),
    ("CONSTRAINTS StoredAtMost12", dict(constraint_stored=12)),
    ("CONSTRAINT InFlightAtMost0", dict(constraint_inflight=0)),
    ("ACTION_CONSTRAINT ServeClientsFirst", dict(action_constraints=["ServeClientsFirst"])),
    ("ACTION_CONSTRAINTS ServeClientsFirst", dict(action_constraints=["ServeClientsFirst"])),
    ("CONSTRAINT StoredAtMost1 InFlightAtMost2\nACTION_CONSTRAINT ServeClientsFirst",
     dict(constraint_stored=1, constraint_inflight=2, action_constraints=["ServeClientsFirst"])),
    ("CONSTRAINT StoredAtMost1\nCONSTRAINT InFlightAtMost2", dict(constraint_stored=1, constraint_inflight=2)),
])
def test_cfg_each_name(text, want):
    assert tlc.model_from_cfg(tlc.parse_cfg(HEAD + text)) == dict(BASE, **want)


def test_cfg_without_constraints_is_unchanged():
    assert tlc.model_from_cfg(tlc.parse_cfg(HEAD)) == BASE
    c = kubecheck.ModelConfig().to_c()
    assert (c.constraint_stored, c.constraint_inflight, c.action_constraints) == (-1, -1, 0)


@pytest.mark.parametrize("text", ["CONSTRAINT StoredAtMost", "CONSTRAINT Cardinality(apiState)<2",
                                  "CONSTRAINT ServeClientsFirst", "ACTION_CONSTRAINT StoredAtMost1",
                                  "ACTION_CONSTRAINT ServeServersFirst", "CONSTRAINT storedatmost1"])
def test_cfg_unknown_name_lists_the_known(text):
    with pytest.raises(tlc.CfgError) as e:
        tlc.parse_cfg(HEAD + text)
    for name in ("StoredAtMost<k>", "InFlightAtMost<k>", "ServeClientsFirst"):
        assert name in str(e.value)


@pytest.mark.parametrize("text", ["CONSTRAINT StoredAtMost1 StoredAtMost2", "CONSTRAINT InFlightAtMost1\nCONSTRAINT InFlightAtMost1"])
def test_cfg_two_bounds_of_a_family(text):
    with pytest.raises(tlc.CfgError, match="one per family"):
        tlc.parse_cfg(HEAD + text)


@pytest.mark.parametrize("con", ["CONSTRAINT StoredAtMost1", "ACTION_CONSTRAINT ServeClientsFirst"])
def test_cfg_refused_combinations(con):
    cfg = tlc.parse_cfg(HEAD + con)
    tlc.check_from_cfg(cfg)
    for kw in (dict(simulate=True), dict(coverage=True), dict(checkpointing=True)):
        with pytest.raises(tlc.CfgError, match="CONSTRAINT"):
            tlc.check_from_cfg(cfg, **kw)
    with pytest.raises(tlc.CfgError, match="PROPERTY"):
        tlc.check_from_cfg(tlc.parse_cfg(HEAD + con + "\nPROPERTY ReconcileCompletes"))
    sym = tlc.parse_cfg(HEAD + con + "\nSYMMETRY SymControllers")
    with pytest.raises(tlc.CfgError, match="SYMMETRY"):
        tlc.check_from_cfg(sym)
    with pytest.raises(tlc.CfgError, match="SYMMETRY"):
        tlc.model_from_cfg(sym)


# ------------------------------------------------------- ModelConfig -> C
def test_model_config_reaches_c():
    MC = kubecheck.ModelConfig
    c = MC(constraint_stored=3, constraint_inflight=0, action_constraints="ServeClientsFirst").to_c()
    assert (c.constraint_stored, c.constraint_inflight, c.action_constraints) == (3, 0, 1)
    assert [MC(action_constraints=a).to_c().action_constraints for a in (0, 1, [], ["ServeClientsFirst"])] == [0, 1, 0, 1]
    for bad in ("ServeServersFirst", 2, ["x"]):
        with pytest.raises(ValueError):
            MC(action_constraints=bad).to_c()
    d = _lib.KcModelConfig()
    d.constraint_stored = d.constraint_inflight = 5
    d.action_constraints = 1
    kubecheck.load().kc_model_config_default(C.byref(d))
    assert (d.constraint_stored, d.constraint_inflight, d.action_constraints) == (-1, -1, 0)


# ------------------------------------------------------ the host predicate
def _spec(model, kw):
    nc, np_, ns = model
    return kubecheck.Spec(kubecheck.ModelConfig(
        nc=nc, np=np_, ns=ns, constraint_stored=kw.get("stored_max", -1), constraint_inflight=kw.get("inflight_max", -1),
        action_constraints=1 if kw.get("serve_clients_first") else 0))


def _check_row(rid, r):
    fx = FIX["rows"][rid]
    for k in ("generated", "distinct", "depth", "cut_state", "cut_action", "level_width", "act_gen", "act_dist"):
        assert r[k] == fx[k], (rid, k)


@pytest.mark.parametrize("rid", ["np2_stored1_serve", "model1_inflight1"])
def test_spec_in_model_equals_host_model_on_every_pair(rid):
    (_, model, kw), = [r for r in con_model.ROWS if r[0] == rid]
    sp = _spec(model, kw)
    lib, cfg = sp._lib, C.byref(sp._c)
    u64 = C.POINTER(C.c_uint64)
    seen = {"pairs": 0, "cuts": [0, 0, 0]}

    def on_pairs(S, X, acts, cuts):
        for i in range(len(acts)):
            got = lib.kc_spec_in_model(cfg, S[i].ctypes.data_as(u64), X[i].ctypes.data_as(u64), int(acts[i]))
            assert got == cuts[i], (rid, seen["pairs"] + i, got, int(cuts[i]))
            seen["cuts"][got] += 1
        seen["pairs"] += len(acts)

    r = con_model.run(*model, on_pairs=on_pairs, **kw)
    _check_row(rid, r)
    assert seen["pairs"] == r["generated"] - r["init"]
    assert seen["cuts"][1:] == [r["cut_state"], r["cut_action"]]


# the other two instantiations built with constraints, capped: (2,1,1) is the
# shape whose client mask has two bits per half, (1,3,1) the one whose object
# universe fills word 0 (U = 64: no ghost bit below which to count)
OTHER_MODELS = [((2, 1, 1), dict(stored_max=1, inflight_max=2, serve_clients_first=True), 10),
                ((2, 1, 1), dict(serve_clients_first=True), 10),
                ((1, 3, 1), dict(stored_max=1, inflight_max=2, serve_clients_first=True), 12),
                ((1, 3, 1), dict(stored_max=1), 10)]


@pytest.mark.parametrize("model,kw,max_levels", OTHER_MODELS)
def test_spec_in_model_equals_host_model_other_models(model, kw, max_levels):
    sp = _spec(model, kw)
    lib, cfg = sp._lib, C.byref(sp._c)
    u64 = C.POINTER(C.c_uint64)
    cuts = [0, 0, 0]

    def on_pairs(S, X, acts, want):
        for i in range(len(acts)):
            got = lib.kc_spec_in_model(cfg, S[i].ctypes.data_as(u64), X[i].ctypes.data_as(u64), int(acts[i]))
            assert got == want[i], (model, i, got, int(want[i]))
            cuts[got] += 1

    r = con_model.run(*model, max_levels=max_levels, on_pairs=on_pairs, **kw)
    assert r["error"] is None and sum(cuts) == r["generated"] - r["init"] > 5000
    assert cuts[1:] == [r["cut_state"], r["cut_action"]]
    assert (cuts[1] > 0) == ("stored_max" in kw) and (cuts[2] > 0) == bool(kw.get("serve_clients_first"))


def test_stored_counts_word0_with_and_without_a_ghost_bit():
    # (1,3,1): U = 64, bit 63 of word 0 is an object; (1,1,1): bit 63 is the lostUpdate ghost
    for model, want in (((1, 3, 1), 2), ((1, 1, 1), 1)):
        x = _spec(model, {}).init()[0].copy()
        x[0] = (1 << 63) | 1
        assert con_model.stored(x, model[0] + model[1]) == want
        for k in (0, 1, 2):
            assert _spec(model, dict(stored_max=k)).in_model(None, x, "CStart") == ("state" if want > k else None)


def test_cli_refusals_end_in_an_error_line(capsys):
    cfg = os.path.join(ROOT, "models", "Constraint.cfg")
    for extra in (["-coverage"], ["-simulate"], ["-checkpointlevels", "5"], ["-recover", "nowhere"]):
        assert tlc.main(["-tool", "-config", cfg] + extra) == 1
        cap = capsys.readouterr()
        assert cap.err.startswith("Error: CONSTRAINT / ACTION_CONSTRAINT (InFlightAtMost1) with ") and cap.out == ""
        assert cap.err.count("\n") == 1


def test_cli_refusals_of_cfg_combinations(tmp_path, capsys):
    for extra, needle in (("PROPERTY ReconcileCompletes", "PROPERTY"), ("SYMMETRY SymControllers", "SYMMETRY")):
        p = tmp_path / "c.cfg"
        p.write_text(HEAD + "ACTION_CONSTRAINT ServeClientsFirst\n" + extra + "\n")
        assert tlc.main(["-tool", "-config", str(p)]) == 1
        cap = capsys.readouterr()
        assert cap.err.startswith("Error: CONSTRAINT / ACTION_CONSTRAINT (ServeClientsFirst) with ") and needle in cap.err
        assert cap.out == ""


def test_spec_in_model_arguments():
    sp = _spec((1, 1, 1), dict(stored_max=0, serve_clients_first=True))
    init = sp.init()
    lib, u64 = sp._lib, C.POINTER(C.c_uint64)
    x = init[0].ctypes.data_as(u64)
    assert lib.kc_spec_in_model(C.byref(sp._c), None, x, 0) == -22          # NULL parent with an action constraint
    assert lib.kc_spec_in_model(C.byref(sp._c), x, x, 22) == -22            # no such action
    assert lib.kc_spec_in_model(C.byref(sp._c), x, x, 4) == 0
    st = _spec((1, 1, 1), dict(stored_max=0))
    assert st.in_model(None, init[0], "CStart") is None                     # Init: the state constraints alone
    full = init[0].copy()
    full[0] = 1
    assert st.in_model(None, full, "CStart") == "state"
    assert _spec((2, 2, 1), dict(stored_max=0))._lib.kc_spec_in_model(
        C.byref(_spec((2, 2, 1), dict(stored_max=0))._c), None, x, 0) == -22   # a model not built with constraints


# ---------------------------------------------------------- the fixture file
@pytest.mark.parametrize("rid", con_model.SMALL)
def test_fixture_rows_recomputed(rid):
    assert con_model.row_fixture(rid) == json.loads(json.dumps(FIX["rows"][rid]))


def test_fixture_rule4_recomputed():
    assert con_model.rule4_fixture() == FIX["rule4"]
    fx = FIX["rule4"]
    # the violating state is outside the constraint, every state before it inside
    assert fx["trace_stored"][-1] > fx["stored_max"] and max(fx["trace_stored"][:-1]) <= fx["stored_max"]
    assert not fx["violation_at_stored_max_1"]


def test_fixture_matches_the_issue_table():
    want = {"model1_inflight1": (575716, 162398, 124, 6442, 0), "model1_inflight0": (411, 102, 15, 70, 0),
            "model1_stored1": (2945, 825, 25, 33, 0), "model1_stored2": (577736, 163408, 124, 0, 0),
            "model1_serve": (577736, 163408, 124, 0, 1010), "np2_stored1": (48050, 9075, 31, 363, 0),
            "np2_stored1_serve": (48050, 9075, 31, 363, 220)}
    for rid, t in want.items():
        fx = FIX["rows"][rid]
        assert (fx["generated"], fx["distinct"], fx["depth"], fx["cut_state"], fx["cut_action"]) == t, rid
    assert FIX["rows"]["model1_inflight0"]["level_width"][:8] == [2, 4, 6, 8, 10, 13, 12, 11]
    assert max(FIX["rows"]["np2_stored1"]["level_width"]) == 663
