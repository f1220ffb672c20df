"""Action properties (TLC's PROPERTY [][A]_vars) without a GPU: the cfg
vocabulary and the refused combinations, the ModelConfig field down to the C
struct, the host predicate kc_spec_step_violations against the host model
(tests/act_model.py) on every step of two runs, the fixture file recomputed,
the variant-1 trace against the oracle's NoLostUpdate trace, and the 2112
message block."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import act_model
import kubecheck
import pyoracle
from kubecheck import _lib, tlc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "actprop_fixtures.json")))
ORACLE = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_fixtures.json")))
HEAD = "CONSTANT REQUESTS_CAN_FAIL = TRUE\nCONSTANT REQUESTS_CAN_TIMEOUT = TRUE\nINVARIANT TypeOK OnlyOneVersion\n"
BASE = {"can_fail": True, "can_timeout": True, "invariants": 3}
NAMES = ("NoBlindUpdate", "OneReplyPerStep", "StoreNeverShrinks")


# ------------------------------------------------------------------ the cfg
def test_vocabulary_is_one():
    assert tuple(kubecheck.ACTION_PROPERTIES) == NAMES == act_model.PROPERTIES == tlc.ACTION_PROPERTY_NAMES
    assert [kubecheck.ACTION_PROPERTIES[n] for n in NAMES] == [1, 2, 4]
    assert _lib.ERR_KINDS[4] == "action_property"


def test_action_property_cfg_file():
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "ActionProperty.cfg")).read())
    assert cfg["properties"] == ["NoBlindUpdate", "OneReplyPerStep"]
    kw, props = tlc.check_from_cfg(cfg)
    assert kw == dict(BASE, action_properties=("NoBlindUpdate", "OneReplyPerStep")) and props == []
    assert kubecheck.ModelConfig(**kw).to_c().action_properties == 3


@pytest.mark.parametrize("text,act,temporal", [
    ("PROPERTY StoreNeverShrinks", ("StoreNeverShrinks",), []),
    ("PROPERTIES NoBlindUpdate NoBlindUpdate", ("NoBlindUpdate",), []),
    ("PROPERTY ReconcileCompletes NoBlindUpdate CleansUpProperly OneReplyPerStep",
     ("NoBlindUpdate", "OneReplyPerStep"), ["ReconcileCompletes", "CleansUpProperly"]),
    ("PROPERTY OneReplyPerStep\nPROPERTY CleansUpProperly", ("OneReplyPerStep",), ["CleansUpProperly"]),
])
def test_cfg_property_list_may_mix(text, act, temporal):
    kw, props = tlc.check_from_cfg(tlc.parse_cfg(HEAD + text))
    assert kw == dict(BASE, action_properties=act) and props == temporal


def test_cfg_without_action_properties_is_unchanged():
    assert tlc.check_from_cfg(tlc.parse_cfg(HEAD + "PROPERTY ReconcileCompletes")) == (BASE, ["ReconcileCompletes"])
    assert tlc.check_from_cfg(tlc.parse_cfg(HEAD)) == (BASE, [])
    assert kubecheck.ModelConfig().to_c().action_properties == 0


def test_cfg_unknown_name_lists_both_vocabularies():
    with pytest.raises(tlc.CfgError) as e:
        tlc.check_from_cfg(tlc.parse_cfg(HEAD + "PROPERTY NoBlindUpdates"))
    for name in NAMES + tuple(kubecheck.PROPERTIES):
        assert name in str(e.value)


REFUSED = [("", dict(simulate=True), "-simulate"), ("", dict(coverage=True), "-coverage"),
           ("", dict(checkpointing=True), "-checkpoint"), ("SYMMETRY SymControllers", {}, "SYMMETRY"),
           ("CONSTRAINT StoredAtMost1", {}, "CONSTRAINT"), ("ACTION_CONSTRAINT ServeClientsFirst", {}, "CONSTRAINT")]


@pytest.mark.parametrize("extra,kw,needle", REFUSED)
def test_cfg_refused_combinations(extra, kw, needle):
    cfg = tlc.parse_cfg(HEAD + "PROPERTY OneReplyPerStep\n" + extra)
    with pytest.raises(tlc.CfgError, match=r"action PROPERTY \(OneReplyPerStep\) with ") as e:
        tlc.check_from_cfg(cfg, **kw)
    assert needle in str(e.value)


def test_cli_refusals_end_in_an_error_line(tmp_path, capsys):
    cfg = os.path.join(ROOT, "models", "ActionProperty.cfg")
    for extra in (["-coverage"], ["-simulate"], ["-checkpointlevels", "5"], ["-recover", "nowhere"]):
        assert tlc.main(["-tool", "-config", cfg] + extra) == 1
        cap = capsys.readouterr()
        assert cap.err.startswith("Error: action PROPERTY (NoBlindUpdate OneReplyPerStep) with ") and cap.out == ""
    p = tmp_path / "c.cfg"
    p.write_text(HEAD + "PROPERTY NoBlindUpdate\nSYMMETRY SymControllers\n")
    assert tlc.main(["-tool", "-config", str(p)]) == 1
    assert "SYMMETRY" in capsys.readouterr().err


# ------------------------------------------------------- ModelConfig -> C
def test_model_config_reaches_c():
    MC = kubecheck.ModelConfig
    got = [MC(action_properties=a).to_c().action_properties
           for a in (0, (), 5, "OneReplyPerStep", ("NoBlindUpdate", "StoreNeverShrinks"), list(NAMES))]
    assert got == [0, 0, 5, 2, 5, 7]
    for bad in ("NoBlindUpdates", 8, ["x"]):
        with pytest.raises(ValueError):
            MC(action_properties=bad).to_c()
    d = _lib.KcModelConfig()
    d.action_properties = 7
    kubecheck.load().kc_model_config_default(C.byref(d))
    assert d.action_properties == 0


# ------------------------------------------------------ the host predicate
def _spec(model, **kw):
    nc, np_, ns = model
    return kubecheck.Spec(kubecheck.ModelConfig(nc=nc, np=np_, ns=ns, action_properties=7, **kw))


def _every_step(model, max_levels=0, **kw):
    """kc_spec_step_violations (all three properties) against act_model's
    predicates on every step of a run; the masks seen."""
    sp = _spec(model, variant=kw.get("variant", 0))
    lib, cfg, u64 = sp._lib, C.byref(sp._c), C.POINTER(C.c_uint64)
    masks = {}

    def on_pairs(S, X, acts, want):
        for i in range(len(acts)):
            got = lib.kc_spec_step_violations(cfg, S[i].ctypes.data_as(u64), X[i].ctypes.data_as(u64), int(acts[i]))
            assert got == want[i], (model, i, got, int(want[i]))
            masks[got] = masks.get(got, 0) + 1

    r = act_model.run(*model, properties=NAMES, max_levels=max_levels, on_pairs=on_pairs, **kw)
    assert sum(masks.values()) == r["step_checked"] == r["generated"] - r["init"]
    return r, masks


def test_spec_step_violations_on_model1_first_30_levels():
    r, masks = _every_step((1, 1, 1), max_levels=30)
    assert r["error"] is None and masks == {0: r["step_checked"]} and r["step_checked"] > 20000


def test_spec_step_violations_on_the_variant1_run():
    # (all three on: the run ends at the first violation, NoBlindUpdate's at depth 27)
    r, masks = _every_step((1, 1, 1), variant=1)
    assert r["error"]["property"] == "NoBlindUpdate" and r["error"]["trace_len"] == 27
    assert masks.get(1, 0) == r["step_violations"]["NoBlindUpdate"] >= 1


def test_spec_step_violations_on_np3_where_word0_is_full():
    # (1,3,1): U = 64, bit 63 of word 0 is an object, not a ghost
    r, masks = _every_step((1, 3, 1), max_levels=9)
    assert r["error"] is None and set(masks) == {0}


def test_spec_step_violations_arguments():
    sp = _spec((1, 1, 1))
    init = sp.init()
    lib, u64 = sp._lib, C.POINTER(C.c_uint64)
    x = init[0].ctypes.data_as(u64)
    assert lib.kc_spec_step_violations(C.byref(sp._c), None, x, 0) == -22
    assert lib.kc_spec_step_violations(C.byref(sp._c), x, x, 22) == -22          # no such action
    assert lib.kc_spec_step_violations(C.byref(sp._c), x, x, 4) == 0             # x == s passes
    shrunk, full = init[0].copy(), init[0].copy()
    full[0] = 3
    shrunk[0] = 1
    assert sp.step_violations(full, shrunk, "APIStart") == 4 and sp.step_violations(shrunk, full, "APIStart") == 0
    other = _spec((2, 2, 1))                                                      # a model not built with them
    assert other._lib.kc_spec_step_violations(C.byref(other._c), x, x, 0) == -22


# ---------------------------------------------------------- the fixture file
@pytest.mark.parametrize("rid", act_model.SMALL)
def test_fixture_rows_recomputed(rid):
    assert act_model.row_fixture(rid) == json.loads(json.dumps(FIX["rows"][rid]))


def test_fixture_verdicts():
    """What the host model found, against the issue's expectation column."""
    rows = FIX["rows"]
    assert rows["model1_noblind"]["verdict"] == rows["model1_onereply"]["verdict"] == "holds"
    for rid in ("model1_noblind", "model1_onereply"):
        assert rows[rid]["complete"] and rows[rid]["step_checked"] == rows[rid]["generated"] - 2 == 577734
        assert rows[rid]["level_width"] == ORACLE["model1"]["level_width"]
    assert rows["model1_shrinks"]["property"] == rows["model1_all"]["property"] == "StoreNeverShrinks"
    assert rows["model1_v1_noblind"]["property"] == rows["np2_v1_noblind"]["property"] == "NoBlindUpdate"
    # steps into already-seen children count: more than one violating step at the error level
    assert rows["np2_nofault_shrinks"]["step_violations"]["StoreNeverShrinks"] > 1
    assert rows["np2_v1_noblind"]["step_violations"]["NoBlindUpdate"] > 1
    for r in rows.values():
        assert r["step_checked"] == r["generated"] - r["init"]
        if r["verdict"] == "violated":
            assert r["trace_len"] == len(r["trace"]) == r["err_level"] == r["depth"] + 1


@pytest.mark.parametrize("rid,oracle_row,length", [("model1_v1_noblind", "variant1_lost_update", 27),
                                                   ("np2_v1_noblind", "np2_variant1_lost_update", 25)])
def test_variant1_trace_is_the_oracles_nolostupdate_trace(rid, oracle_row, length):
    """The step property needs no ghost: its counterexample is the one the
    oracle reports for the NoLostUpdate invariant, bit 63 of word 0 cleared."""
    want = ORACLE[oracle_row]
    assert want["err_invariant"] == 2 and want["trace_len"] == length
    model = FIX["rows"][rid]["model"]
    if rid == "model1_v1_noblind":      # (the small one: the oracle run again, not only its recorded trace)
        got = pyoracle.run(pyoracle.config(*model, variant=1, invariants=7))
        assert got["trace"] == want["trace"]
    mine = FIX["rows"][rid]["trace"]
    assert len(mine) == length
    for a, b in zip(mine, want["trace"]):
        assert [a[0]] + a[1:] == [b[0] & ~(1 << 63)] + b[1:]
        assert not a[0] >> 63


# ------------------------------------------------------------- the messages
def test_2112_message_block():
    fx = FIX["rows"]["model1_v1_noblind"]
    text = "".join(f"State {i + 1}:\n/\\ apiState = {{}}\n/\\ pc = <<{i}>>\n\n" for i in range(fx["trace_len"]))
    zero = {a: 0 for a in kubecheck.ACTIONS}
    r = kubecheck.CheckResult(
        init=2, generated=fx["generated"], distinct=fx["distinct"], queue_left=0, depth=fx["depth"], complete=False,
        act_gen=zero, act_dist=zero, level_width=fx["level_width"], error="action_property", error_action="APIStart",
        error_self=2, error_invariant=None, error_level=fx["err_level"], trace_len=fx["trace_len"], seconds=1.0,
        collision_optimistic=0.0, fpset_slots=0, peak_frontier=0, error_property="NoBlindUpdate", trace_text=text)
    out = tlc.messages(r, 0.0, 1.0)
    codes = [c for c, _, _ in out]
    at = codes.index(2112)
    assert out[at][2] == "Action property NoBlindUpdate is violated." and out[at][1] == 1
    assert codes[at + 1] == 2121 and codes[at + 2: at + 2 + 27] == [2217] * 27 and codes[at + 29] != 2217
    assert out[at + 2][2].startswith("1: ") and out[at + 28][2].startswith("27: ")
    assert 2110 not in codes and 2193 not in codes
    assert tlc.msg(2112, out[at][2], 1, True).startswith("@!@!@STARTMSG 2112:1 @!@!@")
