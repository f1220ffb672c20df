"""The command line's user-defined invariants without a GPU: -defs parsing,
the split of a cfg's INVARIANT list, and every CfgError."""
import os

import pytest

from kubecheck import pred, tlc
from kubecheck.tlc import CfgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = """CONSTANT defaultInitValue = defaultInitValue
CONSTANT REQUESTS_CAN_FAIL = TRUE
CONSTANT REQUESTS_CAN_TIMEOUT = TRUE
SPECIFICATION Spec
"""
DEFS = """---- MODULE Mine ----
\\* a comment line
Small == Cardinality(apiState) <= 2   \\* a trailing comment
Done ==
    \\A c \\in Clients :
        pc[c] = "C5" => ~shouldReconcile[c]

Never == pc["Client"] # "C5"
====
"""


def test_definitions_span_lines_up_to_the_next_name():
    d = pred.parse_definitions(DEFS)
    assert list(d) == ["Small", "Done", "Never"]
    assert pred.parse(d["Small"]) == pred.parse("Cardinality(apiState) <= 2")
    assert pred.parse(d["Done"]) == pred.parse(r'\A c \in Clients : pc[c] = "C5" => ~shouldReconcile[c]')
    assert pred.parse(d["Never"]) == ("cmp", "#", ("atom", "pc", 0), ("const", 13))
    with pytest.raises(pred.PredError, match="defined twice"):
        pred.parse_definitions("A == TRUE\nA == FALSE\n")
    with pytest.raises(pred.PredError, match="no expression"):
        pred.parse_definitions("A ==\nB == TRUE\n")
    with pytest.raises(pred.PredError, match="before the first"):
        pred.parse_definitions("TRUE\nA == TRUE\n")


def test_shipped_reach_files():
    d = pred.parse_definitions(open(os.path.join(ROOT, "models", "Reach.tla")).read())
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Reach.cfg")).read())
    rest, user = tlc.split_user_invariants(cfg, d)
    assert rest["invariants"] == ["TypeOK", "OnlyOneVersion"]
    assert list(user) == ["StoreSmall", "DoneMeansReconciled", "ClientNeverDone"]
    assert tlc.check_from_cfg(rest) == ({"can_fail": True, "can_timeout": True, "invariants": 3}, [])
    for text in d.values():
        pred.parse(text)


def test_split_keeps_cfg_order_and_built_ins():
    d = pred.parse_definitions(DEFS)
    cfg = tlc.parse_cfg(BASE + "INVARIANT Never TypeOK Small\n")
    rest, user = tlc.split_user_invariants(cfg, d)
    assert rest["invariants"] == ["TypeOK"] and list(user) == ["Never", "Small"]
    assert tlc.model_from_cfg(rest)["invariants"] == 1
    # a definition that shares a built-in's name does not replace it; no -defs: nothing changes
    rest, user = tlc.split_user_invariants(tlc.parse_cfg(BASE + "INVARIANT TypeOK\n"), {"TypeOK": "TRUE"})
    assert user == {} and rest["invariants"] == ["TypeOK"]
    cfg = tlc.parse_cfg(BASE + "INVARIANT TypeOK\n")
    assert tlc.split_user_invariants(cfg, None) == (cfg, {})


def test_a_name_found_nowhere_is_the_error_it_always_was():
    cfg = tlc.parse_cfg(BASE + "INVARIANT TypeOK Nowhere\n")
    with pytest.raises(CfgError) as old:
        tlc.model_from_cfg(cfg)
    rest, user = tlc.split_user_invariants(cfg, pred.parse_definitions(DEFS))
    assert user == {}
    with pytest.raises(CfgError) as new:
        tlc.check_from_cfg(rest)
    assert str(new.value) == str(old.value) and "unknown invariant(s) ['Nowhere']" in str(old.value)


@pytest.mark.parametrize("extra,kw,words", [
    ("", dict(simulate=True), "-simulate"),
    ("PROPERTY ReconcileCompletes\n", {}, "PROPERTY list"),
    ("PROPERTY NoBlindUpdate\n", {}, "PROPERTY list"),
    ("SYMMETRY SymClients\n", {}, "SYMMETRY"),
    ("CONSTRAINT StoredAtMost1\n", {}, "constraint discards"),
    ("ACTION_CONSTRAINT ServeClientsFirst\n", {}, "CONSTRAINT / ACTION_CONSTRAINT"),
    ("", dict(coverage=True), "-coverage"),
    ("", dict(checkpointing=True), "-checkpoint / -recover"),
])
def test_refused_combinations(extra, kw, words):
    cfg = tlc.parse_cfg(BASE + "INVARIANT TypeOK Small\n" + extra)
    with pytest.raises(CfgError) as e:
        tlc.split_user_invariants(cfg, pred.parse_definitions(DEFS), **kw)
    assert words in str(e.value) and "Small" in str(e.value)
    # the same cfg without the user invariant is not this function's business
    cfg = tlc.parse_cfg(BASE + "INVARIANT TypeOK\n" + extra)
    assert tlc.split_user_invariants(cfg, pred.parse_definitions(DEFS), **kw)[1] == {}


def test_a_predicate_that_does_not_compile_is_a_cfg_error():
    cfg = tlc.parse_cfg(BASE + "INVARIANT Never\n")
    d = pred.parse_definitions(DEFS)
    with pytest.raises(CfgError, match="Never: the model .* has no process 'Client'"):
        tlc.split_user_invariants(cfg, d, procs=(2, 1, 1))
    with pytest.raises(CfgError, match="Bad: wrong type"):
        tlc.split_user_invariants(tlc.parse_cfg(BASE + "INVARIANT Bad\n"), {"Bad": 'pc["Client"] = "Ok"'})
    nine = {f"I{k}": "TRUE" for k in range(9)}
    with pytest.raises(CfgError, match="at most 8"):
        tlc.split_user_invariants(tlc.parse_cfg(BASE + "INVARIANT " + " ".join(nine) + "\n"), nine)


def test_main_reports_before_any_gpu_work(tmp_path, capsys):
    cfg = tmp_path / "m.cfg"
    cfg.write_text(BASE + "INVARIANT Small\nSYMMETRY SymClients\n")
    defs = tmp_path / "m.tla"
    defs.write_text(DEFS)
    with pytest.raises(CfgError, match="SYMMETRY"):
        tlc.main(["-config", str(cfg), "-defs", str(defs), "-nc", "2", "MC"])
    assert tlc.main(["-config", str(cfg), "-defs", str(tmp_path / "none.tla"), "MC"]) == 1
    assert "cannot read the definitions" in capsys.readouterr().err
    assert tlc.parse_args(["-config", "x.cfg", "-defs", "d.tla"]).defs == "d.tla"
    assert tlc.parse_args(["-config", "x.cfg"]).defs is None
