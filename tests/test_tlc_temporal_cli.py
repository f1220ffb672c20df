"""The command line's user-defined temporal properties: without a GPU the
-defs / cfg parsing, the split of a PROPERTY list and every CfgError; on the
GPU (marked) models/Eventually.cfg, a cfg whose properties all hold, and a cfg
that mixes a built-in and a user property."""
import os
import re
import subprocess
import sys

import pytest

from kubecheck import PROPERTIES, pred, tlc
from kubecheck.tlc import CfgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = """CONSTANT defaultInitValue = defaultInitValue
CONSTANT REQUESTS_CAN_FAIL = FALSE
CONSTANT REQUESTS_CAN_TIMEOUT = FALSE
SPECIFICATION Spec
INVARIANT TypeOK OnlyOneVersion
"""
DEFS = """---- MODULE Mine ----
Done == pc["Client"] = "C5" ~> ~shouldReconcile["Client"]   \\* a trailing comment with <> in it
Boxed ==
    [](pc["Client"] = "C2" =>
        <>(pc["Client"] = "CStart"))
Often == []<>(pc["Client"] = "CStart")
Once == <>(~shouldReconcile["Client"])
Small == Cardinality(apiState) <= 2
Never == <>[](pc["Client"] = "C5")
Always == [](pc["Client"] # "C5")
Twice == pc["Client"] = "C1" ~> pc["Client"] = "C2" ~> pc["Client"] = "C3"
Nested == pc["Client"] = "C1" ~> (<>(pc["Client"] = "C2"))
Typo == pc["Client"] = "Ok" ~> TRUE
====
"""


def defs():
    return pred.parse_definitions(DEFS)


def test_definitions_keep_their_temporal_operators():
    d = defs()
    assert list(d)[:5] == ["Done", "Boxed", "Often", "Once", "Small"]
    assert pred.parse_temporal(d["Boxed"]) == pred.parse_temporal('pc["Client"] = "C2" ~> pc["Client"] = "CStart"')
    assert pred.parse_temporal(d["Done"])[0] == 0 and pred.parse_temporal(d["Once"])[0] == 1
    assert [pred.has_temporal(d[k]) for k in ("Done", "Boxed", "Often", "Once", "Small")] == [True] * 4 + [False]


def test_shipped_eventually_files():
    d = pred.parse_definitions(open(os.path.join(ROOT, "models", "Eventually.tla")).read())
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Eventually.cfg")).read())
    assert cfg["properties"] == ["DoneIsReconciled", "C2Restarts"]
    user = tlc.split_user_properties(cfg, d)
    assert list(user) == ["DoneIsReconciled", "C2Restarts"]
    kw, props = tlc.check_from_cfg(cfg, user_props=user)
    assert kw == {"can_fail": False, "can_timeout": False, "invariants": 3} and props == cfg["properties"]
    for text in d.values():
        pred.compile_temporal(text)
    assert pred.parse_temporal(d["C2RestartsBoxed"]) == pred.parse_temporal(d["C2Restarts"])


def test_split_keeps_cfg_order_built_ins_and_action_properties():
    cfg = tlc.parse_cfg(BASE + "PROPERTY Often ReconcileCompletes NoBlindUpdate Done Often\n")
    user = tlc.split_user_properties(cfg, defs())
    assert list(user) == ["Often", "Done"]
    kw, props = tlc.check_from_cfg(cfg, user_props=user)
    assert props == ["Often", "ReconcileCompletes", "Done", "Often"]            # cfg order, the action property aside
    assert kw["action_properties"] == ("NoBlindUpdate",)
    # a definition that shares a built-in's name does not replace it; no -defs: nothing changes
    cfg = tlc.parse_cfg(BASE + "PROPERTY ClientRestarts\n")
    assert tlc.split_user_properties(cfg, {"ClientRestarts": "<>TRUE"}) == {}
    assert tlc.split_user_properties(cfg, None) == {}
    assert tlc.check_from_cfg(cfg)[1] == ["ClientRestarts"]
    assert "ClientRestarts" in PROPERTIES


def test_a_name_found_nowhere_is_the_unknown_property_error():
    cfg = tlc.parse_cfg(BASE + "PROPERTY Done Nowhere\n")
    user = tlc.split_user_properties(cfg, defs())
    assert list(user) == ["Done"]
    with pytest.raises(CfgError, match=r"unknown temporal property\(ies\) \['Nowhere'\]"):
        tlc.check_from_cfg(cfg, user_props=user)
    with pytest.raises(CfgError, match=r"unknown temporal property\(ies\) \['Done', 'Nowhere'\]"):
        tlc.check_from_cfg(cfg)                                                  # without -defs both are unknown


@pytest.mark.parametrize("name,words", [
    ("Small", ["PROPERTY Small", "no temporal operator", "INVARIANT"]),
    ("Never", ["PROPERTY Never", "<>[]", "SCC"]),
    ("Always", ["PROPERTY Always", "[]P", "INVARIANT"]),
    ("Twice", ["PROPERTY Twice", "more than one temporal operator"]),
    ("Nested", ["PROPERTY Nested", "inside an operand"]),
    ("Typo", ["PROPERTY Typo", "wrong type"]),
])
def test_a_definition_that_is_no_supported_formula_is_a_cfg_error(name, words):
    cfg = tlc.parse_cfg(BASE + f"PROPERTY Done {name}\n")
    with pytest.raises(CfgError) as e:
        tlc.split_user_properties(cfg, defs())
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_a_formula_that_does_not_compile_for_the_model_is_a_cfg_error():
    cfg = tlc.parse_cfg(BASE + "PROPERTY Done\n")
    with pytest.raises(CfgError, match="PROPERTY Done: the model .* has no process 'Client'"):
        tlc.split_user_properties(cfg, defs(), procs=(2, 1, 1))


@pytest.mark.parametrize("extra,kw,words", [
    ("", dict(simulate=True), "-simulate checks no temporal PROPERTY"),
    ("SYMMETRY SymClients\n", {}, "SYMMETRY SymClients with a PROPERTY list"),
    ("CONSTRAINT StoredAtMost1\n", {}, "with a PROPERTY list"),
    ("ACTION_CONSTRAINT ServeClientsFirst\n", {}, "with a PROPERTY list"),
    ("", dict(coverage=True), "-coverage with a PROPERTY list"),
    ("", dict(checkpointing=True), "-checkpoint / -recover with a PROPERTY list"),
])
def test_the_refusals_of_a_property_list_stay(extra, kw, words):
    cfg = tlc.parse_cfg(BASE + "PROPERTY Done\n" + extra)
    user = tlc.split_user_properties(cfg, defs())
    assert list(user) == ["Done"]
    with pytest.raises(CfgError) as e:
        tlc.check_from_cfg(cfg, user_props=user, **kw)
    assert words in str(e.value)


def test_user_invariants_with_a_user_property_are_refused():
    # the refusal itself is split_user_invariants' own and older than user properties; what is new is that the
    # PROPERTY list it meets may hold a user formula, which split_user_properties accepts on the same cfg
    cfg = tlc.parse_cfg(BASE.replace("OnlyOneVersion", "OnlyOneVersion Small") + "PROPERTY Done\n")
    assert list(tlc.split_user_properties(cfg, defs())) == ["Done"]
    with pytest.raises(CfgError, match=r"user-defined INVARIANT \(Small\) with a PROPERTY list"):
        tlc.split_user_invariants(cfg, defs())


def test_main_reports_before_any_gpu_work(tmp_path):
    cfg = tmp_path / "m.cfg"
    cfg.write_text(BASE + "PROPERTY Done Small\n")
    d = tmp_path / "m.tla"
    d.write_text(DEFS)
    with pytest.raises(CfgError, match="PROPERTY Small: its definition has no temporal operator"):
        tlc.main(["-config", str(cfg), "-defs", str(d), "MC"])
    cfg.write_text(BASE + "PROPERTY Done\n")
    with pytest.raises(CfgError, match="unknown temporal property"):
        tlc.main(["-config", str(cfg), "MC"])                                   # no -defs
    assert "User-defined temporal properties" in tlc.__doc__


# ---------------------------------------------------------------- on the GPU
def _cli(cfg_path, defs_path, *more):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tla-kubernetes_amd"))
    p = subprocess.run([sys.executable, "-m", "kubecheck.tlc", "-tool", "-config", str(cfg_path), "-defs",
                        str(defs_path), *more, "MC"], capture_output=True, text=True, env=env, timeout=300)
    codes = [int(c) for c in re.findall(r"@!@!@STARTMSG (\d+):\d+ @!@!@", p.stdout)]
    return p, codes


def _checked(stdout):
    return re.findall(r"Checking temporal property (\w+) under", stdout)


@pytest.mark.gpu
def test_cli_eventually_cfg():
    p, codes = _cli(os.path.join(ROOT, "models", "Eventually.cfg"), os.path.join(ROOT, "models", "Eventually.tla"))
    assert p.returncode == 13, p.stderr
    assert "17020 states generated, 8203 distinct states found, 0 states left on queue." in p.stdout
    assert "No error has been found" in p.stdout
    # the first property holds, the second is violated and ends the run
    assert _checked(p.stdout) == ["DoneIsReconciled", "C2Restarts"]
    assert codes.count(2192) == 2 and codes.count(2116) == 1 and codes.count(2264) == 1 and codes[-1] == 2186
    at = codes.index(2116)
    assert codes[at - 1] == 2192 and codes[at + 1] == 2264
    tail = codes[at + 2:-1]
    assert set(tail[:-1]) == {2217} and tail[-1] in (2122, 2218)
    last = re.search(r"STARTMSG (2122|2218):4 @!@!@\n(\d+): (Back to state (\d+)|Stuttering)\n", p.stdout)
    n = len(tail) - 1
    assert last and int(last.group(2)) == n + 1 and n >= 24              # the prefix alone has 24 states
    if last.group(4):
        assert 24 <= int(last.group(4)) <= n                             # the cycle lies behind the trigger state
    # state 24 is the first with the client at C2 that can stay away from CStart for ever
    states = re.findall(r"STARTMSG 2217:4 @!@!@\n(\d+): .*?/\\ pc = \((.*?)\)", p.stdout, flags=re.S)
    assert len(states) == n and [int(k) for k, _ in states] == list(range(1, n + 1))
    assert states[23][1].startswith('"Client" :> "C2"')
    assert all(not pc.startswith('"Client" :> "CStart"') for _, pc in states[23:])


@pytest.mark.gpu
def test_cli_exits_0_when_everything_listed_holds(tmp_path):
    cfg = tmp_path / "holds.cfg"
    cfg.write_text(BASE + "PROPERTY DoneIsReconciled\n")
    p, codes = _cli(cfg, os.path.join(ROOT, "models", "Eventually.tla"))
    assert p.returncode == 0, p.stderr
    assert _checked(p.stdout) == ["DoneIsReconciled"] and 2116 not in codes and codes[-1] == 2186
    # under per-process fairness nobody is starved: the shipped cfg's two properties both hold
    p, codes = _cli(os.path.join(ROOT, "models", "Eventually.cfg"), os.path.join(ROOT, "models", "Eventually.tla"),
                    "-fairness", "process")
    assert p.returncode == 0, p.stderr
    assert _checked(p.stdout) == ["DoneIsReconciled", "C2Restarts"] and 2116 not in codes
    assert p.stdout.count("under weak fairness of every process") == 2


@pytest.mark.gpu
def test_cli_mixes_built_in_and_user_properties_in_cfg_order(tmp_path):
    # a user property that holds, then a built-in that is violated, then one never reached
    cfg = tmp_path / "mixed.cfg"
    cfg.write_text(BASE + "PROPERTY DoneIsReconciled ClientRestarts C2Restarts\n")
    p, codes = _cli(cfg, os.path.join(ROOT, "models", "Eventually.tla"))
    assert p.returncode == 13, p.stderr
    assert _checked(p.stdout) == ["DoneIsReconciled", "ClientRestarts"] and codes.count(2116) == 1
    # a built-in that holds, then the user property that is violated
    cfg.write_text(BASE + "PROPERTY SomeActorRestarts C2Restarts\n")
    p, codes = _cli(cfg, os.path.join(ROOT, "models", "Eventually.tla"))
    assert p.returncode == 13, p.stderr
    assert _checked(p.stdout) == ["SomeActorRestarts", "C2Restarts"] and codes.count(2116) == 1
    assert codes.index(2116) > [i for i, c in enumerate(codes) if c == 2192][1]
