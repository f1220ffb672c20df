"""Liveness checking without a GPU: kc_live_stay against the independent model
(tests/live_model.py), the model's own terminal / self-loop rule, the new
structs and argument checks of the C ABI, the cfg handling and the message
formatter of the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kubecheck
from kubecheck import ModelConfig, Spec, _lib, tlc

import live_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_HEAD = "CONSTANT REQUESTS_CAN_FAIL = TRUE REQUESTS_CAN_TIMEOUT = TRUE\n"

# the graphs' sizes as literals (tests/test_gpu_liveness.py has the whole table):
# name -> (states, edges, depth)
GRAPHS = {"default_101": (207, 378, 34), "nodeadlock_110": (140, 479, 15), "nofaults_111": (8203, 17018, 109)}


def test_properties_names():
    assert kubecheck.PROPERTIES == live_model.PROPERTIES == (
        "ReconcileCompletes", "CleansUpProperly", "ClientRestarts", "SomeActorRestarts")


@pytest.mark.parametrize("name", list(live_model.MODELS))
def test_stay_matches_model(oracle, name):
    m = live_model.model(oracle, name)
    assert (len(m.states), m.edges, m.depth) == GRAPHS[name]
    assert m.self_loops == 0 and m.assert_action is None
    sp = Spec(ModelConfig(**live_model.MODELS[name]))
    for p, pname in enumerate(live_model.PROPERTIES):
        want = [m.stay(p, t) for t in m.states]
        got = [sp.stay(p, np.array(t, dtype=np.uint64)) for t in m.states]
        assert got == want, pname
        # by name too
        assert sp.stay(pname, np.array(m.states[0], dtype=np.uint64)) == want[0]
    # the predicates are not degenerate on the largest model
    if name == "nofaults_111":
        assert [sum(m.stay(p, t) for t in m.states) for p in range(4)] == [7398, 427, 7591, 6545]


def test_stay_errors():
    lib = kubecheck.load()
    for flags in (dict(nc=2, np=0), dict(nc=2, np=1), dict(nc=0, np=1)):
        sp = Spec(ModelConfig(**flags))
        t = sp.init()[0]
        for p in (0, 1, 2):
            with pytest.raises(kubecheck.KubecheckError) as e:
                sp.stay(p, t)
            assert e.value.code == -22 and "property" in str(e.value)
        assert sp.stay(3, t) is False           # every actor is at its start label in Init
    sp = Spec(ModelConfig())
    for p in (-1, 4, 99):
        with pytest.raises(kubecheck.KubecheckError) as e:
            sp.stay(p, sp.init()[0])
        assert e.value.code == -22
    assert lib.kc_live_stay(None, 0, None) == -22
    bad = sp.init()[0].copy()
    bad[0] = 1 << 40                              # apiState outside the object universe
    with pytest.raises(kubecheck.KubecheckError):
        sp.stay(0, bad)


def test_model_self_loops_and_terminal_rule():
    # 0 -> 0, 1 ; 1 -> 1 ; 2 -> 2, 3 ; 3 -> 2 ; 4 -> (nothing) ; 5 -> 1 (not alive below)
    succ = [[0, 1], [1], [2, 3], [2], [], [1]]
    # 1 and 4 are terminal (no successor other than themselves); 0's self-loop does not keep it
    L, terminal, rounds = live_model.eliminate(succ, {0, 2, 3, 4})
    assert terminal == {1, 4}
    assert L == {2, 3, 4} and rounds == 2
    # with 1 alive, 0 has a successor in L
    L, _, rounds = live_model.eliminate(succ, {0, 1, 5})
    assert L == {0, 1, 5} and rounds == 1
    # a chain dies from its end, one state per Jacobi round
    chain = [[1], [2], [3], [4], [4, 5], [5]]
    L, terminal, rounds = live_model.eliminate(chain, {0, 1, 2, 3})
    assert terminal == {5} and L == set() and rounds == 5


@pytest.mark.skipif(kubecheck.device_count() > 0, reason="checks the no-GPU failure mode")
def test_create_without_gpu_is_enodev():
    with pytest.raises(kubecheck.KubecheckError) as e:
        kubecheck.LivenessChecker(ModelConfig(), "ReconcileCompletes")
    assert e.value.code == -19 and "no CPU fallback" in str(e.value)


def test_create_argument_checks():
    lib = kubecheck.load()
    h = C.c_void_p()
    assert lib.kc_live_create(None, None, C.byref(h)) == -22
    assert b"NULL" in lib.kc_last_error()
    c = ModelConfig().to_c()
    for prop, ms in ((4, 0), (-1, 0), (0, 8), (0, 2**27 + 1)):
        l = _lib.KcLiveConfig(prop, ms)
        assert lib.kc_live_create(C.byref(c), C.byref(l), C.byref(h)) == -22, (prop, ms)
        assert not h.value
    c2 = ModelConfig(nc=2, np=0).to_c()
    l = _lib.KcLiveConfig(1, 0)
    assert lib.kc_live_create(C.byref(c2), C.byref(l), C.byref(h)) == -22
    assert b"property" in lib.kc_last_error()
    assert lib.kc_live_run(None, None) == -22
    assert lib.kc_live_trace(None, None, None, 0) == -22
    assert lib.kc_live_alive(None, None, None, 0) == -22
    with pytest.raises(ValueError):
        kubecheck.LivenessChecker(ModelConfig(), "NoSuchProperty")


def test_struct_layouts_match_header(tmp_path):
    structs = {"kc_live_config": _lib.KcLiveConfig, "kc_live_result": _lib.KcLiveResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kubecheck.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                         check=True).stdout.split("\n") if l)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f in py._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(py, f[0]).offset, (cname, f[0])


def test_check_from_cfg():
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Liveness.cfg")).read())
    kw, props = tlc.check_from_cfg(cfg)
    assert props == ["ReconcileCompletes", "CleansUpProperly"]
    plain = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Model_1.cfg")).read())
    assert kw == tlc.model_from_cfg(plain) == dict(can_fail=True, can_timeout=True, invariants=3)
    assert tlc.check_from_cfg(plain) == (kw, [])
    # the build-defined properties, in cfg order
    _, props = tlc.check_from_cfg(tlc.parse_cfg(CFG_HEAD + "PROPERTIES SomeActorRestarts ClientRestarts"))
    assert props == ["SomeActorRestarts", "ClientRestarts"]
    with pytest.raises(tlc.CfgError, match="Termination"):
        tlc.check_from_cfg(tlc.parse_cfg(CFG_HEAD + "PROPERTY ReconcileCompletes Termination"))
    with pytest.raises(tlc.CfgError, match="simulate"):
        tlc.check_from_cfg(cfg, simulate=True)
    assert tlc.check_from_cfg(plain, simulate=True) == (kw, [])
    # the other checks of model_from_cfg still apply
    with pytest.raises(tlc.CfgError):
        tlc.check_from_cfg(tlc.parse_cfg(CFG_HEAD + "INVARIANT Nope\nPROPERTY ReconcileCompletes"))


def test_model_from_cfg_still_refuses_properties():
    cfg = tlc.parse_cfg(open(os.path.join(ROOT, "models", "Liveness.cfg")).read())
    with pytest.raises(tlc.CfgError, match="out of scope"):
        tlc.model_from_cfg(cfg)


def _result(**kw):
    base = dict(property="ReconcileCompletes", states=3, edges=3, init=1, depth=3, stay_states=2, live_states=2,
                live_terminal=0, rounds=1, error=None, error_action=None, error_self=-1, violated=True,
                kind="back-to-state", prefix_len=2, trace_len=3, loop_start=1, seconds=0.0, build_ms=0.0,
                trim_ms=0.0, trace_text="State 1:\n/\\ a = 1\n/\\ b = 2\nState 2:\n/\\ a = 2\nState 3:\n/\\ a = 3\n")
    base.update(kw)
    return kubecheck.LiveResult(**base)


def test_live_messages():
    out = tlc.live_messages(_result())
    assert [c for c, _, _ in out] == [2116, 2264, 2217, 2217, 2217, 2122]
    assert out[0][2] == "Temporal properties were violated."
    assert out[1][2] == "The following behavior constitutes a counter-example:"
    assert out[2][2] == "1: /\\ a = 1\n/\\ b = 2" and out[4][2] == "3: /\\ a = 3"
    assert out[5] == (2122, 4, "4: Back to state 2")
    out = tlc.live_messages(_result(kind="stuttering", loop_start=-1))
    assert [c for c, _, _ in out] == [2116, 2264, 2217, 2217, 2217, 2218]
    assert out[5] == (2218, 4, "4: Stuttering")
    text = tlc.msg(*[out[5][0], out[5][2], out[5][1]], tool=True)
    assert text.startswith("@!@!@STARTMSG 2218:4 @!@!@") and text.endswith("@!@!@ENDMSG 2218 @!@!@")
