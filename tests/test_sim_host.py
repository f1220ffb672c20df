"""Simulation mode without a GPU: the RNG's host copies, kc_sim_replay against
the independent model (tests/sim_model.py), the new structs and argument
checks of the C ABI, and the command line's parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kubecheck
from kubecheck import ModelConfig, Spec, _lib, tlc

import sim_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = [0, 1, 2**32, 2**63, 2**64 - 1]

# the configurations of the GPU error cases (tests/test_gpu_simulate.py): (flags, depth)
CONFIGS = [
    (dict(nc=2), 64),
    (dict(variant=2), 128),
    (dict(variant=1, invariants=7), 128),
    (dict(np=2, variant=1, invariants=7), 128),
    (dict(variant=4), 64),
    (dict(variant=5), 8),
    (dict(ns=0), 32),
    (dict(ns=0, check_deadlock=False), 32),
]


def test_rng_matches_formula():
    for seed in EDGE:
        for w in EDGE:
            for k in EDGE:
                assert Spec.sim_rand(seed, w, k) == sim_model.rand(seed, w, k), (seed, w, k)
    # and away from the edges
    for i in range(200):
        seed, w, k = sim_model.mix(i), i * 7919, i % 130
        assert Spec.sim_rand(seed, w, k) == sim_model.rand(seed, w, k)
    # not degenerate: the words of one walk differ
    assert len({Spec.sim_rand(1, 0, k) for k in range(64)}) == 64


def test_pick_ends_and_formula():
    for n in (1, 2, 32):
        assert Spec.sim_pick(2**64 - 1, n) == n - 1
        assert Spec.sim_pick(0, n) == 0
    for i in range(200):
        r, n = sim_model.mix(i), 1 + i % 32
        assert Spec.sim_pick(r, n) == sim_model.pick(r, n) < n


@pytest.mark.parametrize("flags,depth", CONFIGS, ids=[str(c[0]) for c in CONFIGS])
def test_replay_matches_model(oracle, flags, depth):
    model = sim_model.Model(oracle, **flags)
    sp = Spec(ModelConfig(**flags))
    kinds = set()
    for w in range(64):
        want = model.walk(1, depth, w)
        states, actions, kind = sp.sim_replay(1, depth, w)
        assert kind == want.kind, w
        assert len(states) == want.length, w
        assert actions == want.actions, w
        for a, b in zip(states, want.states):
            assert tuple(int(x) for x in a) == b, w
        kinds.add(kind)
    assert "running" not in kinds


def test_replay_model1_has_no_error(oracle):
    model = sim_model.Model(oracle)
    sp = Spec(ModelConfig())
    for w in range(16):
        want = model.walk(1, 128, w)
        states, actions, kind = sp.sim_replay(1, 128, w)
        assert kind == want.kind == "depth" and len(states) == 128
        assert actions == want.actions
        assert tuple(int(x) for x in states[-1]) == want.states[-1]
    # a cap smaller than the walk: the count is still the walk's
    kind = C.c_int()
    c = ModelConfig().to_c()
    out = np.zeros((4, sp.tuple_words), dtype=np.uint64)
    n = kubecheck.load().kc_sim_replay(C.byref(c), 1, 128, 0, out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       None, 4, C.byref(kind))
    assert n == 128 and tuple(int(x) for x in out[3]) == model.walk(1, 128, 0).states[3]


def test_struct_layouts_match_header(tmp_path):
    """kc_sim_config and kc_sim_result: the ctypes mirrors have the header's
    sizes and offsets (the method of tests/test_abi.py)."""
    structs = {"kc_sim_config": _lib.KcSimConfig, "kc_sim_result": _lib.KcSimResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kubecheck.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append(f'  printf("KC_SIM_MAX_DEPTH %d\\n", KC_SIM_MAX_DEPTH);')
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
    assert int(got["KC_SIM_MAX_DEPTH"]) == _lib.KC_SIM_MAX_DEPTH == 65535


def _create(cfg, sim):
    h = C.c_void_p()
    rc = kubecheck.load().kc_sim_create(C.byref(cfg) if cfg is not None else None,
                                        C.byref(sim) if sim is not None else None, C.byref(h))
    if rc == 0:
        kubecheck.load().kc_sim_destroy(h)
    return rc


def test_bad_arguments_return_einval():
    lib = kubecheck.load()
    cfg = ModelConfig().to_c()
    good = dict(seed=1, num_walks=16, depth=8)
    assert lib.kc_sim_create(None, None, None) == -22
    assert b"NULL" in lib.kc_last_error()
    assert _create(None, _lib.KcSimConfig(**good)) == -22
    assert _create(cfg, None) == -22
    assert lib.kc_sim_create(C.byref(cfg), C.byref(_lib.KcSimConfig(**good)), None) == -22
    for bad in (dict(num_walks=0), dict(num_walks=2**30 + 1), dict(depth=0), dict(depth=-1),
                dict(depth=_lib.KC_SIM_MAX_DEPTH + 1), dict(steps_per_launch=-1)):
        assert _create(cfg, _lib.KcSimConfig(**dict(good, **bad))) == -22, bad
        assert lib.kc_last_error()
    bad_model = ModelConfig().to_c()
    bad_model.nc = 7
    assert _create(bad_model, _lib.KcSimConfig(**good)) == -22
    assert b"unsupported model" in lib.kc_last_error()
    assert lib.kc_sim_run(None, None) == -22
    assert lib.kc_sim_walks(None, None, None, None) == -22
    assert lib.kc_sim_trace(None, 0, None, None, 0) == -22
    assert lib.kc_sim_trace_text(None, 0, None, 0) == -22
    # the host replay checks its arguments too
    kind = C.c_int()
    assert lib.kc_sim_replay(None, 1, 8, 0, None, None, 0, C.byref(kind)) == -22
    assert lib.kc_sim_replay(C.byref(cfg), 1, 0, 0, None, None, 0, C.byref(kind)) == -22
    assert lib.kc_sim_replay(C.byref(cfg), 1, _lib.KC_SIM_MAX_DEPTH + 1, 0, None, None, 0, C.byref(kind)) == -22
    assert lib.kc_sim_replay(C.byref(bad_model), 1, 8, 0, None, None, 0, C.byref(kind)) == -22


@pytest.mark.skipif(kubecheck.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly():
    assert _create(ModelConfig().to_c(), _lib.KcSimConfig(seed=1, num_walks=16, depth=8)) == -19
    with pytest.raises(kubecheck.KubecheckError) as e:
        kubecheck.Simulator(seed=1, num_walks=16, depth=8)
    assert e.value.code == -19 and "no CPU fallback" in str(e.value)


def test_exports():
    for name in ("Simulator", "SimResult"):
        assert name in kubecheck.__all__ and hasattr(kubecheck, name)


def test_cli_parsing():
    a = tlc.parse_args(["-config", "x.cfg", "MC"])
    assert not a.simulate and a.spec == "MC" and a.config == "x.cfg"
    a = tlc.parse_args(["-simulate", "-config", "x.cfg", "MC"])
    assert a.simulate and a.num == 65536 and a.depth == 100 and a.seed is None and not a.cont
    assert a.spec == "MC" and a.config == "x.cfg"
    a = tlc.parse_args(["-config", "x.cfg", "-simulate", "MC"])        # the spec is not -simulate's argument
    assert a.simulate and a.num == 65536 and a.spec == "MC"
    a = tlc.parse_args(["-simulate", "num=100", "-depth", "7", "-seed", "42", "-continue", "-nc", "2"])
    assert (a.simulate, a.num, a.depth, a.seed, a.cont, a.nc) == (True, 100, 7, 42, True, 2)
    a = tlc.parse_args(["-simulate"])
    assert a.simulate and a.num == 65536
    for bad in ("num=", "num=abc", "num=0", "num=-3", "num=1.5", "nmu=5", "num=5,file=x"):
        with pytest.raises(tlc.CfgError):
            tlc.parse_args(["-simulate", bad])
        assert tlc.main(["-simulate", bad]) == 1
    with pytest.raises(tlc.CfgError):
        tlc.parse_args(["-simulate", "-depth", "0"])
    with pytest.raises(tlc.CfgError):
        tlc.parse_args(["-simulate", "-depth", "65536"])


def test_sim_messages_shape():
    """The message stream of a simulation result: the BFS's violation and
    coverage bodies, the steps per action in the place of both counts."""
    r = kubecheck.SimResult(
        steps=10, act_steps={a: i for i, a in enumerate(kubecheck.ACTIONS)}, walks_error=1, walks_depth=2,
        walks_terminated=0, distinct_visited=9, error="assertion", error_action="C4", error_self=0,
        error_invariant=None, trace_len=2, error_walk=3, seconds=0.5, kernel_ms=1.0, fpset_slots=64,
        trace_text="State 1:\n/\\ a = 1\n\nState 2:\n/\\ a = 2\n\n")
    msgs = tlc.sim_messages(r, 2, 1, 3, 64, 0.0, 0.5)
    codes = [c for c, _, _ in msgs]
    assert codes[:3] == [2262, 2187, 2185] and codes[-1] == 2186
    assert codes.count(2217) == 2 and codes.index(2132) < codes.index(2121) < codes.index(2217)
    assert codes.count(2772) == len(kubecheck.ACTIONS) and codes.count(2773) == 1
    bodies = {c: b for c, _, b in msgs}
    assert "seed 1" in bodies[2187] and "3 behaviors" in bodies[2187] and "64 states" in bodies[2187]
    assert bodies[2132] == "The first argument of Assert evaluated to FALSE (action C4)."
    assert [b for c, _, b in msgs if c == 2772][-1].endswith(": 21:21")
    assert "10 steps" in bodies[2210] and "9 distinct states visited" in bodies[2210]
