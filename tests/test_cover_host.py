"""Expression-level coverage on the host (no GPU): the independent model
(tests/cover_model.py) and Spec.cover against TLC's recorded coverage block
(tests/golden/model1_coverage.json, written by tools/make_coverage_golden.py)
through tlc.COVERAGE_LINES, the 33 counters the oracle also keeps, the rendered
-tool block, and the C-ABI's refusals."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import cover_model
import kubecheck
import pyoracle
from kubecheck import tlc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "model1_coverage.json")))
SUMS = json.load(open(os.path.join(ROOT, "tests", "golden", "model1_cover_sums.json")))
FIVE = {675, 783, 828, 966, 981}      # the cost figures the issue leaves underived (MC.out lines)


def result_of(ref):
    """What tlc.messages reads of a CheckResult, from an oracle run."""
    return types.SimpleNamespace(
        init=ref["init"], generated=ref["generated"], distinct=ref["distinct"], depth=ref["depth"],
        queue_left=ref["queue_left"], error=None, act_gen=ref["act_gen"], act_dist=ref["act_dist"],
        outdeg_hist=ref["newdeg_hist"][:16])


def sums_over(cfg, model, levels, spec=None):
    """(cover_model, Spec.cover) summed over the oracle's states of `levels`."""
    tot, tot_spec = {}, {}
    for lv in levels:
        t = pyoracle.level_tuples(cfg, lv)
        tot = cover_model.add(tot, cover_model.cover(t, *model))
        if spec is not None:
            tot_spec = cover_model.add(tot_spec, spec.cover(t))
    return tot, tot_spec


class Model1:
    def __init__(self):
        self.cfg = pyoracle.config(keep_trace=False)
        self.ref = pyoracle.run(self.cfg)
        spec = kubecheck.Spec(kubecheck.ModelConfig())
        self.model, self.spec = sums_over(self.cfg, (1, 1, 1), range(1, self.ref["depth"] + 1), spec)
        self.r = result_of(self.ref)


@pytest.fixture(scope="module")
def m1():
    return Model1()


def test_names_are_the_models():
    assert kubecheck.cover_names() == cover_model.NAMES
    assert kubecheck.load().kc_cover_count() == len(cover_model.NAMES)
    assert kubecheck.load().kc_cover_name(-1) is None
    assert kubecheck.load().kc_cover_name(len(cover_model.NAMES)) is None


def test_table_has_the_goldens_rows():
    assert len(tlc.COVERAGE_LINES) == len(GOLDEN) == 348
    for row, e in zip(tlc.COVERAGE_LINES, GOLDEN):
        assert (row[0], row[1], list(row[2])) == (e["code"], e["depth"], e["span"]), e["mcout_line"]
        if e["code"] in (2773, 2772, 2774):
            assert row[3] == e["name"]
    by = {c: sum(1 for e in GOLDEN if e["code"] == c) for c in (2221, 2775, 2774, 2772, 2773)}
    assert by == {2221: 315, 2775: 8, 2774: 2, 2772: 22, 2773: 1}
    # spans of the action heads are the ones the plain block prints
    heads = {row[3]: row[2] for row in tlc.COVERAGE_LINES if row[0] == 2772}
    assert heads == tlc.ACTION_SPANS


def test_unknown_costs_are_among_the_five():
    unknown = {e["mcout_line"] for row, e in zip(tlc.COVERAGE_LINES, GOLDEN) if row[0] == 2775 and row[4] is None}
    assert unknown == set(tlc.COVERAGE_COST_UNKNOWN)
    assert unknown <= FIVE


def test_model1_counts_equal_tlc(m1):
    assert m1.model["states"] == 163408
    vals = tlc.coverage_values(m1.r, m1.model)
    bad = []
    for (code, depth, span, name, count, cost), e in zip(vals, GOLDEN):
        if count != e["count"]:
            bad.append((e["mcout_line"], "count", count, e["count"]))
        # (a 2772 head's first number is the action's distinct count: TLC's own, from its
        # worker interleaving; ours is the engine's, as without the flag)
        if e["code"] != 2772 and e["mcout_line"] not in tlc.COVERAGE_COST_UNKNOWN and cost != e["cost"]:
            bad.append((e["mcout_line"], "cost", cost, e["cost"]))
    assert not bad, bad


def test_spec_cover_equals_model(m1):
    assert m1.spec == m1.model


def test_recorded_sums_are_the_models(m1):
    # the fixture the GPU tests compare the device vector with
    assert SUMS == m1.model


def oracle_subset(ref):
    want = {"B_" + k: v for k, v in ref["branch"].items()}
    want.update({"cov_" + k: v for k, v in ref["cov"].items()})
    return want


def test_model1_subset_equals_oracle(m1):
    want = oracle_subset(m1.ref)
    assert len(want) == 33
    assert {k: m1.model[k] for k in want} == want


@pytest.mark.parametrize("model,max_levels", [((2, 1, 1), None), ((1, 2, 1), 31)])
def test_subset_equals_oracle(model, max_levels):
    nc, np_, ns = model
    if max_levels is None:
        # nc=2 ends in an error: the levels before the one it is found in
        err = pyoracle.run(pyoracle.config(nc, np_, ns, keep_trace=False))
        assert err["err_kind"] != 0
        max_levels = err["err_level"] - 1
    cfg = pyoracle.config(nc, np_, ns, keep_trace=False, max_levels=max_levels)
    ref = pyoracle.run(cfg)
    assert ref["err_kind"] == 0
    spec = kubecheck.Spec(kubecheck.ModelConfig(nc=nc, np=np_, ns=ns))
    got, got_spec = sums_over(cfg, model, range(1, max_levels), spec)
    want = oracle_subset(ref)
    assert {k: got[k] for k in want} == want
    assert got_spec == got
    assert got["states"] == sum(ref["level_width"][:max_levels - 1])
    # (state, self) pairs and act_gen: equal wherever an action has one successor per pair
    for a in ("C1", "C10", "C11", "c12", "C13", "C2", "C3", "C8", "C7", "C4", "C5", "PVCStart", "PVCListedPVCs",
              "PVCDone"):
        assert got["pairs_" + a] == ref["act_gen"][a], a
    assert 2 * got["pairs_CStart"] == ref["act_gen"]["CStart"]
    assert 3 * got["pairs_DoRequest"] == ref["act_gen"]["DoRequest"]
    assert 2 * got["en_DoReply"] == ref["act_gen"]["DoReply"]


def golden_body(e, with_cost=True, act_dist=None):
    """The message body MC.out holds for a golden entry; act_dist: the distinct
    half of a 2772 head from the run at hand (as without the flag)."""
    l1, c1, l2, c2 = e["span"]
    span = f"line {l1}, col {c1} to line {l2}, col {c2} of module KubeAPI"
    if e["code"] == 2772:
        return f"<{e['name']} {span}>: {act_dist[e['name']]}:{e['count']}"
    if e["code"] == 2773:
        return f"<{e['name']} {span}>: {e['cost']}:{e['count']}"
    if e["code"] == 2774:
        return f"<{e['name']} {span}>"
    body = f"  {'|' * e['depth']}{span}: {e['count']}"
    return f"{body}:{e['cost']}" if e["code"] == 2775 and with_cost else body


def coverage_block(msgs):
    codes = [m[0] for m in msgs]
    return msgs[codes.index(2201) + 1:codes.index(2202)]


def test_messages_reproduce_the_coverage_block(m1):
    msgs = tlc.messages(m1.r, 0.0, 1.0, coverage=m1.model)
    block = coverage_block(msgs)
    assert len(block) == len(GOLDEN)
    for (code, cls, body), e in zip(block, GOLDEN):
        assert (code, cls) == (e["code"], 0)
        assert body == golden_body(e, e["mcout_line"] not in tlc.COVERAGE_COST_UNKNOWN, m1.r.act_dist), e["mcout_line"]
    # the rest of the stream is what it is without the flag
    plain = tlc.messages(m1.r, 0.0, 1.0)
    strip = lambda ms: [m for m in ms if m not in coverage_block(ms)]  # noqa: E731
    assert strip(msgs) == strip(plain)


def test_messages_without_the_flag_are_unchanged(m1):
    block = coverage_block(tlc.messages(m1.r, 0.0, 1.0))
    want = [(2773, 0, f"<Init line 455, col 1 to line 455, col 4 of module KubeAPI>: {m1.r.init}:{m1.r.init}")]
    for e in GOLDEN:
        if e["code"] == 2772:
            want.append((2772, 0, golden_body(e, act_dist=m1.r.act_dist)))
    assert block == want


def test_cli_flag_and_refusals():
    a = tlc.parse_args(["-coverage", "-tool", "MC"])
    assert a.coverage and a.tool and a.spec == "MC"
    a = tlc.parse_args(["-coverage", "3", "-config", "x.cfg"])     # TLC's minutes: accepted, ignored
    assert a.coverage and a.config == "x.cfg" and a.spec == "MC"
    assert not tlc.parse_args(["-tool"]).coverage
    with pytest.raises(tlc.CfgError):
        tlc.parse_args(["-coverage", "-simulate"])
    base = "CONSTANT REQUESTS_CAN_FAIL = TRUE REQUESTS_CAN_TIMEOUT = TRUE\nSPECIFICATION Spec\n"
    with pytest.raises(tlc.CfgError):
        tlc.check_from_cfg(tlc.parse_cfg(base + "PROPERTY ReconcileCompletes"), coverage=True)
    with pytest.raises(tlc.CfgError):
        tlc.check_from_cfg(tlc.parse_cfg(base + "SYMMETRY SymControllers"), coverage=True)
    with pytest.raises(tlc.CfgError):
        tlc.check_from_cfg(tlc.parse_cfg(base), simulate=True, coverage=True)
    kw, props = tlc.check_from_cfg(tlc.parse_cfg(base + "INVARIANT TypeOK"), coverage=True)
    assert kw["invariants"] == 1 and props == []


def test_abi_symbols_and_bad_arguments():
    lib = kubecheck.load()
    for sym in ("kc_engine_set_coverage", "kc_engine_coverage", "kc_spec_cover", "kc_cover_count", "kc_cover_name"):
        assert hasattr(lib, sym), sym
    n = lib.kc_cover_count()
    out = (C.c_uint64 * n)()
    cfg = kubecheck.ModelConfig().to_c()
    t = np.zeros(1 + 19 * 3, dtype=np.uint64)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    assert lib.kc_spec_cover(None, u64(t), 1, out) == -22
    assert lib.kc_spec_cover(C.byref(cfg), None, 1, out) == -22
    assert lib.kc_spec_cover(C.byref(cfg), u64(t), 1, None) == -22
    assert lib.kc_spec_cover(C.byref(cfg), u64(t), 1, out) == -22          # a server's pc is not APIStart
    assert b"tuple 0" in lib.kc_last_error()
    bad = kubecheck.ModelConfig(nc=3, np=3, ns=1).to_c()
    assert lib.kc_spec_cover(C.byref(bad), u64(t), 0, out) == -22
    assert lib.kc_spec_cover(C.byref(cfg), None, 0, out) == 0 and list(out) == [0] * n
    assert lib.kc_engine_set_coverage(None, 1) == -22
    assert lib.kc_engine_coverage(None, out, n) == -22
    init = kubecheck.Spec(kubecheck.ModelConfig()).init()
    got = kubecheck.Spec(kubecheck.ModelConfig()).cover(init)
    assert got == cover_model.cover(init)
    assert got["states"] == 2 and got["pairs_CStart"] == 2 and got["B_CSTART_THEN"] == 3
