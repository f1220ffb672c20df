"""Expression-level coverage on the GPU: the engine's summed vector (k_cover
over each expanded level) against the host definition (Spec.cover), the
independent model (tests/cover_model.py), the oracle's 55 counters and TLC's
recorded coverage block, on the narrow, the deferred wide and the materialising
paths, in both claim modes; single levels as differences of bounded runs; the
whole NP=2 model (740.6M states expanded; 64-bit totals); the refusals; and
coverage off."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import cover_model
import kubecheck
import pyoracle
from kubecheck import tlc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GOLDEN = json.load(open(os.path.join(GOLD, "model1_coverage.json")))
SUMS = json.load(open(os.path.join(GOLD, "model1_cover_sums.json")))
NP2_LEVELS = 31          # levels 26-30 are wider than the narrow path takes (8,192)
NP2_EXPANDED = 149618


def run(coverage=True, **kw):
    with kubecheck.ModelChecker(kubecheck.ModelConfig(**kw), coverage=coverage) as mc:
        return mc.run()


# ------------------------------------------------------------------- Model_1
@pytest.mark.parametrize("first_claim", [False, True])
def test_model1_equals_host_sums_and_tlc(first_claim):
    r = run(first_claim=first_claim)
    assert r.error is None and (r.distinct, r.generated) == (163408, 577736)
    assert max(r.level_width) == 3939                     # every level narrow
    assert r.coverage == SUMS                             # (== cover_model == Spec.cover: tests/test_cover_host.py)
    for (code, depth, span, name, count, cost), e in zip(tlc.coverage_values(r, r.coverage), GOLDEN):
        assert count == e["count"], e["mcout_line"]
        if e["code"] != 2772 and e["mcout_line"] not in tlc.COVERAGE_COST_UNKNOWN:
            assert cost == e["cost"], e["mcout_line"]


def test_cli_tool_coverage_equals_golden():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tla-kubernetes_amd"))
    cmd = [sys.executable, "-m", "kubecheck.tlc", "-tool", "-coverage", "-nocheckfps", "-config",
           os.path.join(ROOT, "models", "Model_1.cfg")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    a = lines.index("@!@!@STARTMSG 2201:0 @!@!@") + 3
    b = lines.index("@!@!@STARTMSG 2202:0 @!@!@")
    block = lines[a:b]
    assert len(block) == 3 * len(GOLDEN)
    for k, e in enumerate(GOLDEN):
        start, body, end = block[3 * k:3 * k + 3]
        assert start == f"@!@!@STARTMSG {e['code']}:0 @!@!@" and end == f"@!@!@ENDMSG {e['code']} @!@!@"
        l1, c1, l2, c2 = e["span"]
        span = f"line {l1}, col {c1} to line {l2}, col {c2} of module KubeAPI"
        if e["code"] == 2774:
            assert body == f"<{e['name']} {span}>"
        elif e["code"] == 2773:
            assert body == f"<{e['name']} {span}>: {e['cost']}:{e['count']}"
        elif e["code"] == 2772:       # the distinct half is the engine's own, as without the flag
            assert body.startswith(f"<{e['name']} {span}>: ") and body.endswith(f":{e['count']}")
        elif e["code"] == 2775 and e["mcout_line"] not in tlc.COVERAGE_COST_UNKNOWN:
            assert body == f"  {'|' * e['depth']}{span}: {e['count']}:{e['cost']}"
        else:
            assert body == f"  {'|' * e['depth']}{span}: {e['count']}", e["mcout_line"]


# ------------------------------------------------------- NP=2, 31 levels
class Np2:
    """The oracle's levels 1..30 of NP=2, their host sums per level, and its bounded run."""

    def __init__(self):
        self.cfg = pyoracle.config(1, 2, 1, keep_trace=False, max_levels=NP2_LEVELS)
        self.ref = pyoracle.run(self.cfg)
        spec = kubecheck.Spec(kubecheck.ModelConfig(np=2))
        self.level = {}
        self.total = {}
        for lv in range(1, NP2_LEVELS):
            t = pyoracle.level_tuples(self.cfg, lv)
            self.level[lv] = cover_model.cover(t, 1, 2, 1)
            assert spec.cover(t) == self.level[lv]
            self.total = cover_model.add(self.total, self.level[lv])


@pytest.fixture(scope="module")
def np2():
    return Np2()


def check_np2(r, np2):
    assert r.error is None and r.depth == NP2_LEVELS
    assert r.level_width == np2.ref["level_width"]
    assert r.level_width[29] == 35224 and all(w > 8192 for w in r.level_width[25:30])
    assert r.coverage["states"] == NP2_EXPANDED == sum(r.level_width[:30])
    assert r.coverage == np2.total
    # the oracle's 55 counters
    assert {k: r.coverage["B_" + k] for k in np2.ref["branch"]} == np2.ref["branch"]
    assert {k: r.coverage["cov_" + k] for k in np2.ref["cov"]} == np2.ref["cov"]
    assert r.act_gen == np2.ref["act_gen"]


@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("keep_trace", [True, False])
def test_np2_bounded_equals_host(np2, first_claim, keep_trace):
    r = run(np=2, max_levels=NP2_LEVELS, first_claim=first_claim, keep_trace=keep_trace)
    assert r.deferred_states > 0 and r.narrow_levels > 0
    check_np2(r, np2)


@pytest.mark.parametrize("first_claim", [False, True])
def test_np2_materialising_path(np2, first_claim, monkeypatch):
    monkeypatch.setenv("KC_DEFER", "0")
    r = run(np=2, max_levels=NP2_LEVELS, first_claim=first_claim)
    assert r.deferred_states == 0
    check_np2(r, np2)


def test_np2_chunked_levels(np2):
    # explicit chunks: every level on the wide path, the widest in five chunks
    r = run(np=2, max_levels=NP2_LEVELS, chunk_states=8192)
    assert r.narrow_levels == 0 and r.levels_chunks > NP2_LEVELS
    check_np2(r, np2)


@pytest.mark.parametrize("first_claim", [False, True])
@pytest.mark.parametrize("level", [27, 12])          # a deferred wide level and a narrow one
def test_one_level_alone(np2, level, first_claim):
    hi = run(np=2, first_claim=first_claim, max_levels=level + 1).coverage
    lo = run(np=2, first_claim=first_claim, max_levels=level).coverage
    assert {k: hi[k] - lo[k] for k in hi} == np2.level[level]
    assert hi["states"] - lo["states"] == np2.ref["level_width"][level - 1]


def test_rerun_and_switching_off(np2):
    with kubecheck.ModelChecker(kubecheck.ModelConfig(np=2, max_levels=NP2_LEVELS)) as mc:
        assert mc.run().coverage is None
        assert mc.run(coverage=True).coverage == np2.total
        assert mc.run().coverage == np2.total             # the setting stays; the sums start again
        assert mc.run(coverage=False).coverage is None


# ------------------------------------------------------------- NP=2, whole
def test_np2_whole_both_modes():
    full = json.load(open(os.path.join(GOLD, "np2_full.json")))
    det = run(np=2, keep_trace=False)
    first = run(np=2, keep_trace=False, first_claim=True)
    assert det.claim_mode == "minimum" and first.claim_mode == "first"
    for r in (det, first):
        assert r.error is None and r.distinct == full["distinct"] and r.generated == full["generated"]
        assert r.act_gen == full["act_gen"]
    c = det.coverage
    assert c == first.coverage
    d, g = det.distinct, det.act_gen
    assert c["states"] == d
    assert c["cov_api2"] >= c["cov_api"]
    # THEN + ELSE of every IF = the action's pairs (CStart: its two branches)
    assert c["B_CSTART_THEN"] + c["B_CSTART_ELSE"] == 2 * c["pairs_CStart"] == g["CStart"]
    for a, arms in (("C1", ("C1_START", "C1_C10")), ("C11", ("C11_START", "C11_c12")),
                    ("C13", ("C13_START", "C13_C2")), ("C3", ("C3_START", "C3_C8")), ("C8", ("C8_C4", "C8_C6")),
                    ("C7", ("C7_START", "C7_C4")), ("PVCListedPVCs", ("PVCL_START", "PVCL_HAVE"))):
        assert c["B_" + arms[0]] + c["B_" + arms[1]] == c["pairs_" + a] == g[a], a
    assert c["B_API_FORCE_REPLACE"] + c["B_API_FORCE_CREATE"] == c["B_API_FORCE"]
    assert c["B_API_UPDATE_OK"] + c["B_API_UPDATE_ERR"] == c["B_API_UPDATE"]
    assert c["B_API_CREATE"] + c["B_API_FORCE"] + c["B_API_GET"] + c["B_API_DELETE"] + c["B_API_UPDATE"] + \
        c["B_API_ASSERT"] + c["B_API_LIST"] == g["APIStart"]
    # every |-guard line = self-set size x distinct
    vals = tlc.coverage_values(det, c, procs=(1, 2, 1))
    rows = list(zip(tlc.COVERAGE_LINES, vals))
    size = {"P": 4, "NC": 1, "NP": 2, "NS": 1}
    guards = 0
    for k, (row, v) in enumerate(rows):
        if row[0] == 2772 and rows[k + 2][0][1] == 1:
            guards += 1
            assert rows[k + 2][1][4] == size[rows[k + 2][0][3].split("*")[0]] * d, row[3]
            assert rows[k + 1][1][4] >= rows[k + 2][1][4]
    assert guards == 22
    assert all(v[4] is None or v[4] >= 0 for v in vals)
    # Model_1's zero-count lines (KubeAPI.tla line of each) that are alive here.
    # None can be: no process ever issues a Create (:700-705), the PVC a Get asks for is never
    # deleted (C6 deletes Secrets only, :727-728), and :742 follows an Assert(FALSE).
    alive = sorted({row[2][0] for row, v in rows if row[0] == 2221 and v[4] > 0} &
                   {e["span"][0] for e in GOLDEN if e["code"] == 2221 and e["count"] == 0})
    print("Model_1 zero-count lines non-zero at NP=2:", alive)
    assert alive == []


# ------------------------------------------------------------------ refusals
def test_symmetric_engine_refuses():
    with kubecheck.ModelChecker(kubecheck.ModelConfig(np=2, symmetry="controllers")) as mc:
        with pytest.raises(kubecheck.KubecheckError) as ei:
            mc.set_coverage(True)
        assert ei.value.code == -22 and "symmetry" in str(ei.value)
        mc.set_coverage(False)
    # a mask that selects no group runs the plain engine
    assert run(symmetry="controllers", max_levels=5).coverage["states"] > 0


@pytest.mark.parametrize("kw", [dict(seen_hbm_bytes=1 << 24), dict(frontier_hbm_bytes=1 << 24), dict(trace_host=True)])
def test_spill_options_refuse(kw):
    with kubecheck.ModelChecker(kubecheck.ModelConfig(**kw)) as mc:
        with pytest.raises(kubecheck.KubecheckError) as ei:
            mc.set_coverage(True)
        assert ei.value.code == -22


# -------------------------------------------------------------- coverage off
def test_off_launches_what_it_always_did():
    lib = kubecheck.load()
    with kubecheck.ModelChecker(kubecheck.ModelConfig(np=2, max_levels=NP2_LEVELS)) as never:
        r0 = never.run()
        k0, n0 = never.kernel_times(), never.narrow_times()[1:]
        out = (C.c_uint64 * lib.kc_cover_count())()
        assert lib.kc_engine_coverage(never._h, out, len(out)) == -22
        assert b"off" in lib.kc_last_error()
    with kubecheck.ModelChecker(kubecheck.ModelConfig(np=2, max_levels=NP2_LEVELS), coverage=True) as mc:
        on = mc.run()
        k_on = mc.kernel_times()
        r1 = mc.run(coverage=False)
        k1, n1 = mc.kernel_times(), mc.narrow_times()[1:]
    assert r0.coverage is None and r1.coverage is None and on.coverage is not None
    assert {k: v[1] for k, v in k1.items()} == {k: v[1] for k, v in k0.items()}
    assert n1 == n0
    assert {k: v[1] for k, v in k_on.items()} == {k: v[1] for k, v in k0.items()}   # k_cover is none of the four
    assert (r1.distinct, r1.generated, r1.act_gen, r1.act_dist) == (r0.distinct, r0.generated, r0.act_gen, r0.act_dist)
    assert (on.distinct, on.generated, on.act_gen, on.act_dist) == (r0.distinct, r0.generated, r0.act_gen, r0.act_dist)


def test_error_run_has_no_coverage():
    lib = kubecheck.load()
    with kubecheck.ModelChecker(kubecheck.ModelConfig(nc=2), coverage=True) as mc:
        r = mc.run()
        assert r.error is not None and r.coverage is None
        out = (C.c_uint64 * lib.kc_cover_count())()
        assert lib.kc_engine_coverage(mc._h, out, len(out)) == -22
        assert b"error" in lib.kc_last_error()
        assert lib.kc_engine_coverage(mc._h, out, 3) == -22
