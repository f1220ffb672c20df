"""bench.py's command line: the plain line, --full, --dump-outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kubecheck import ACTIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model1(mcout, fixtures):
    fx = fixtures["model1"]
    return {"init": mcout["init"], "generated": mcout["generated"], "distinct": mcout["distinct"],
            "queue_left": mcout["queue_left"], "depth": mcout["depth"], "complete": True,
            "act_gen": mcout["act_gen"], "act_dist": fx["act_dist"], "level_width": fx["level_width"],
            "outdeg_hist": fx["outdeg_hist"]}


def test_options(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_arrays(bench, mcout, fixtures, tmp_path):
    r = _model1(mcout, fixtures)
    # first-claim mode: only what does not depend on which copy of a state won
    first = bench.check_outputs(r, "first")
    assert sorted(first) == ["act_gen", "counts", "level_width"]
    det = bench.check_outputs(r, "minimum")
    assert sorted(det) == ["act_dist", "act_gen", "counts", "level_width", "outdeg_hist"]
    bench.dump_outputs(str(tmp_path / "o"), det)
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in os.listdir(tmp_path / "o")}
    assert sorted(got) == sorted(det) and all(a.dtype == np.float64 for a in got.values())
    assert got["counts"].tolist() == [mcout["init"], mcout["generated"], mcout["distinct"], mcout["queue_left"],
                                      mcout["depth"], 1]
    assert got["level_width"].tolist() == fixtures["model1"]["level_width"]
    assert got["act_gen"].tolist() == [mcout["act_gen"][a] for a in ACTIONS]
    assert sum(got["act_dist"]) + mcout["init"] == mcout["distinct"]


@pytest.mark.gpu
def test_plain_line_and_dump_model1(mcout, fixtures, tmp_path):
    # a plain run: the headline line only, and the last timed check's results as .npy
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "model1",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "distinct states/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    # value = distinct states per second of a timed step (ms_per_step is printed to 3 decimals)
    assert abs(d["value"] - mcout["distinct"] / (d["ms_per_step"] * 1e-3)) <= (
        0.0005 / d["ms_per_step"] + 1e-6) * d["value"]
    assert not {"cpu_baseline", "deterministic", "first_claim"} & set(d)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {"counts", "level_width", "act_gen"} <= set(got)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["counts"].tolist() == [mcout["init"], mcout["generated"], mcout["distinct"], mcout["queue_left"],
                                      mcout["depth"], 1]
    assert got["level_width"].tolist() == fixtures["model1"]["level_width"]
    assert got["act_gen"].tolist() == [mcout["act_gen"][a] for a in ACTIONS]
