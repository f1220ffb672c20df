#!/usr/bin/env python3
"""Regenerate tests/golden/pred_fixtures.json: what a run with user-defined
invariants must report, from the host model tests/pred_model.py (a sequential
BFS over the CPU oracle's successors that judges states with pred.evaluate).
Data only: counts, widths, names and traces.  Needs no GPU; the two NP=2 rows
walk 34 levels of the oracle and take most of the time.

    python tools/make_pred_golden.py [row ...]
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "tla-kubernetes_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import pred_model  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pred_fixtures.json")


def main() -> None:
    want = sys.argv[1:] or [r[0] for r in pred_model.ROWS]
    rows = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            rows = json.load(f)["rows"]
    for rid in want:
        t = time.time()
        rows[rid] = pred_model.row_fixture(rid)
        r = rows[rid]
        print(f"{rid}: {r['verdict']} level {r.get('err_level')} {r['generated']} / {r['distinct']} / depth {r['depth']}, "
              f"evaluated {r['states_evaluated']}, violations {r['violations']} ({time.time() - t:.1f} s)", file=sys.stderr)
    order = [r[0] for r in pred_model.ROWS]
    rows = {k: rows[k] for k in order if k in rows}
    with open(OUT, "w") as f:
        json.dump({"rows": rows}, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
