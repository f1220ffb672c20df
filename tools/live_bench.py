#!/usr/bin/env python3
"""Timings of the liveness check (kubecheck.LivenessChecker) on one GPU.

    python tools/live_bench.py [--reps 3] [--fairness next|process] [--formulas] [--json OUT.json] [--md OUT.md]

For Model_1 and for NP=2 with both constants FALSE, every property: the size of
the graph, |S| and |L|, the trim rounds, and build_ms (the graph build), trim_ms
(mark and trim) and the whole run's wall time, each the best of --reps runs
after one warm-up run on the same handle.  Writes one JSON document and the
table of DESIGN.md §7.12.  With --fairness process (per-process weak fairness,
the fair SCCs) the rows also hold the SCC counts, |F|, the SCC phase's launches
and scc_ms, the JSON goes to profiles/live_bench_fair.json unless --json says
otherwise, and the table is the one of DESIGN.md §7.13.  With --formulas every
model gets further rows: the built-in properties spelled as user formulas
(DESIGN.md §4.14, §7.22), which take the program-driven mark kernel and the
first-trigger launch in place of the compiled stay predicate.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-kubernetes_amd"))

MODELS = [("Model_1", dict()), ("NP=2, constants FALSE", dict(np=2, can_fail=False, can_timeout=False))]
# the built-in properties as a user writes them (row name -> formula)
FORMULAS = {
    "ReconcileCompletes as a formula": 'shouldReconcile["Client"] ~> ~shouldReconcile["Client"]',
    "ClientRestarts as a formula": '[]<>(pc["Client"] = "CStart")',
    "SomeActorRestarts as a formula":
        r'[]<>((\E c \in Clients : pc[c] = "CStart") \/ (\E p \in Controllers : pc[p] = "PVCStart"))',
}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--fairness", choices=("next", "process"), default="next")
    ap.add_argument("--formulas", action="store_true", help="also the built-ins spelled as user formulas")
    a = ap.parse_args()
    fair = a.fairness == "process"
    if fair and a.json is None:
        a.json = os.path.join(ROOT, "profiles", "live_bench_fair.json")

    import kubecheck

    if kubecheck.device_count() < 1:
        print("live_bench: no GPU visible", file=sys.stderr)
        return 1
    doc = {"what": "liveness check timings", "reps": a.reps, "fairness": a.fairness,
           "build": kubecheck.load().kc_build_info().decode(), "runs": []}
    for name, flags in MODELS:
        rows = [(p, dict(property=p)) for p in kubecheck.PROPERTIES]
        if a.formulas:
            rows += [(n, dict(formula=f, name=n)) for n, f in FORMULAS.items()]
        for prop, which in rows:
            with kubecheck.LivenessChecker(kubecheck.ModelConfig(**flags), fairness=a.fairness, **which) as lc:
                lc.run()                                    # warm-up
                runs = [lc.run() for _ in range(a.reps)]
            r = runs[0]
            row = {"model": name, "property": prop, "states": r.states, "edges": r.edges, "depth": r.depth,
                   "stay_states": r.stay_states, "live_states": r.live_states, "violated": r.violated,
                   "kind": r.kind, "trace_len": r.trace_len, "rounds": r.rounds,
                   "build_ms": min(x.build_ms for x in runs), "trim_ms": min(x.trim_ms for x in runs),
                   "seconds": min(x.seconds for x in runs),
                   "build_ms_all": [x.build_ms for x in runs], "trim_ms_all": [x.trim_ms for x in runs],
                   "seconds_all": [x.seconds for x in runs]}
            if fair:
                row.update({"sccs": r.sccs, "fair_sccs": r.fair_sccs, "fair_states": r.fair_states,
                            "scc_rounds": r.scc_rounds, "scc_ms": min(x.scc_ms for x in runs),
                            "scc_ms_all": [x.scc_ms for x in runs]})
            doc["runs"].append(row)
            print(json.dumps(row), flush=True)

    md = ["| model | property | states / edges / depth | \\|S\\| → \\|L\\| | rounds | build ms | trim ms | run ms |",
          "|---|---|---|---|---|---|---|---|"]
    if fair:
        md = ["| model | property | \\|S\\| → \\|L\\| | SCCs / fair / \\|F\\| | trim rounds | SCC launches | build ms | "
              "trim ms | scc ms | run ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["runs"]:
        if fair:
            md.append(f"| {r['model']} | {r['property']} | {r['stay_states']:,} → {r['live_states']:,} | "
                      f"{r['sccs']:,} / {r['fair_sccs']:,} / {r['fair_states']:,} | {r['rounds']} | "
                      f"{r['scc_rounds']} | {r['build_ms']:.2f} | {r['trim_ms']:.2f} | {r['scc_ms']:.2f} | "
                      f"{r['seconds'] * 1e3:.2f} |")
            continue
        md.append(f"| {r['model']} | {r['property']} | {r['states']:,} / {r['edges']:,} / {r['depth']} | "
                  f"{r['stay_states']:,} → {r['live_states']:,} | {r['rounds']} | {r['build_ms']:.2f} | "
                  f"{r['trim_ms']:.2f} | {r['seconds'] * 1e3:.2f} |")
    text = "\n".join(md) + "\n"
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
