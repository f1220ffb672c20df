#!/usr/bin/env python3
"""What symmetry reduction (ModelConfig.symmetry) costs and buys on one GPU.

    python tools/sym_bench.py [--reps 3] [--np3-levels 52] [--np3-deepest 66]
                              [--json OUT.json] [--md OUT.md]

In one process on one box, symmetry off and on ("controllers"), in both claim
modes (first_claim 0 / 1): the whole NP=2 model; the first --np3-levels BFS
levels of NP=3 (bench.py's np3_52 workload) at equal level counts; and how
many more NP=3 levels the symmetric run takes before it holds as many
fingerprints as the unreduced prefix does (the seen-set and the frontiers are
what fills HBM: the symmetric run is bounded two levels further at a time
until its distinct count passes the unreduced run's).  Times are kc_result's
seconds (host clock of one check), the best of --reps runs after one warm-up
run.  No figure is gated: a slower symmetric run is reported as it comes.
Writes one JSON document and the tables of DESIGN.md section 7.14.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-kubernetes_amd"))


def measure(kubecheck, reps, **kw):
    with kubecheck.ModelChecker(kubecheck.ModelConfig(keep_trace=False, **kw)) as mc:
        mc.run()                                             # warm-up
        runs = [mc.run() for _ in range(reps)]
    r = runs[0]
    best = min(x.seconds for x in runs)
    return r, {"symmetry": kw.get("symmetry", 0), "first_claim": bool(kw.get("first_claim")),
               "max_levels": kw.get("max_levels", 0), "distinct": r.distinct, "generated": r.generated,
               "depth": r.depth, "levels": len(r.level_width), "peak_frontier": r.peak_frontier,
               "fpset_slots": r.fpset_slots, "claim_mode": r.claim_mode, "complete": r.complete,
               "seconds": best, "seconds_all": [x.seconds for x in runs],
               "distinct_per_s": r.distinct / best, "generated_per_s": r.generated / best}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--np3-levels", type=int, default=52)
    ap.add_argument("--np3-deepest", type=int, default=66)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()

    import kubecheck

    if kubecheck.device_count() < 1:
        print("sym_bench: no GPU visible", file=sys.stderr)
        return 1
    doc = {"what": "symmetry reduction: time and states, on and off", "reps": a.reps,
           "build": kubecheck.load().kc_build_info().decode(), "np2": [], "np3": [], "np3_deeper": []}
    widths = {}
    for name, kw in (("np2", dict(np=2)), ("np3", dict(np=3, max_levels=a.np3_levels))):
        for fc in (False, True):
            for sym in (0, "controllers"):
                r, row = measure(kubecheck, a.reps, symmetry=sym, first_claim=fc, **kw)
                row["model"] = name
                doc[name].append(row)
                widths[(name, fc, sym)] = r.level_width
                print(json.dumps(row), flush=True)
    doc["np2_sym_level_width"] = widths[("np2", False, "controllers")]
    assert widths[("np2", True, "controllers")] == doc["np2_sym_level_width"], "the claim modes disagree"

    # NP=3 further down under symmetry, first-claim mode (8-B seen-set slots)
    base = next(x for x in doc["np3"] if not x["symmetry"] and x["first_claim"])
    fits = a.np3_levels
    for levels in range(a.np3_levels + 2, a.np3_deepest + 1, 2):
        try:
            r, row = measure(kubecheck, 1, np=3, max_levels=levels, symmetry="controllers", first_claim=True)
        except kubecheck.KubecheckError as e:
            doc["np3_deeper"].append({"max_levels": levels, "error": str(e)})
            print(json.dumps(doc["np3_deeper"][-1]), flush=True)
            break
        doc["np3_deeper"].append(row)
        print(json.dumps(row), flush=True)
        # the deepest prefix of this run within the unreduced prefix's counts
        total = 0
        for lv, w in enumerate(r.level_width, 1):
            total += w
            if total <= base["distinct"] and w <= base["peak_frontier"]:
                fits = max(fits, lv)
        if r.distinct > base["distinct"]:
            break
    doc["np3_levels_unreduced"] = a.np3_levels
    doc["np3_levels_symmetric_same_fingerprints"] = fits

    md = ["| model | levels | claims | symmetry | distinct | generated | ms | distinct/s | ms vs off |",
          "|---|---|---|---|---|---|---|---|---|"]
    for name in ("np2", "np3"):
        for row in doc[name]:
            off = next(x for x in doc[name] if not x["symmetry"] and x["first_claim"] == row["first_claim"])
            md.append(f"| {name} | {row['levels']} | {row['claim_mode']} | {row['symmetry'] or 'off'} | "
                      f"{row['distinct']:,} | {row['generated']:,} | {row['seconds'] * 1e3:.1f} | "
                      f"{row['distinct_per_s']:.3g} | {row['seconds'] / off['seconds']:.2f}x |")
    md += ["", "| NP=3 symmetric, first-claim: levels | distinct (orbits) | peak frontier | ms |", "|---|---|---|---|"]
    for row in doc["np3_deeper"]:
        if "error" in row:
            md.append(f"| {row['max_levels']} | {row['error']} | | |")
        else:
            md.append(f"| {row['levels']} | {row['distinct']:,} | {row['peak_frontier']:,} | {row['seconds'] * 1e3:.1f} |")
    md.append("")
    md.append(f"Unreduced NP=3 to level {a.np3_levels}: {base['distinct']:,} fingerprints, peak frontier "
              f"{base['peak_frontier']:,}; the symmetric run stays within both to level {fits}.")
    text = "\n".join(md) + "\n"
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
