#!/usr/bin/env python3
"""Throughput of simulation mode (kubecheck.Simulator) on one GPU.

    python tools/sim_bench.py [--walks 1048576] [--depth 128] [--seed 1] [--reps 3]
                              [--json OUT.json] [--md OUT.md]

For Model_1, NP=2 and NP=3, with and without count_distinct, at
steps_per_launch 8 / 32 / 128: walk-steps per second from the HIP-event time of
the walk launches (kernel_ms) and from the host clock of the whole run
(seconds), the best of --reps runs after one warm-up run.  The comparator is the
project's own: the single-thread rate of the host replay (kc_sim_replay) on the
same box.  Writes one JSON document and the table of DESIGN.md §7.11.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-kubernetes_amd"))

MODELS = [("Model_1", dict()), ("NP=2", dict(np=2)), ("NP=3", dict(np=3))]
SWEEP = (8, 32, 128)


def replay_rate(kubecheck, flags, seed, depth, budget=1.0):
    """Walk-steps per second of kc_sim_replay on one host thread."""
    sp = kubecheck.Spec(kubecheck.ModelConfig(**flags))
    import ctypes as C
    lib, cfg, kind = kubecheck.load(), sp.cfg.to_c(), C.c_int()
    steps, w, t0 = 0, 0, time.perf_counter()
    while time.perf_counter() - t0 < budget:
        steps += lib.kc_sim_replay(C.byref(cfg), seed, depth, w, None, None, 0, C.byref(kind)) - 1
        w += 1
    return steps / (time.perf_counter() - t0), w


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--depth", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()

    import kubecheck

    if kubecheck.device_count() < 1:
        print("sim_bench: no GPU visible", file=sys.stderr)
        return 1
    doc = {"what": "simulation mode throughput", "walks": a.walks, "depth": a.depth, "seed": a.seed,
           "reps": a.reps, "build": kubecheck.load().kc_build_info().decode(), "runs": [], "replay": []}
    for name, flags in MODELS:
        for distinct in (False, True):
            for spl in SWEEP:
                with kubecheck.Simulator(kubecheck.ModelConfig(**flags), seed=a.seed, num_walks=a.walks,
                                         depth=a.depth, steps_per_launch=spl, count_distinct=distinct) as sim:
                    sim.run()                                    # warm-up
                    runs = [sim.run() for _ in range(a.reps)]
                best_k = min(r.kernel_ms for r in runs)
                best_s = min(r.seconds for r in runs)
                r = runs[0]
                row = {"model": name, "count_distinct": distinct, "steps_per_launch": spl, "steps": r.steps,
                       "launches": r.launches, "distinct_visited": r.distinct_visited,
                       "fpset_slots": r.fpset_slots, "walks_error": r.walks_error,
                       "kernel_ms": best_k, "seconds": best_s,
                       "kernel_ms_all": [x.kernel_ms for x in runs], "seconds_all": [x.seconds for x in runs],
                       "steps_per_s_kernel": r.steps / (best_k * 1e-3), "steps_per_s_wall": r.steps / best_s}
                doc["runs"].append(row)
                print(json.dumps(row), flush=True)
        rate, n = replay_rate(kubecheck, flags, a.seed, a.depth)
        doc["replay"].append({"model": name, "steps_per_s": rate, "walks": n})
        print(json.dumps(doc["replay"][-1]), flush=True)

    md = ["| model | count_distinct | steps/launch | kernel ms | G steps/s (kernel) | wall ms | G steps/s (wall) |"
          " distinct visited |", "|---|---|---|---|---|---|---|---|"]
    for r in doc["runs"]:
        md.append(f"| {r['model']} | {'yes' if r['count_distinct'] else 'no'} | {r['steps_per_launch']} | "
                  f"{r['kernel_ms']:.2f} | {r['steps_per_s_kernel'] / 1e9:.2f} | {r['seconds'] * 1e3:.1f} | "
                  f"{r['steps_per_s_wall'] / 1e9:.2f} | {r['distinct_visited'] or '-'} |")
    md += ["", "| model | kc_sim_replay, one host thread, M steps/s |", "|---|---|"]
    md += [f"| {r['model']} | {r['steps_per_s'] / 1e6:.2f} |" for r in doc["replay"]]
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
