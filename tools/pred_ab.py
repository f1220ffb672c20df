#!/usr/bin/env python3
"""What user-defined invariants cost, on one GPU box.

(a) No user invariant, against the parent commit: bench.py's own workloads,
    unmodified, run from a checkout of the parent commit (its tree and its
    built library) and from this tree, alternating (and alternating which
    goes first), `--rounds` times each.
    The parent's own run-to-run spread on the box is the yardstick.
(b) One single-leaf invariant and (c) eight invariants that fill the
    instruction limit, in bench.py's timing loop (bench_single: two warm-up
    runs, five timed, first-claim mode), with a plain run before and after.

    python tools/pred_ab.py --parent-tree DIR [--rounds 3] [--out profiles/pred_ab.json]

DIR holds the parent commit's bench.py, tla-kubernetes_amd/kubecheck (with
lib/libkubecheck.so built from the parent's sources) and tests/golden.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--no-second-line"]
WORKLOADS = {"np2": dict(nc=1, np=2, ns=1), "model1": dict(nc=1, np=1, ns=1)}
SINGLE = {"StoreSmall": "Cardinality(apiState) <= 60"}
# 8 x (8 leaves, 7 ORs, END) = 128 instructions; every one holds on every state
EIGHT = {f"Full{k}": " \\/ ".join(["Cardinality(apiState) <= 60"] + ['Len(stack["Client"]) > 1'] * 7) for k in range(8)}


def bench_line(tree: str, workload: str) -> dict:
    r = subprocess.run([sys.executable, "bench.py"] + BENCH + ["--workload", workload], cwd=tree, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    return json.loads(line)


def timed_loop(kw: dict, invariants, warmup: int = 2, steps: int = 5) -> dict:
    """bench.py's bench_single loop with `invariants` set on the engine."""
    import torch
    import kubecheck

    cfg = kubecheck.ModelConfig(**kw, keep_trace=True, timing=2, fpset_slots=1 << 20, first_claim=True)
    with kubecheck.ModelChecker(cfg, invariants=invariants) as mc:
        for _ in range(warmup):
            mc.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rs = [mc.run() for _ in range(steps)]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    r = rs[-1]
    assert r.error is None and r.complete
    out = {"ms_per_check": round(dt * 1e3 / steps, 3), "distinct": r.distinct, "generated": r.generated, "depth": r.depth}
    if invariants:
        u = r.user_invariants
        assert all(x.violations == 0 for x in u)
        out.update(states_evaluated=u[0].states_evaluated, invariants=len(u),
                   instructions=kubecheck.pred.compile_invariants(invariants, kw["nc"], kw["np"], kw["ns"]).n_instr)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pred_ab.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tla-kubernetes_amd"))
    import kubecheck

    res = {"tool": "tools/pred_ab.py", "bench_args": BENCH, "rounds": a.rounds, "order": "parent first in even rounds, this commit first in odd rounds",
           "build": kubecheck.load().kc_build_info().decode(), "no_invariant": {}, "with_invariants": {}}
    for wl in WORKLOADS:
        rows = {"parent": [], "this": []}
        for k in range(a.rounds):
            # (the side that goes first alternates, so neither always follows the other)
            sides = [("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)]
            for side, tree in (sides if k % 2 == 0 else sides[::-1]):
                j = bench_line(tree, wl)
                rows[side].append(j["ms_per_step"])
                counts = (j["config"]["distinct"], j["config"]["generated"], j["config"]["depth"])
                assert rows.setdefault("counts", counts) == counts
                print(f"{wl} {side}: {j['ms_per_step']} ms", file=sys.stderr, flush=True)
        p, t = rows["parent"], rows["this"]
        rows["parent_spread_ms"] = round(max(p) - min(p), 3)
        rows["this_inside_parent_range"] = [min(p) <= x <= max(p) for x in t]
        rows["this_max_outside_ms"] = round(max(0.0, max(t) - max(p), min(p) - min(t)), 3)
        res["no_invariant"][wl] = rows
    for wl, kw in WORKLOADS.items():
        rows = {"plain_before": timed_loop(kw, None)}
        rows["single_leaf"] = timed_loop(kw, SINGLE)
        rows["eight_full"] = timed_loop(kw, EIGHT)
        rows["plain_after"] = timed_loop(kw, None)
        plain = (rows["plain_before"]["ms_per_check"] + rows["plain_after"]["ms_per_check"]) / 2
        rows["single_leaf_cost_ms"] = round(rows["single_leaf"]["ms_per_check"] - plain, 3)
        rows["eight_full_cost_ms"] = round(rows["eight_full"]["ms_per_check"] - plain, 3)
        print(f"{wl}: {json.dumps(rows)}", file=sys.stderr, flush=True)
        res["with_invariants"][wl] = rows
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
