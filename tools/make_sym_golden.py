#!/usr/bin/env python3
"""Regenerate tests/golden/sym_fixtures.json: what a run under symmetry
reduction must count, from the CPU oracle's per-level state sets and the host
model of the permutation group (tests/sym_model.py).  Data only: level widths
and counts.  Needs no GPU; takes about half a minute (one oracle successor
call per orbit of the cases that pin generated counts).

    python tools/make_sym_golden.py [case ...]
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import pyoracle  # noqa: E402
import sym_model  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sym_fixtures.json")

# name -> (model, symmetry, oracle config kwargs, with generated / act_gen?)
COUNT_CASES = {
    "121_ml22": ((1, 2, 1), "controllers", dict(max_levels=22), False),
    "121_ml30": ((1, 2, 1), "controllers", dict(max_levels=30), False),
    "121_ml34": ((1, 2, 1), "controllers", dict(max_levels=34), True),
    "121_ml36": ((1, 2, 1), "controllers", dict(max_levels=36), False),
    "121_ml34_nofaults": ((1, 2, 1), "controllers", dict(max_levels=34, can_fail=False, can_timeout=False), True),
    "121_ml40_nofaults": ((1, 2, 1), "controllers", dict(max_levels=40, can_fail=False, can_timeout=False), True),
    "131_ml14": ((1, 3, 1), "controllers", dict(max_levels=14), False),
    "131_ml16": ((1, 3, 1), "controllers", dict(max_levels=16), True),
}
# runs that end in an error: the unreduced run's error (kind, level, trace
# length: symmetry must keep them) and the counts of the levels before it: a
# run bounded at the error's level for an Assert (raised when a state of that
# level is expanded; levels 1 .. err_level - 1 are), one level earlier for an
# invariant (its violating state is found when the level before is expanded)
ERROR_CASES = {
    "201_c4": ((2, 0, 1), "clients", dict()),
    "211_c4": ((2, 1, 1), "clients", dict()),
    "221_err": ((2, 2, 1), "actors", dict()),
    "121_v1_nolostupdate": ((1, 2, 1), "controllers", dict(variant=1, invariants=7)),
}


def count_case(model, sym, kw, with_generated):
    cfg = pyoracle.config(*model, **kw)
    e = sym_model.expected(cfg, sym_model.MASKS[sym], with_generated=with_generated)
    return dict(model=list(model), symmetry=sym, config=kw, **e)


def error_case(model, sym, kw):
    ref = pyoracle.run(pyoracle.config(*model, **kw))
    assert ref["err_kind"] != 0, "an error case without an error"
    out = dict(model=list(model), symmetry=sym, config=kw,
               error=dict(err_kind=ref["err_kind"], err_level=ref["err_level"], trace_len=ref["trace_len"],
                          err_action=ref["err_action"], err_invariant=ref["err_invariant"],
                          states=ref["distinct"]))
    bounded = dict(kw, max_levels=ref["err_level"] - (0 if ref["err_kind"] == 1 else 1))
    e = sym_model.expected(pyoracle.config(*model, **bounded), sym_model.MASKS[sym], with_generated=True)
    out["before_error"] = dict(config=bounded, **e)
    return out


def main(argv):
    data = json.load(open(OUT)) if os.path.exists(OUT) and argv else {}
    for name, (model, sym, kw, gen) in COUNT_CASES.items():
        if argv and name not in argv:
            continue
        t0 = time.time()
        data[name] = count_case(model, sym, kw, gen)
        print(f"{name}: {data[name]['states']} states, {data[name]['distinct']} orbits ({time.time() - t0:.1f} s)",
              flush=True)
    for name, (model, sym, kw) in ERROR_CASES.items():
        if argv and name not in argv:
            continue
        t0 = time.time()
        data[name] = error_case(model, sym, kw)
        print(f"{name}: error at level {data[name]['error']['err_level']}, "
              f"{data[name]['before_error']['distinct']} orbits before it ({time.time() - t0:.1f} s)", flush=True)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
