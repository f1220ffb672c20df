"""Host model of action properties (TLC's PROPERTY [][A]_vars, a step
invariant), in the oracle's tuple space.

TEST INFRASTRUCTURE ONLY.  A sequential BFS over pyoracle.successors that
applies DESIGN.md §4.12's rules directly; independent of the product's packed
form.  The predicates are written on the canonical tuple
(include/kubecheck.h: word 0 = apiState as a mask over U, bit 63 the
lostUpdate ghost; then 19 words per process, q[11..14] = requests present /
op / status / object byte, q[15..18] = listRequests present / kind / status /
objs; status 1 = "Pending", 2 = "Ok"; op 3 = "Update"; object byte bit 1 =
the identity; element u of U = identity << (A + 1) | spec << A | vv):

  NoBlindUpdate      every requests[c] that is an Update, "Pending" in s and
                     "Ok" in x has some o in apiState (unprimed) of the same
                     identity with c in o.vv (HasRead, KubeAPI.tla:733)
  OneReplyPerStep    at most one of requests[a], listRequests[a] leaves
                     "Pending" in the step
  StoreNeverShrinks  Cardinality(apiState') >= Cardinality(apiState)

Rules: (1) every generated successor of every expanded parent is a step and
is checked, whether the child is new or seen; a step with x == s passes;
Init states are not steps; (2) on one step a new child's invariants come
before the action properties (TLC's order); (3) the error is the first in
generation order of the first level that has one; (4) that level is still
counted to its end: step_checked, step_violations, generated, distinct and the
level widths are whole-level numbers; (5) a property that holds changes
nothing else.
"""
from __future__ import annotations

import numpy as np

try:
    import pyoracle
except ImportError:      # run as a script (the fixture writer): the oracle's directory is not on the path yet
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import pyoracle
from con_model import _block, pending_lists, pending_requests, stored, violated

PROPERTIES = ("NoBlindUpdate", "OneReplyPerStep", "StoreNeverShrinks")   # bit k = PROPERTIES[k]
OP_UPDATE, ST_PENDING, ST_OK = 3, 1, 2


def no_blind_update(s, x, actors: int) -> bool:
    api = int(s[0])
    half = 1 << (actors + 1)
    for c in range(actors):
        qs, qx = _block(s, c), _block(x, c)
        if not (int(qs[11]) == 1 and int(qs[12]) == OP_UPDATE and int(qs[13]) == ST_PENDING):
            continue
        if not (int(qx[11]) == 1 and int(qx[13]) == ST_OK):
            continue
        ident = (int(qs[14]) >> 1) & 1
        if not any((api >> u) & 1 and (u >> c) & 1 for u in range(ident * half, (ident + 1) * half)):
            return False
    return True


def one_reply_per_step(s, x, actors: int) -> bool:
    A = range(actors)
    left = len(set(pending_requests(s, A)) - set(pending_requests(x, A))) + \
        len(set(pending_lists(s, A)) - set(pending_lists(x, A)))
    return left <= 1


def store_never_shrinks(s, x, actors: int) -> bool:
    return stored(x, actors) >= stored(s, actors)


PREDICATES = (no_blind_update, one_reply_per_step, store_never_shrinks)


def step_violations(s, x, actors: int, mask: int = 7) -> int:
    """The mask of the properties in `mask` that the step s -> x violates."""
    if np.array_equal(np.asarray(s, dtype=np.uint64), np.asarray(x, dtype=np.uint64)):
        return 0
    v = 0
    for k, p in enumerate(PREDICATES):
        if (mask >> k) & 1 and not p(s, x, actors):
            v |= 1 << k
    return v


def mask_of(names) -> int:
    return sum(1 << PROPERTIES.index(n) for n in names)


def run(nc=1, np_=1, ns=1, *, properties=(), variant=0, invariants=3, can_fail=True, can_timeout=True,
        check_deadlock=True, max_levels=0, on_pairs=None, pair_chunk=1 << 15) -> dict:
    """The BFS with action properties.  on_pairs(S, X, actions, masks): called
    with chunks of every (parent, successor) pair in generation order (uint64
    arrays, action ids, step_violations answers under `properties`)."""
    cfg = pyoracle.config(nc, np_, ns, can_fail=can_fail, can_timeout=can_timeout, variant=variant,
                          check_deadlock=check_deadlock, invariants=invariants)
    actors = nc + np_
    mask = mask_of(properties)
    out = {"generated": 0, "distinct": 0, "init": 0, "level_width": [], "error": None, "complete": False,
           "step_checked": 0, "step_violations": {p: 0 for p in PROPERTIES}}
    seen = set()
    states, parent = [], []
    pS, pX, pA, pM = [], [], [], []

    def flush():
        if on_pairs and pS:
            on_pairs(np.array(pS, dtype=np.uint64), np.array(pX, dtype=np.uint64), np.array(pA, dtype=np.int32),
                     np.array(pM, dtype=np.int32))
        del pS[:], pX[:], pA[:], pM[:]

    def fail(err, sidx, x):
        if out["error"] is not None:
            return
        trace = []
        while sidx is not None and sidx >= 0:
            trace.append(states[sidx])
            sidx = parent[sidx]
        trace.reverse()
        trace.append(np.array(x, dtype=np.uint64))
        err.update(trace=trace, trace_len=len(trace))
        out["error"] = err

    level = []
    for t in pyoracle.level_tuples(cfg, 1):
        out["generated"] += 1
        out["init"] += 1
        if t.tobytes() in seen:
            continue
        seen.add(t.tobytes())
        out["distinct"] += 1
        states.append(t.copy())
        parent.append(-1)
        level.append((states[-1], len(states) - 1))
        inv = violated(t, nc, np_, invariants)
        if inv is not None:
            fail({"kind": "invariant", "invariant": inv, "level": 1}, None, t)
    depth = 0
    while level and out["error"] is None:
        depth += 1
        out["level_width"].append(len(level))
        if max_levels and depth >= max_levels:
            break
        nxt = []
        for s, sidx in level:
            succ, failed = pyoracle.successors(cfg, s)
            if succ is None:
                fail({"kind": "assertion", "action": failed, "level": depth}, parent[sidx], s)
                continue
            if not succ and check_deadlock:
                fail({"kind": "deadlock", "level": depth}, parent[sidx], s)
                continue
            for a, x in succ:
                out["generated"] += 1
                out["step_checked"] += 1
                key = x.tobytes()
                if key not in seen:
                    seen.add(key)
                    out["distinct"] += 1
                    xc = x.copy()
                    states.append(xc)
                    parent.append(sidx)
                    nxt.append((xc, len(states) - 1))
                    inv = violated(x, nc, np_, invariants)
                    if inv is not None:
                        fail({"kind": "invariant", "invariant": inv, "level": depth + 1}, sidx, x)
                bad = step_violations(s, x, actors, mask)
                if on_pairs:
                    pS.append(s), pX.append(x.copy()), pA.append(pyoracle.ACTIONS.index(a)), pM.append(bad)
                    if len(pS) >= pair_chunk:
                        flush()
                if bad:
                    for k, p in enumerate(PROPERTIES):
                        if (bad >> k) & 1:
                            out["step_violations"][p] += 1
                    low = (bad & -bad).bit_length() - 1
                    fail({"kind": "action_property", "property": PROPERTIES[low], "action": a, "level": depth + 1},
                         sidx, x)
        level = nxt
    flush()
    out["depth"] = len(out["level_width"])
    out["complete"] = out["error"] is None and not level
    return out


# ---- the fixture file (tests/golden/actprop_fixtures.json)
NOFAULT = dict(can_fail=False, can_timeout=False)
ROWS = [   # id, (nc, np, ns), run() keywords
    ("model1_noblind", (1, 1, 1), dict(properties=("NoBlindUpdate",))),
    ("model1_onereply", (1, 1, 1), dict(properties=("OneReplyPerStep",))),
    ("model1_shrinks", (1, 1, 1), dict(properties=("StoreNeverShrinks",))),
    ("model1_all", (1, 1, 1), dict(properties=PROPERTIES)),
    ("model1_v1_noblind", (1, 1, 1), dict(properties=("NoBlindUpdate",), variant=1)),
    ("np2_v1_noblind", (1, 2, 1), dict(properties=("NoBlindUpdate",), variant=1)),
    ("np2_nofault_shrinks", (1, 2, 1), dict(properties=("StoreNeverShrinks",), **NOFAULT)),
]
SMALL = ("model1_v1_noblind", "model1_shrinks")      # recomputed by the CPU tests


def row_fixture(rid: str) -> dict:
    (_, model, kw), = [r for r in ROWS if r[0] == rid]
    r = run(*model, **kw)
    e = r["error"]
    out = {"model": list(model), "run": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()},
           "verdict": "holds" if e is None else "violated" if e["kind"] == "action_property" else e["kind"],
           "generated": r["generated"], "distinct": r["distinct"], "depth": r["depth"], "init": r["init"],
           "level_width": r["level_width"], "step_checked": r["step_checked"],
           "step_violations": r["step_violations"], "complete": r["complete"]}
    if e is not None:
        out.update(property=e.get("property"), action=e.get("action"), err_level=e["level"],
                   trace_len=e["trace_len"], trace=[[int(v) for v in t] for t in e["trace"]])
    return out


def fixtures() -> dict:
    return {"rows": {rid: row_fixture(rid) for rid, _, _ in ROWS}}


if __name__ == "__main__":
    import json
    import sys
    json.dump(fixtures(), sys.stdout, indent=None, sort_keys=True, separators=(",", ":"))
    sys.stdout.write("\n")
