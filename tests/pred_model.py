"""Host model of user-defined invariants, in the oracle's
tuple space.

TEST INFRASTRUCTURE ONLY.  A sequential BFS over pyoracle.successors (TLC
-workers 1 order, which is the deterministic claim mode's index order) that
applies §4.13's rules directly and judges every state with pred.evaluate; it
never sees the packed state or a compiled program.

Rules: (1) a user invariant is evaluated on every state the run expands, Init
states included (levels 1..L-1 of a run bounded by max_levels = L), once;
(2) the first level that holds a violating state ends the run, after that
level's expansion: generated, distinct and the widths are whole-level numbers
and include the width of what that level found; (3) the state reported is the
violating one with the smallest index in the level, the invariant the first
given that it violates, the trace its parent chain; (4) that violation comes
before anything the expansion of the same level found (an Assert, a deadlock,
a built-in invariant on a new state); a built-in error of an earlier level,
or of the Init states, comes first; (5) invariants that hold change nothing.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "tla-kubernetes_amd")):
    if os.path.abspath(p) not in [os.path.abspath(q) for q in sys.path]:
        sys.path.insert(0, os.path.abspath(p))
import pyoracle  # noqa: E402
from con_model import violated  # noqa: E402
from kubecheck import pred  # noqa: E402


def run(nc=1, np_=1, ns=1, *, user=None, variant=0, invariants=3, can_fail=True, can_timeout=True,
        check_deadlock=True, max_levels=0, on_level=None) -> dict:
    """user: {name: predicate text}.  on_level(depth, tuples): every expanded level's states, in index order."""
    cfg = pyoracle.config(nc, np_, ns, can_fail=can_fail, can_timeout=can_timeout, variant=variant,
                          check_deadlock=check_deadlock, invariants=invariants)
    names = list(user or {})
    asts = [pred.parse(user[n], nc, np_, ns) for n in names]
    out = {"generated": 0, "distinct": 0, "init": 0, "level_width": [], "error": None, "complete": False,
           "states_evaluated": 0, "violations": {n: 0 for n in names}}
    seen = set()
    states, parent = [], []

    def chain(sidx):
        trace = []
        while sidx is not None and sidx >= 0:
            trace.append(states[sidx])
            sidx = parent[sidx]
        trace.reverse()
        return trace

    def fail(err, sidx, x=None):
        if out["error"] is not None:
            return
        trace = chain(sidx)
        if x is not None:
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
        if on_level:
            on_level(depth, [s for s, _ in level])
        # the level's own states, judged as it is expanded
        user_err = None
        out["states_evaluated"] += len(level)
        for s, sidx in level:
            bad = [k for k, a in enumerate(asts) if not pred.evaluate(a, s, nc, np_, ns)]
            for k in bad:
                out["violations"][names[k]] += 1
            if bad and user_err is None:
                user_err = ({"kind": "user_invariant", "name": names[bad[0]], "k": bad[0], "level": depth}, sidx)
        nxt = []
        built_in = None
        for s, sidx in level:
            succ, failed = pyoracle.successors(cfg, s)
            if succ is None:
                built_in = built_in or ({"kind": "assertion", "action": failed, "level": depth}, parent[sidx], s)
                continue
            if not succ and check_deadlock:
                built_in = built_in or ({"kind": "deadlock", "level": depth}, parent[sidx], s)
                continue
            for _, x in succ:
                out["generated"] += 1
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
                        built_in = built_in or ({"kind": "invariant", "invariant": inv, "level": depth + 1}, sidx, x)
        if user_err is not None:
            if nxt:
                out["level_width"].append(len(nxt))
            fail(user_err[0], user_err[1])
        elif built_in is not None:
            fail(*built_in)
        level = nxt
    out["depth"] = len(out["level_width"])
    out["complete"] = out["error"] is None and not level
    return out


# ---- the example set: what the compile-against-evaluate tests and the GPU tests share
PENDING_BOTH = r'\A a \in Actors : ~((a \in DOMAIN requests /\ requests[a].status = "Pending") /\ ' \
               r'(a \in DOMAIN listRequests /\ listRequests[a].status = "Pending"))'
ONLY_ONE_VERSION = r'Cardinality({o \in apiState : o.k = "Secret"}) <= 1 /\ ' \
                   r'Cardinality({o \in apiState : o.k = "PVC"}) <= 1'


def at_most_one_pending(nc, np_):
    """At most one request or list request "Pending" over all actors: no two of the 2A fields at once."""
    names = pred.proc_names(nc, np_, 0)
    fields = [f'({q} \\in DOMAIN {v} /\\ {v}[{q}].status = "Pending")'
              for q in (f'"{n}"' for n in names) for v in ("requests", "listRequests")]
    pairs = [f"~({a} /\\ {b})" for i, a in enumerate(fields) for b in fields[i + 1:]]
    return " /\\ ".join(pairs)


HOLD_M1 = {"StoreSmall": "Cardinality(apiState) <= 2",
           "DoneMeansReconciled": r'\A c \in Clients : pc[c] = "C5" => ~shouldReconcile[c]',
           "NotBothPending": PENDING_BOTH}
NP2_BOTH_DONE = r'~(\A p \in Controllers : pc[p] = "PVCDone")'
NP2_C5_BOTH_DONE = r'~(pc["Client"] = "C5" /\ pc["PVCController1"] = "PVCDone" /\ pc["PVCController2"] = "PVCDone")'
NP2_HOLDS = r'Cardinality(apiState) <= 4 /\ (\A p \in Controllers : Len(stack[p]) <= 1)'

EXAMPLES_M1 = dict(HOLD_M1)
EXAMPLES_M1.update({
    "StoreAtMostOne": "Cardinality(apiState) <= 1",
    "NeverC4": r'\A c \in Clients : pc[c] # "C4"',
    "NeverC5": r'\A c \in Clients : pc[c] # "C5"',
    "NeverPVCDone": 'pc["PVCController"] # "PVCDone"',
    "OnePending": at_most_one_pending(1, 1),
    "OnlyOneVersion": ONLY_ONE_VERSION,
    "Mixed": r'(requests["Client"].op \in {"Get", "Force"} \/ "Client" \notin DOMAIN requests) <=> '
             r'~(op["Client"] = "Update" /\ kind["PVCController"] = defaultInitValue)',
    "ListSize": r'\E a \in Actors : Cardinality(listRequests[a].objs) >= 1 => Cardinality(apiState) >= 1',
    "ReadBy": r'Cardinality({o \in apiState : "Client" \in o.vv /\ "PVCController" \notin o.vv /\ '
              r'"spec" \notin DOMAIN o}) < 2',
    "OpsAgree": r'\A c \in Clients : requests[c].op = op[c] \/ Len(stack[c]) = 0',
    "Sizes": 'Cardinality(listRequests["PVCController"].objs) <= Cardinality(apiState)',
})
EXAMPLES_NP2 = {"BothDone": NP2_BOTH_DONE, "C5BothDone": NP2_C5_BOTH_DONE, "Holds": NP2_HOLDS,
                "OneListPending": r'\A a \in Actors : \A b \in Actors : pc[a] = pc[b] \/ '
                                  r'~(listRequests[a].status = "Pending" /\ listRequests[b].status = "Pending")'}
EXAMPLES_C101 = {"StoreSmall": "Cardinality(apiState) <= 1", "NeverC5": 'pc["Client"] # "C5"',
                 "Reconciled": 'shouldReconcile["Client"] => pc["Client"] # "C4"',
                 "OnePending": at_most_one_pending(1, 0)}

# ---- the fixture file (tests/golden/pred_fixtures.json)
NOFAULT = dict(can_fail=False, can_timeout=False)
ROWS = [   # id, (nc, np, ns), {name: text}, run() keywords
    ("model1_holds", (1, 1, 1), HOLD_M1, {}),
    ("model1_store1", (1, 1, 1), {"StoreAtMostOne": EXAMPLES_M1["StoreAtMostOne"]}, {}),
    ("model1_c4", (1, 1, 1), {"NeverC4": EXAMPLES_M1["NeverC4"]}, {}),
    ("model1_c5", (1, 1, 1), {"NeverC5": EXAMPLES_M1["NeverC5"]}, {}),
    ("model1_pvcdone", (1, 1, 1), {"NeverPVCDone": EXAMPLES_M1["NeverPVCDone"]}, {}),
    ("model1_onepending", (1, 1, 1), {"OnePending": EXAMPLES_M1["OnePending"]}, {}),
    ("model1_two", (1, 1, 1), {"NeverC5": EXAMPLES_M1["NeverC5"], "NeverC4": EXAMPLES_M1["NeverC4"],
                               "OnePending": EXAMPLES_M1["OnePending"]}, {}),
    ("variant2_oov", (1, 1, 1), {"OnlyOneVersion": ONLY_ONE_VERSION}, dict(variant=2, invariants=0)),
    ("variant5_oov", (1, 1, 1), {"OnlyOneVersion": ONLY_ONE_VERSION}, dict(variant=5, invariants=0)),
    # the user invariant's level is the one whose expansion finds the built-in violation
    ("variant2_precedence", (1, 1, 1), {"NotC1WhileReply": r'~(pc["Client"] = "C1" /\ pc["PVCController"] = "DoReply")'},
     dict(variant=2)),
    ("c101_c5", (1, 0, 1), {"NeverC5": EXAMPLES_C101["NeverC5"]}, NOFAULT),
    ("np2_bothdone", (1, 2, 1), {"BothDone": NP2_BOTH_DONE}, {}),
    ("np2_c5_bothdone", (1, 2, 1), {"C5BothDone": NP2_C5_BOTH_DONE}, {}),
]
SMALL = ("model1_store1", "model1_onepending", "variant5_oov", "c101_c5")      # recomputed by the CPU tests


def row_fixture(rid: str) -> dict:
    (_, model, user, kw), = [r for r in ROWS if r[0] == rid]
    r = run(*model, user=user, **kw)
    e = r["error"]
    out = {"model": list(model), "user": user, "run": kw,
           "verdict": "holds" if e is None else "violated" if e["kind"] == "user_invariant" else e["kind"],
           "generated": r["generated"], "distinct": r["distinct"], "depth": r["depth"], "init": r["init"],
           "level_width": r["level_width"], "states_evaluated": r["states_evaluated"],
           "violations": r["violations"], "complete": r["complete"]}
    if e is not None:
        out.update(name=e.get("name"), k=e.get("k"), err_level=e["level"], trace_len=e["trace_len"],
                   trace=[[int(v) for v in t] for t in e["trace"]])
    return out


def fixtures() -> dict:
    return {"rows": {rid: row_fixture(rid) for rid, _, _, _ in ROWS}}
