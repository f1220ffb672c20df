"""Host model of state and action constraints (TLC's CONSTRAINT and
ACTION_CONSTRAINT), in the oracle's tuple space.

TEST INFRASTRUCTURE ONLY.  A sequential BFS over pyoracle.successors that
applies DESIGN.md §4.11's rules directly; independent of the product's packed
form.  The predicates are written on the canonical tuple
(include/kubecheck.h: word 0 = apiState as a mask over U, bit 63 the
lostUpdate ghost; then 19 words per process, q[11] / q[13] = requests
present / status, q[15] / q[17] = listRequests present / status, status 1 =
"Pending"):

  StoredAtMost<k>    popcount(word 0 below bit 63) <= k
  InFlightAtMost<k>  #{actors with requests pending} + #{actors with
                     listRequests pending} <= k
  ServeClientsFirst  an APIStart step that takes a PVC controller's requests[p]
                     or listRequests[p] out of "Pending" is allowed only if no
                     client's requests or listRequests is pending before it

Rules: (1) every successor counts as generated (total and per action);
(2) in the model iff every state constraint holds in x and every action
constraint on s -> x, state constraints first; (3) a successor outside is
discarded: no seen-set lookup, not distinct, not queued; (4) its invariants
are still checked; (5) deadlock is Next's alone; (6) Init states outside a
state constraint are discarded (generated, not distinct); (7) depth = levels
with at least one in-model state.
"""
from __future__ import annotations

import numpy as np

import pyoracle

PER_PROC = 19
GHOST = 1 << 63
IN, CUT_STATE, CUT_ACTION = 0, 1, 2


def _block(t, a):
    return t[1 + PER_PROC * a: 1 + PER_PROC * (a + 1)]


def stored(t, actors: int = 1) -> int:
    """Objects in apiState: word 0 below bit 63, the lostUpdate ghost; with 4
    actors the object universe has 64 elements and bit 63 is one of them (no
    ghost exists then)."""
    w = int(t[0])
    return bin(w if actors + 2 >= 6 else w & (GHOST - 1)).count("1")


def pending_requests(t, actors):
    return [a for a in actors if int(_block(t, a)[11]) == 1 and int(_block(t, a)[13]) == 1]


def pending_lists(t, actors):
    return [a for a in actors if int(_block(t, a)[15]) == 1 and int(_block(t, a)[17]) == 1]


def state_cut(t, nc, np_, stored_max=-1, inflight_max=-1) -> bool:
    A = range(nc + np_)
    if stored_max >= 0 and stored(t, nc + np_) > stored_max:
        return True
    if inflight_max >= 0 and len(pending_requests(t, A)) + len(pending_lists(t, A)) > inflight_max:
        return True
    return False


def action_cut(s, x, action, nc, np_) -> bool:
    """ServeClientsFirst on the step s -> x made by `action` (a name)."""
    if action != "APIStart":
        return False
    ctl = range(nc, nc + np_)
    served = [p for p in pending_requests(s, ctl) if p not in pending_requests(x, ctl)] + \
             [p for p in pending_lists(s, ctl) if p not in pending_lists(x, ctl)]
    if not served:
        return False
    cl = range(nc)
    return bool(pending_requests(s, cl) or pending_lists(s, cl))


def in_model(s, x, action, nc, np_, stored_max=-1, inflight_max=-1, serve_clients_first=False) -> int:
    """0 in, 1 state-cut, 2 action-cut (s = None: an Init state)."""
    if state_cut(x, nc, np_, stored_max, inflight_max):
        return CUT_STATE
    if serve_clients_first and s is not None and action_cut(s, x, action, nc, np_):
        return CUT_ACTION
    return IN


def violated(t, nc, np_, invariants=3):
    """Index of the first violated invariant (0 TypeOK, 1 OnlyOneVersion) or None."""
    A = nc + np_
    half = 1 << (A + 1)                        # U = 2^(A+2) bits, identity = the top index bit
    lo, hi = (1 << half) - 1, ((1 << half) - 1) << half
    if invariants & 1:
        for a in range(A):
            q = _block(t, a)
            if int(q[11]) and not (1 <= int(q[12]) <= 5 and int(q[14]) != 0 and 1 <= int(q[13]) <= 3):
                return 0
            if int(q[15]):
                km = {1: lo, 2: hi}.get(int(q[16]), 0)
                if (int(q[18]) & ~km) or not 1 <= int(q[17]) <= 3:
                    return 0
    if invariants & 2:
        w = int(t[0])
        if bin(w & lo).count("1") > 1 or bin(w & hi).count("1") > 1:
            return 1
    return None


def run(nc=1, np_=1, ns=1, *, stored_max=-1, inflight_max=-1, serve_clients_first=False, variant=0,
        invariants=3, check_deadlock=True, max_levels=0, keep_levels=(), keep_trace=False, on_pairs=None,
        pair_chunk=1 << 15) -> dict:
    """The constrained BFS.  keep_levels: levels whose FIFO state arrays are
    returned (levels[L]).  keep_trace: parent pointers, so a violation carries
    its trace.  on_pairs(S, X, actions, cuts): called with chunks of every
    (parent, successor) pair in generation order (uint64 arrays, action ids,
    in_model answers)."""
    cfg = pyoracle.config(nc, np_, ns, variant=variant, check_deadlock=check_deadlock, invariants=invariants)
    kw = dict(stored_max=stored_max, inflight_max=inflight_max, serve_clients_first=serve_clients_first)
    act_gen = {a: 0 for a in pyoracle.ACTIONS}
    act_dist = {a: 0 for a in pyoracle.ACTIONS}
    out = {"generated": 0, "distinct": 0, "cut_state": 0, "cut_action": 0, "level_width": [], "levels": {},
           "error": None, "act_gen": act_gen, "act_dist": act_dist, "init": 0, "complete": False,
           "first_cut_level": None}       # the level the first discarded successor would have been in
    seen = set()
    states, parent = [], []                    # keep_trace: every distinct state and its parent's index
    pS, pX, pA, pC = [], [], [], []

    def flush():
        if on_pairs and pS:
            on_pairs(np.array(pS, dtype=np.uint64), np.array(pX, dtype=np.uint64), np.array(pA, dtype=np.int32),
                     np.array(pC, dtype=np.int32))
        del pS[:], pX[:], pA[:], pC[:]

    def fail(inv, sidx, x):
        trace = []
        if keep_trace:
            while sidx is not None and sidx >= 0:
                trace.append(states[sidx])
                sidx = parent[sidx]
            trace.reverse()
        trace.append(np.array(x, dtype=np.uint64))
        out["error"] = {"kind": "invariant", "invariant": inv, "trace": trace, "trace_len": len(trace)}

    level = []                                 # (tuple, index into states)
    for t in pyoracle.level_tuples(cfg, 1):
        out["generated"] += 1
        out["init"] += 1
        cut = in_model(None, t, None, nc, np_, **kw)
        inv = violated(t, nc, np_, invariants)
        if cut:
            out["cut_state"] += 1
        if inv is not None and out["error"] is None:
            fail(inv, None, t)
        if cut:
            continue
        seen.add(t.tobytes())
        out["distinct"] += 1
        if keep_trace:
            states.append(t.copy())
            parent.append(-1)
        level.append((t.copy(), len(states) - 1))
    depth = 0
    while level and out["error"] is None:
        depth += 1
        out["level_width"].append(len(level))
        if depth in keep_levels:
            out["levels"][depth] = np.array([t for t, _ in level], dtype=np.uint64)
        if max_levels and depth >= max_levels:
            break
        nxt = []
        for s, sidx in level:
            succ, failed = pyoracle.successors(cfg, s)
            if succ is None:
                out["error"] = {"kind": "assertion", "action": failed}
                break
            if not succ and check_deadlock:
                out["error"] = {"kind": "deadlock"}
                break
            for a, x in succ:
                out["generated"] += 1
                act_gen[a] += 1
                cut = in_model(s, x, a, nc, np_, **kw)
                if on_pairs:
                    pS.append(s), pX.append(x.copy()), pA.append(pyoracle.ACTIONS.index(a)), pC.append(cut)
                    if len(pS) >= pair_chunk:
                        flush()
                if cut:
                    out["cut_state" if cut == CUT_STATE else "cut_action"] += 1
                    if out["first_cut_level"] is None:
                        out["first_cut_level"] = depth + 1
                    inv = violated(x, nc, np_, invariants)
                    if inv is not None:
                        fail(inv, sidx, x)
                        break
                    continue
                key = x.tobytes()
                if key in seen:
                    continue
                seen.add(key)
                out["distinct"] += 1
                act_dist[a] += 1
                inv = violated(x, nc, np_, invariants)
                if inv is not None:
                    fail(inv, sidx, x)
                    break
                xc = x.copy()
                if keep_trace:
                    states.append(xc)
                    parent.append(sidx)
                nxt.append((xc, len(states) - 1))
            if out["error"] is not None:
                break
        if out["error"] is not None:
            break
        level = nxt
    flush()
    out["depth"] = len(out["level_width"])
    out["complete"] = out["error"] is None and not level
    return out


# ---- the fixture file (tests/golden/constraint_fixtures.json)
ROWS = [   # id, (nc, np, ns), run() keywords
    ("model1_inflight1", (1, 1, 1), dict(inflight_max=1)),
    ("model1_inflight0", (1, 1, 1), dict(inflight_max=0)),
    ("model1_stored1", (1, 1, 1), dict(stored_max=1)),
    ("model1_stored2", (1, 1, 1), dict(stored_max=2)),
    ("model1_serve", (1, 1, 1), dict(serve_clients_first=True)),
    ("np2_stored1", (1, 2, 1), dict(stored_max=1)),
    ("np2_stored1_serve", (1, 2, 1), dict(stored_max=1, serve_clients_first=True)),
]
SMALL = ("model1_inflight0", "model1_stored1", "np2_stored1", "np2_stored1_serve")
# rule 4: seeded variant 2 (Force adds without replacing) under StoredAtMost<k>.
# At k = 1 no violation is reachable (the second Force is already outside the
# bound, and nothing reads a stored version before it); k = 2 is the smallest
# bound at which the host model finds one, and the violating state holds three
# objects: outside the constraint, every state before it inside.
RULE4 = dict(model=(1, 1, 1), variant=2, stored_max=2)
LEVELS_ROW = "np2_stored1"      # the run whose FIFO level sets are pinned


def _sha(a) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def row_fixture(rid: str) -> dict:
    (_, model, kw), = [r for r in ROWS if r[0] == rid]
    levels = ()
    if rid == LEVELS_ROW:
        probe = run(*model, **kw)
        levels = (probe["first_cut_level"], 1 + probe["level_width"].index(max(probe["level_width"])))
    r = run(*model, keep_levels=levels, **kw)
    assert r["error"] is None and r["complete"]
    out = {"model": list(model), "constraint": kw, "generated": r["generated"], "distinct": r["distinct"],
           "depth": r["depth"], "cut_state": r["cut_state"], "cut_action": r["cut_action"],
           "level_width": r["level_width"], "act_gen": r["act_gen"], "act_dist": r["act_dist"]}
    if levels:
        out["levels"] = {str(L): {"width": len(r["levels"][L]), "sha256": _sha(r["levels"][L])} for L in levels}
    return out


def rule4_fixture() -> dict:
    k1 = run(*RULE4["model"], variant=RULE4["variant"], stored_max=1)
    r = run(*RULE4["model"], variant=RULE4["variant"], stored_max=RULE4["stored_max"], keep_trace=True)
    e = r["error"]
    return {"model": list(RULE4["model"]), "variant": RULE4["variant"], "stored_max": RULE4["stored_max"],
            "violation_at_stored_max_1": k1["error"] is not None,
            "note": "no violation is reachable at k = 1; k = 2 is the smallest bound with one",
            "invariant": e["invariant"], "trace_len": e["trace_len"],
            "trace_stored": [stored(t) for t in e["trace"]], "trace": [[int(v) for v in t] for t in e["trace"]]}


def fixtures() -> dict:
    return {"rows": {rid: row_fixture(rid) for rid, _, _ in ROWS}, "rule4": rule4_fixture()}


if __name__ == "__main__":
    import json
    import sys
    json.dump(fixtures(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
