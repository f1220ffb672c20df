"""TLC-style command line for the KubeAPI model checker.

    python -m kubecheck.tlc [-config MC.cfg] [-deadlock] [-tool] [-nc N -np N -ns N]
                            [-variant V] [-workers N] [-fp K]
                            [-simulate [num=N]] [-depth D] [-seed S] [-continue]
                            [-fairness next|process] [-coverage [minutes]]
                            [-checkpoint MINUTES] [-checkpointlevels N] [-metadir DIR]
                            [-recover DIR] [MC]

Reads the same inputs as the reference's toolbox run: a TLC model config
(KubeAPI.toolbox/Model_1/MC.cfg:1-16 — CONSTANT assignments, either direct
`X = TRUE` or TLC's `X <- def` indirection resolved through MC.tla:5-12;
SPECIFICATION; INVARIANT) and prints TLC's `-tool` message stream
(@!@!@STARTMSG code:class ... @!@!@ENDMSG code) for the messages the
reference run shows (MC.out: 2262, 2187, 2185, 2189/2190, 2193 with both
collision estimates, 2201/2773/2772/2202 coverage with TLC's source spans,
2200 progress, 2199, 2194, 2268 outdegree, 2186) plus violation reports.
SANY's messages (2220/2219) are not produced (no TLA+ front end).  The
model check itself
runs on the GPU (kubecheck.ModelChecker); -workers and -fp are accepted for
command-line compatibility (the GPU replaces the worker pool; fingerprints
are kubecheck's own 64-bit hash, not TLC's FP64 #K).

Simulation mode (TLC's -simulate): with `-simulate [num=N]` a
kubecheck.Simulator runs instead of the ModelChecker: N seeded random
behaviours of at most `-depth D` states (default 100, TLC's), each state
checked against the invariants, the Asserts and deadlock.  `-seed S` makes the
run reproducible (default: from the clock); the run stops at the first launch
in which a behaviour errs unless `-continue` is given.  It prints a start
banner naming the seed, the walks and the depth; on an error the violation
message (2110/2132/2114), 2121 and the 2217 states of the behaviour, replayed
on the host; the coverage block with the steps taken per action in the place
of both counts; a totals line; 2186.  The exit code is 12 on an error, as for
the BFS.  Differences from TLC: N defaults to 65,536 behaviours (TLC's
-simulate runs until it is stopped), the random stream is kubecheck's own
(no -aril), and the reference holds no simulation output, so the
simulate-specific message bodies and codes claim no match with TLC's.
Without -simulate nothing changes.

Temporal properties: a cfg with a PROPERTY list (models/Liveness.cfg; the names
of kubecheck.PROPERTIES: KubeAPI.tla's ReconcileCompletes and CleansUpProperly,
and the build-defined ClientRestarts and SomeActorRestarts) first runs the BFS
exactly as without it.  If that ends without an error, each property is
checked in cfg order by a kubecheck.LivenessChecker under WF_vars(Next)
(include/kubecheck.h, "Liveness"), a 2192 line naming it, between the BFS
block and its closing 2186.  The first violation is reported and ends the run:
2116 "Temporal properties were violated.", 2264 "The following behavior
constitutes a counter-example:", the 2217 states, then 2122 "Back to state N"
or 2218 "Stuttering"; the exit code is 13.  The reference holds no liveness
output, so these codes and their wording claim no match with TLC's.
-simulate together with a PROPERTY list is an error.  Without a PROPERTY list
nothing changes.

Symmetry: `SYMMETRY name` in the cfg (models/Symmetry.cfg) turns on symmetry
reduction, TLC's way: the seen-set keeps one fingerprint per permutation
orbit, the states explored and every trace stay real states.  There is no
TLA+ front end, so no Permutations(...) expression: the name is one of the
build-defined sets SymClients, SymControllers (use with -np 2 or more) and
SymActors (both).  The 2187 banner then names the set, and the distinct
counts are orbit counts.  SYMMETRY together with a PROPERTY list or with
-simulate is an error (liveness under symmetry is unsound, as TLC warns; a
random walk has no seen-set to reduce).  Without the keyword nothing changes.

Constraints: `CONSTRAINT name ...` and `ACTION_CONSTRAINT name ...` in the cfg
(models/Constraint.cfg) are TLC's: a successor outside them is generated,
its invariants are checked, and it is discarded without a seen-set lookup
(DESIGN.md §4.11).  The names are build-defined, as the SYMMETRY sets are:
`StoredAtMost<k>`, `InFlightAtMost<k>` (one bound per family) and
`ServeClientsFirst`; several are conjoined.  The 2187 line names them with the
two discard counts.  Together with -simulate, a PROPERTY list, SYMMETRY,
-coverage or the checkpoint flags they are an error.

Expression-level coverage: with `-coverage` (TLC's flag; its optional
argument, the minutes between periodic reports, is accepted and ignored: only
the final block is printed) the engine also counts, on the GPU and over every
state it expands, the base counters of DESIGN.md §4.9, and the coverage block
carries TLC's per-expression lines between the per-action ones: 2221 (one
evaluation count per sub-expression), 2775 (count:cost of a set constructor)
and the 2774 headers of the invariants, in the order and with the spans of
MC.out:47-1090 (the table COVERAGE_LINES).  For Model_1 every count equals the
reference run's.  Five of the eight cost figures are not derived
(COVERAGE_COST_UNKNOWN): those lines print their count alone.  For other
process counts the lines are the same expressions with self sets of NC clients
and NP controllers; TLC pins none of them.  After a run that ends in an error
the block has the per-action lines only.  -coverage with -simulate, a PROPERTY
list or SYMMETRY is an error.  Without the flag nothing changes.

Checkpoint and recover: `-checkpoint MINUTES` (TLC's flag;
0 = none, as in TLC) makes the BFS write a checkpoint into `-metadir DIR`
(TLC's flag; default: `states` next to the .cfg) whenever that much time has
passed, `-checkpointlevels N` (kubecheck's own, as -fairness is: a run that
takes milliseconds cannot be cut by minutes) every N levels; each checkpoint
replaces the one before.  `-recover DIR` (TLC's flag) starts the search from
DIR's checkpoint instead of the initial states and reports cumulative
results.  Under -tool a run that wrote a checkpoint prints TLC's 2195
("Checkpointing of run ...") and 2196 ("Checkpointing completed at ...") once,
for the last one, and a recovered run prints 2197 ("Starting recovery from
checkpoint ...") and 2198 ("Recovery completed. N states examined. M states
on queue.") in place of the initial-state messages.  The reference holds no
checkpoint output: the codes and wording are recalled from TLC's message
table and claim no match.  These flags together with -simulate, a PROPERTY
list or -coverage are an error.

User-defined invariants: `-defs FILE` names a file of `Name == expr`
definitions (kubecheck.pred's language: TLA+-flavoured predicates over the
spec's variables; an expression may span lines up to the next `Name ==`
line).  An INVARIANT name of the cfg that is defined there is compiled to a
predicate program and checked on the GPU on every state the BFS expands
(DESIGN.md §4.13); a violation prints what a built-in one prints (2110
"Invariant Name is violated." and the behaviour).  A name found nowhere is the
unknown-invariant error it always was.  A user invariant with -simulate, a
PROPERTY list, SYMMETRY, CONSTRAINT / ACTION_CONSTRAINT, -coverage or the
checkpoint flags is an error (models/Reach.cfg, models/Reach.tla).

User-defined temporal properties: a PROPERTY name that is neither one of
kubecheck.PROPERTIES nor an action property and that the `-defs` file defines
is a temporal formula of the user's: P ~> Q, [](P => <>Q), []<>Q or <>Q over
kubecheck.pred's predicates (pred.parse_temporal).  It is
checked in cfg order with the built-in ones, by the same LivenessChecker under
the same fairness, with the same 2192 / 2116 / 2264 / 2217 messages and exit
code 13 (models/Eventually.cfg, models/Eventually.tla).  A definition without a
temporal operator listed under PROPERTY, <>[]Q, a bare []P and nested or
combined temporal formulas are errors that name the shape.  What a PROPERTY
list is refused with (-simulate, SYMMETRY, CONSTRAINT, -coverage, the
checkpoint flags, user INVARIANTs) is refused with these too.

`-fairness process` checks the properties under weak
fairness of every process (PlusCal's `fair process`; a .cfg cannot say this,
so it is an option) instead of WF_vars(Next), the default; the 2192 line names
the fairness assumed.  It is refused together with -simulate.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import re
import sys
import time
from typing import Dict, List, Optional

KNOWN_INVARIANTS = ("TypeOK", "OnlyOneVersion")          # KubeAPI.tla:776,787
# build-defined (not in KubeAPI.tla): no Update overwrites a version its
# writer has not read (the optimistic concurrency HasRead gives Update,
# :733), with its lostUpdate history variable; run with -variant 1 it fails
BUILD_INVARIANTS = ("NoLostUpdate",)
# build-defined symmetry sets (there is no Permutations(...) to evaluate):
# the cfg's SYMMETRY name -> ModelConfig.symmetry
SYMMETRY_NAMES = {"SymClients": "clients", "SymControllers": "controllers", "SymActors": "actors"}
# build-defined constraints (there is no TLA+ expression evaluator): the cfg's
# CONSTRAINT names StoredAtMost<k> (Cardinality(apiState) <= k) and
# InFlightAtMost<k> (pending requests + pending list requests <= k), one bound
# per family; the ACTION_CONSTRAINT names -> ModelConfig.action_constraints
CONSTRAINT_FAMILIES = {"StoredAtMost": "constraint_stored", "InFlightAtMost": "constraint_inflight"}
ACTION_CONSTRAINT_NAMES = ("ServeClientsFirst",)
KNOWN_CONSTRAINTS = tuple(f + "<k>" for f in CONSTRAINT_FAMILIES) + ACTION_CONSTRAINT_NAMES
# build-defined action properties (a PROPERTY whose formula is [][A]_vars;
# there is no TLA+ expression evaluator): the names of kubecheck.ACTION_PROPERTIES
ACTION_PROPERTY_NAMES = ("NoBlindUpdate", "OneReplyPerStep", "StoreNeverShrinks")
KNOWN_CONSTANTS = ("REQUESTS_CAN_FAIL", "REQUESTS_CAN_TIMEOUT", "defaultInitValue")  # :4-6,374


class CfgError(ValueError):
    pass


def _strip_comments(text: str) -> str:
    text = re.sub(r"\(\*.*?\*\)", " ", text, flags=re.S)
    return "\n".join(line.split("\\*", 1)[0] for line in text.splitlines())


def parse_defs(tla_text: str) -> Dict[str, str]:
    """`name == value` definitions of a TLC-generated MC.tla (MC.tla:5-12)."""
    out = {}
    for m in re.finditer(r"^(\w+)\s*==\s*\n?\s*(\S+)", _strip_comments(tla_text), flags=re.M):
        out[m.group(1)] = m.group(2)
    return out


def parse_cfg(cfg_text: str, defs: Optional[Dict[str, str]] = None) -> dict:
    """Parse a TLC .cfg (the subset MC.cfg uses)."""
    defs = defs or {}
    toks = _strip_comments(cfg_text).split()
    out: dict = {"constants": {}, "specification": None, "invariants": [], "properties": [],
                 "symmetry": None, "constraints": [], "action_constraints": []}
    i, section = 0, None
    keywords = {"CONSTANT", "CONSTANTS", "SPECIFICATION", "INVARIANT", "INVARIANTS",
                "PROPERTY", "PROPERTIES", "INIT", "NEXT", "SYMMETRY",
                "CONSTRAINT", "CONSTRAINTS", "ACTION_CONSTRAINT", "ACTION_CONSTRAINTS"}
    while i < len(toks):
        t = toks[i]
        if t in keywords:
            section = t
            i += 1
            continue
        if section in ("CONSTANT", "CONSTANTS"):
            if i + 2 < len(toks) + 1 and i + 1 < len(toks) and toks[i + 1] in ("=", "<-"):
                name, op, val = t, toks[i + 1], toks[i + 2]
                if op == "<-":
                    if val not in defs:
                        raise CfgError(f"{name} <- {val}: definition {val} not found in MC.tla")
                    val = defs[val]
                out["constants"][name] = val
                i += 3
                continue
            raise CfgError(f"bad CONSTANT entry near {t!r}")
        if section == "SPECIFICATION":
            out["specification"] = t
        elif section in ("INVARIANT", "INVARIANTS"):
            out["invariants"].append(t)
        elif section in ("PROPERTY", "PROPERTIES"):
            out["properties"].append(t)
        elif section == "SYMMETRY":
            if out["symmetry"] is not None:
                raise CfgError(f"SYMMETRY takes one name, got {out['symmetry']!r} and {t!r}")
            if t not in SYMMETRY_NAMES:
                raise CfgError(f"SYMMETRY {t}: expected one of {tuple(SYMMETRY_NAMES)} (build-defined; "
                               "Permutations(...) expressions are not evaluated)")
            out["symmetry"] = t
        elif section in ("CONSTRAINT", "CONSTRAINTS"):
            m = re.fullmatch(r"(StoredAtMost|InFlightAtMost)(\d+)", t)
            if not m:
                raise CfgError(f"CONSTRAINT {t}: expected one of {KNOWN_CONSTRAINTS[:2]} (build-defined; "
                               f"TLA+ expressions are not evaluated; known names: {KNOWN_CONSTRAINTS})")
            if any(c.startswith(m.group(1)) for c in out["constraints"]):
                raise CfgError(f"CONSTRAINT {t}: a second {m.group(1)}<k> bound (one per family)")
            out["constraints"].append(t)
        elif section in ("ACTION_CONSTRAINT", "ACTION_CONSTRAINTS"):
            if t not in ACTION_CONSTRAINT_NAMES:
                raise CfgError(f"ACTION_CONSTRAINT {t}: expected one of {ACTION_CONSTRAINT_NAMES} (build-defined; "
                               f"known names: {KNOWN_CONSTRAINTS})")
            if t not in out["action_constraints"]:
                out["action_constraints"].append(t)
        else:
            raise CfgError(f"unsupported cfg token {t!r}")
        i += 1
    return out


def model_from_cfg(cfg: dict) -> dict:
    """Validate a parsed cfg against KubeAPI.tla and map it to ModelConfig kwargs."""
    if cfg["specification"] not in (None, "Spec"):
        raise CfgError(f"SPECIFICATION {cfg['specification']}: only Spec (KubeAPI.tla:765)")
    bad = [x for x in cfg["invariants"] if x not in KNOWN_INVARIANTS + BUILD_INVARIANTS]
    if bad:
        raise CfgError(f"unknown invariant(s) {bad}; KubeAPI.tla defines {KNOWN_INVARIANTS}"
                       f" (and the build {BUILD_INVARIANTS})")
    if cfg["properties"]:
        raise CfgError("temporal PROPERTY checking (liveness) is out of scope")
    kw = {}
    for name, key in (("REQUESTS_CAN_FAIL", "can_fail"), ("REQUESTS_CAN_TIMEOUT", "can_timeout")):
        v = cfg["constants"].get(name)
        if v not in ("TRUE", "FALSE"):
            raise CfgError(f"{name} must be TRUE or FALSE (ASSUME, KubeAPI.tla:8-9), got {v!r}")
        kw[key] = v == "TRUE"
    unknown = set(cfg["constants"]) - set(KNOWN_CONSTANTS)
    if unknown:
        raise CfgError(f"unknown CONSTANT(s) {sorted(unknown)}")
    # the INVARIANT list selects the checks (an empty list checks none, as in TLC)
    kw["invariants"] = (1 if "TypeOK" in cfg["invariants"] else 0) | \
        (2 if "OnlyOneVersion" in cfg["invariants"] else 0) | \
        (4 if "NoLostUpdate" in cfg["invariants"] else 0)
    if cfg.get("symmetry"):
        kw["symmetry"] = SYMMETRY_NAMES[cfg["symmetry"]]
    for c in cfg.get("constraints") or []:
        m = re.fullmatch(r"(StoredAtMost|InFlightAtMost)(\d+)", c)
        if not m:
            raise CfgError(f"CONSTRAINT {c}: known names: {KNOWN_CONSTRAINTS}")
        if CONSTRAINT_FAMILIES[m.group(1)] in kw:
            raise CfgError(f"CONSTRAINT {c}: a second {m.group(1)}<k> bound (one per family)")
        kw[CONSTRAINT_FAMILIES[m.group(1)]] = int(m.group(2))
    if cfg.get("action_constraints"):
        bad = [x for x in cfg["action_constraints"] if x not in ACTION_CONSTRAINT_NAMES]
        if bad:
            raise CfgError(f"unknown ACTION_CONSTRAINT(s) {bad}; known names: {KNOWN_CONSTRAINTS}")
        kw["action_constraints"] = list(cfg["action_constraints"])
    if ("constraint_stored" in kw or "constraint_inflight" in kw or "action_constraints" in kw) and cfg.get("symmetry"):
        raise CfgError(f"CONSTRAINT / ACTION_CONSTRAINT with SYMMETRY {cfg['symmetry']}: TLC needs a symmetric "
                       "constraint, and these would each need an argument")
    return kw


def split_user_invariants(cfg: dict, defs: Optional[Dict[str, str]], procs=(1, 1, 1), simulate: bool = False,
                          coverage: bool = False, checkpointing: bool = False):
    """Take the INVARIANT names that `defs` (-defs FILE: name -> predicate
    text) defines out of a parsed cfg: (the cfg without them, {name: text} in
    cfg order).  A name that is neither built in nor defined stays, and
    model_from_cfg reports it as it always did.  The predicates are compiled
    here (no GPU), so a bad one is a CfgError before anything runs."""
    from . import pred

    builtin = KNOWN_INVARIANTS + BUILD_INVARIANTS
    user = {x: defs[x] for x in cfg["invariants"] if x not in builtin and defs and x in defs}
    if not user:
        return cfg, {}
    names = " ".join(user)
    if simulate:
        raise CfgError(f"user-defined INVARIANT ({names}) with -simulate: the walks check the built-in invariants only")
    if cfg["properties"]:
        raise CfgError(f"user-defined INVARIANT ({names}) with a PROPERTY list: not supported together")
    if cfg.get("symmetry"):
        raise CfgError(f"user-defined INVARIANT ({names}) with SYMMETRY {cfg['symmetry']}: a predicate that names a "
                       "process is not orbit-invariant")
    if cfg.get("constraints") or cfg.get("action_constraints"):
        raise CfgError(f"user-defined INVARIANT ({names}) with CONSTRAINT / ACTION_CONSTRAINT: TLC checks invariants on "
                       "the successors a constraint discards; they are never expanded here, so they would be missed")
    if coverage:
        raise CfgError(f"user-defined INVARIANT ({names}) with -coverage: not supported together")
    if checkpointing:
        raise CfgError(f"user-defined INVARIANT ({names}) with -checkpoint / -recover: a checkpoint holds no "
                       "invariant counts")
    try:
        pred.compile_invariants(user, *procs)
    except pred.PredError as e:
        raise CfgError(f"user-defined INVARIANT {e}") from None
    return dict(cfg, invariants=[x for x in cfg["invariants"] if x not in user]), user


def split_user_properties(cfg: dict, defs: Optional[Dict[str, str]], procs=(1, 1, 1)) -> Dict[str, str]:
    """The PROPERTY names of a parsed cfg that are neither kubecheck's
    PROPERTIES nor action properties and that `defs` (-defs FILE: name ->
    text) defines: {name: formula text} in cfg order.  Each is compiled here
    (no GPU), so a definition without a temporal operator, a shape that is not
    supported or a bad predicate is a CfgError before anything runs.  A name
    defined nowhere stays the unknown-property error it always was."""
    from . import pred
    from ._lib import PROPERTIES

    user: Dict[str, str] = {}
    for x in cfg["properties"]:
        if x in PROPERTIES or x in ACTION_PROPERTY_NAMES or not defs or x not in defs or x in user:
            continue
        try:
            if not pred.has_temporal(defs[x]):
                raise CfgError(f"PROPERTY {x}: its definition has no temporal operator (~>, <>, []): a state "
                               "predicate: list it under INVARIANT")
            pred.compile_temporal(defs[x], *procs)
        except pred.PredError as e:
            raise CfgError(f"user-defined PROPERTY {x}: {e}") from None
        user[x] = defs[x]
    return user


def check_from_cfg(cfg: dict, simulate: bool = False, coverage: bool = False, checkpointing: bool = False,
                   user_props: Optional[Dict[str, str]] = None):
    """model_from_cfg for a cfg that may list temporal properties: (ModelConfig
    kwargs, the PROPERTY names in cfg order).  The names must be kubecheck's
    PROPERTIES or keys of user_props (split_user_properties: the user's
    temporal formulas); simulation mode checks none.  coverage: -coverage was
    given; checkpointing: one of -checkpoint, -checkpointlevels, -recover was."""
    from ._lib import PROPERTIES

    # a PROPERTY list may mix temporal names (the liveness phase, after a clean
    # BFS) and action properties ([][A]_vars: checked by the BFS on every step)
    act_props = [x for x in cfg["properties"] if x in ACTION_PROPERTY_NAMES]
    props = [x for x in cfg["properties"] if x not in ACTION_PROPERTY_NAMES]
    if act_props:
        # action properties: the single-GPU in-HBM BFS alone
        names = " ".join(act_props)
        if cfg.get("constraints") or cfg.get("action_constraints"):
            raise CfgError(f"action PROPERTY ({names}) with CONSTRAINT / ACTION_CONSTRAINT: not supported together")
        if cfg.get("symmetry"):
            raise CfgError(f"action PROPERTY ({names}) with SYMMETRY {cfg['symmetry']}: a step is checked between "
                           "real states, the seen-set holds orbits")
        if simulate:
            raise CfgError(f"action PROPERTY ({names}) with -simulate: the walks check invariants only")
        if coverage:
            raise CfgError(f"action PROPERTY ({names}) with -coverage: the coverage counters name none")
        if checkpointing:
            raise CfgError(f"action PROPERTY ({names}) with -checkpoint / -recover: a checkpoint names none")
    if cfg.get("constraints") or cfg.get("action_constraints"):
        # constraints: the single-GPU BFS alone
        names = " ".join(list(cfg.get("constraints") or []) + list(cfg.get("action_constraints") or []))
        if simulate:
            raise CfgError(f"CONSTRAINT / ACTION_CONSTRAINT ({names}) with -simulate: the walks step through Next alone")
        if props:
            raise CfgError(f"CONSTRAINT / ACTION_CONSTRAINT ({names}) with a PROPERTY list: liveness is checked on "
                           "the unconstrained behaviour graph")
        if cfg.get("symmetry"):
            raise CfgError(f"CONSTRAINT / ACTION_CONSTRAINT ({names}) with SYMMETRY {cfg['symmetry']}: TLC needs a "
                           "symmetric constraint, and these would each need an argument")
        if coverage:
            raise CfgError(f"CONSTRAINT / ACTION_CONSTRAINT ({names}) with -coverage: not counted under constraints")
        if checkpointing:
            raise CfgError(f"CONSTRAINT / ACTION_CONSTRAINT ({names}) with -checkpoint / -recover: a checkpoint "
                           "names no constraint")
    if checkpointing and props:
        raise CfgError("-checkpoint / -recover with a PROPERTY list: a checkpoint holds the BFS's state, "
                       "not the liveness graph")
    if coverage and simulate:
        raise CfgError("-coverage with -simulate: expression-level coverage is counted by the BFS only")
    if coverage and props:
        raise CfgError("-coverage with a PROPERTY list: expression-level coverage is counted by the BFS only")
    if coverage and cfg.get("symmetry"):
        raise CfgError(f"-coverage with SYMMETRY {cfg['symmetry']}: the states explored stand for orbits, "
                       "so the counts would be no evaluation counts")
    bad = [x for x in props if x not in PROPERTIES and x not in (user_props or {})]
    if bad:
        raise CfgError(f"unknown temporal property(ies) {bad}; known: {PROPERTIES}; "
                       f"action properties: {ACTION_PROPERTY_NAMES}; a formula of your own: define it in the "
                       "-defs file")
    if props and simulate:
        raise CfgError("-simulate checks no temporal PROPERTY (liveness needs the whole state graph)")
    if cfg.get("symmetry") and props:
        raise CfgError(f"SYMMETRY {cfg['symmetry']} with a PROPERTY list: liveness checking under symmetry "
                       "reduction is unsound")
    if cfg.get("symmetry") and simulate:
        raise CfgError(f"SYMMETRY {cfg['symmetry']} with -simulate: a random walk has no seen-set to reduce")
    kw = model_from_cfg(dict(cfg, properties=[]))
    if act_props:
        kw["action_properties"] = tuple(dict.fromkeys(act_props))
    return kw, props


def msg(code: int, text: str, cls: int = 0, tool: bool = True) -> str:
    if not tool:
        return text
    return f"@!@!@STARTMSG {code}:{cls} @!@!@\n{text}\n@!@!@ENDMSG {code} @!@!@"


# Source locations TLC's coverage messages print for each action (msg 2772)
# and for Init (msg 2773): the definition heads in KubeAPI.tla, e.g.
# "DoRequest(self) ==" at KubeAPI.tla:471, columns 1-15 (MC.out:78-621, :48).
INIT_SPAN = (455, 1, 455, 4)
ACTION_SPANS = {
    "DoRequest": (471, 1, 471, 15), "DoReply": (485, 1, 485, 13),
    "DoListRequest": (499, 1, 499, 19), "DoListReply": (513, 1, 513, 17),
    "CStart": (528, 1, 528, 12), "C1": (551, 1, 551, 8), "C10": (558, 1, 558, 9),
    "C11": (570, 1, 570, 9), "c12": (577, 1, 577, 9), "C13": (589, 1, 589, 9),
    "C2": (596, 1, 596, 8), "C3": (604, 1, 604, 8), "C8": (611, 1, 611, 8),
    "C6": (618, 1, 618, 8), "C7": (631, 1, 631, 8), "C4": (638, 1, 638, 8),
    "C5": (645, 1, 645, 8), "PVCStart": (655, 1, 655, 14), "PVCListedPVCs": (665, 1, 665, 19),
    "PVCHavePVCs": (673, 1, 673, 17), "PVCDone": (690, 1, 690, 13), "APIStart": (698, 1, 698, 14),
}


# Expression-level coverage (TLC's -coverage): every message
# of the reference run's coverage block (MC.out:47-1090) in its order, as
#   (message code, nesting depth, span in KubeAPI.tla, formula[, cost formula]).
# 2773 / 2772 / 2774 rows head Init, an action or an invariant and carry its
# name in the formula's place.  A 2221 / 2775 formula is a fixed integer
# combination of the run's summed base counters (csrc/cover.h, the names of
# kubecheck.cover_names()), gen_<Action> (act_gen), init, and the sizes of the
# self sets P = |ProcSet|, NC, NP, NS.  The rules behind them:
#   * a guard conjunct counts its evaluations plus the pairs that go on to
#     produce a successor: |self set| * states + enabled pairs;
#   * \E and CHOOSE over apiState stop at the first match, a set comprehension
#     visits every element, in the order Secret before PVC;
#   * an argument bound to a primed expression is evaluated at every use
#     (:722 requests'[c].obj: once per o1.n and once more per o1.k).
# A 2775 cost is count + the sizes of the sets built where that explains the
# recorded number; None where it does not (COVERAGE_COST_UNKNOWN).
COVERAGE_LINES = (
    (2773, 0, (455, 1, 455, 4), 'Init'),
    (2221, 0, (456, 12, 456, 24), '1'),
    (2221, 0, (457, 12, 457, 39), '1'),
    (2221, 0, (458, 12, 458, 43), '1'),
    (2221, 0, (460, 12, 460, 56), '1'),
    (2221, 0, (461, 12, 461, 57), '1'),
    (2221, 0, (463, 12, 463, 58), '1'),
    (2221, 0, (465, 12, 465, 54), '1'),
    (2221, 0, (466, 12, 466, 47), 'init'),
    (2221, 0, (467, 12, 469, 77), 'init'),
    (2772, 0, (471, 1, 471, 15), 'DoRequest'),
    (2221, 0, (471, 23, 471, 44), 'P*states + pairs_DoRequest'),
    (2221, 1, (471, 23, 471, 30), 'P*states'),
    (2221, 0, (472, 26, 475, 53), 'pairs_DoRequest'),
    (2221, 0, (476, 29, 476, 69), 'pairs_DoRequest'),
    (2221, 0, (477, 29, 480, 53), 'gen_DoRequest - pairs_DoRequest'),
    (2221, 0, (481, 23, 481, 59), 'gen_DoRequest'),
    (2221, 0, (482, 23, 483, 59), 'gen_DoRequest'),
    (2772, 0, (485, 1, 485, 13), 'DoReply'),
    (2221, 0, (485, 21, 485, 40), 'P*states + en_DoReply'),
    (2221, 1, (485, 21, 485, 28), 'P*states'),
    (2221, 0, (486, 21, 486, 53), 'pairs_DoReply + en_DoReply'),
    (2221, 1, (486, 21, 486, 41), 'pairs_DoReply'),
    (2221, 0, (487, 27, 487, 30), 'en_DoReply'),
    (2221, 0, (488, 27, 488, 44), 'en_DoReply'),
    (2221, 0, (489, 24, 490, 80), 'en_DoReply'),
    (2221, 0, (491, 21, 491, 68), 'gen_DoReply'),
    (2221, 0, (492, 21, 492, 68), 'gen_DoReply'),
    (2221, 0, (493, 21, 493, 71), 'gen_DoReply'),
    (2221, 0, (494, 21, 494, 71), 'gen_DoReply'),
    (2221, 0, (495, 21, 495, 81), 'gen_DoReply'),
    (2772, 0, (499, 1, 499, 19), 'DoListRequest'),
    (2221, 0, (499, 27, 499, 52), 'P*states + pairs_DoListRequest'),
    (2221, 1, (499, 27, 499, 34), 'P*states'),
    (2221, 0, (500, 30, 503, 65), 'pairs_DoListRequest'),
    (2221, 0, (504, 33, 504, 73), 'pairs_DoListRequest'),
    (2221, 0, (505, 33, 508, 65), 'gen_DoListRequest - pairs_DoListRequest'),
    (2221, 0, (509, 27, 509, 67), 'gen_DoListRequest'),
    (2221, 0, (510, 27, 511, 63), 'gen_DoListRequest'),
    (2772, 0, (513, 1, 513, 17), 'DoListReply'),
    (2221, 0, (513, 25, 513, 48), 'P*states + en_DoListReply'),
    (2221, 1, (513, 25, 513, 32), 'P*states'),
    (2221, 0, (514, 25, 514, 61), 'pairs_DoListReply + en_DoListReply'),
    (2221, 1, (514, 25, 514, 49), 'pairs_DoListReply'),
    (2221, 0, (515, 31, 515, 34), 'en_DoListReply'),
    (2221, 0, (516, 31, 516, 52), 'en_DoListReply'),
    (2221, 0, (517, 28, 519, 92), 'en_DoListReply'),
    (2221, 0, (520, 25, 520, 72), 'gen_DoListReply'),
    (2221, 0, (521, 25, 521, 78), 'gen_DoListReply'),
    (2221, 0, (522, 25, 522, 75), 'gen_DoListReply'),
    (2221, 0, (523, 25, 524, 55), 'gen_DoListReply'),
    (2772, 0, (528, 1, 528, 12), 'CStart'),
    (2221, 0, (528, 20, 528, 38), 'NC*states + pairs_CStart'),
    (2221, 1, (528, 20, 528, 27), 'NC*states'),
    (2221, 0, (529, 23, 529, 83), 'pairs_CStart'),
    (2221, 0, (530, 26, 530, 29), 'pairs_CStart'),
    (2221, 0, (531, 26, 531, 50), 'pairs_CStart'),
    (2221, 0, (532, 23, 532, 44), 'gen_CStart'),
    (2221, 0, (533, 28, 541, 42), 'B_CSTART_THEN'),
    (2221, 0, (542, 31, 546, 82), 'B_CSTART_ELSE'),
    (2221, 0, (547, 31, 547, 73), 'B_CSTART_ELSE'),
    (2221, 0, (548, 31, 548, 53), 'B_CSTART_ELSE'),
    (2221, 0, (549, 20, 549, 67), 'gen_CStart'),
    (2772, 0, (551, 1, 551, 8), 'C1'),
    (2221, 0, (551, 16, 551, 30), 'NC*states + pairs_C1'),
    (2221, 1, (551, 16, 551, 23), 'NC*states'),
    (2221, 0, (552, 19, 552, 46), 'gen_C1'),
    (2221, 0, (553, 24, 553, 62), 'B_C1_START'),
    (2221, 0, (554, 24, 554, 59), 'B_C1_C10'),
    (2221, 0, (555, 16, 556, 52), 'gen_C1'),
    (2772, 0, (558, 1, 558, 9), 'C10'),
    (2221, 0, (558, 17, 558, 32), 'NC*states + pairs_C10'),
    (2221, 1, (558, 17, 558, 24), 'NC*states'),
    (2221, 0, (559, 17, 565, 68), 'gen_C10'),
    (2221, 0, (566, 17, 566, 55), 'gen_C10'),
    (2221, 0, (567, 17, 568, 47), 'gen_C10'),
    (2772, 0, (570, 1, 570, 9), 'C11'),
    (2221, 0, (570, 17, 570, 32), 'NC*states + pairs_C11'),
    (2221, 1, (570, 17, 570, 24), 'NC*states'),
    (2221, 0, (571, 20, 571, 47), 'gen_C11'),
    (2221, 0, (572, 25, 572, 63), 'B_C11_START'),
    (2221, 0, (573, 25, 573, 60), 'B_C11_c12'),
    (2221, 0, (574, 17, 575, 53), 'gen_C11'),
    (2772, 0, (577, 1, 577, 9), 'c12'),
    (2221, 0, (577, 17, 577, 32), 'NC*states + pairs_c12'),
    (2221, 1, (577, 17, 577, 24), 'NC*states'),
    (2221, 0, (578, 17, 584, 68), 'gen_c12'),
    (2221, 0, (585, 17, 585, 55), 'gen_c12'),
    (2221, 0, (586, 17, 587, 47), 'gen_c12'),
    (2772, 0, (589, 1, 589, 9), 'C13'),
    (2221, 0, (589, 17, 589, 32), 'NC*states + pairs_C13'),
    (2221, 1, (589, 17, 589, 24), 'NC*states'),
    (2221, 0, (590, 20, 590, 83), 'gen_C13'),
    (2221, 1, (590, 20, 590, 47), 'gen_C13'),
    (2221, 1, (590, 52, 590, 83), 'c13_ok'),
    (2221, 2, (444, 22, 446, 58), 'c13_ok'),
    (2221, 3, (444, 25, 444, 37), 'c13_ok'),
    (2221, 3, (445, 25, 446, 58), 'c13_pvc'),
    (2221, 4, (445, 28, 445, 51), 'c13_pvc'),
    (2221, 4, (446, 28, 446, 58), 'c13_spec'),
    (2221, 2, (590, 65, 590, 82), 'c13_ok'),
    (2221, 0, (591, 25, 591, 63), 'B_C13_START'),
    (2221, 0, (592, 25, 592, 59), 'B_C13_C2'),
    (2221, 0, (593, 17, 594, 53), 'gen_C13'),
    (2772, 0, (596, 1, 596, 8), 'C2'),
    (2221, 0, (596, 16, 596, 30), 'NC*states + pairs_C2'),
    (2221, 1, (596, 16, 596, 23), 'NC*states'),
    (2221, 0, (597, 16, 597, 74), 'gen_C2'),
    (2221, 0, (598, 16, 599, 68), 'gen_C2'),
    (2221, 0, (600, 16, 600, 47), 'gen_C2'),
    (2221, 0, (601, 16, 602, 35), 'gen_C2'),
    (2772, 0, (604, 1, 604, 8), 'C3'),
    (2221, 0, (604, 16, 604, 30), 'NC*states + pairs_C3'),
    (2221, 1, (604, 16, 604, 23), 'NC*states'),
    (2221, 0, (605, 19, 605, 50), 'gen_C3'),
    (2221, 0, (606, 24, 606, 62), 'B_C3_START'),
    (2221, 0, (607, 24, 607, 58), 'B_C3_C8'),
    (2221, 0, (608, 16, 609, 52), 'gen_C3'),
    (2772, 0, (611, 1, 611, 8), 'C8'),
    (2221, 0, (611, 16, 611, 30), 'NC*states + pairs_C8'),
    (2221, 1, (611, 16, 611, 23), 'NC*states'),
    (2221, 0, (612, 19, 612, 46), 'gen_C8'),
    (2221, 0, (613, 24, 613, 58), 'B_C8_C4'),
    (2221, 0, (614, 24, 614, 58), 'B_C8_C6'),
    (2221, 0, (615, 16, 616, 52), 'gen_C8'),
    (2772, 0, (618, 1, 618, 8), 'C6'),
    (2221, 0, (618, 16, 618, 30), 'NC*states + pairs_C6'),
    (2221, 1, (618, 16, 618, 23), 'NC*states'),
    (2221, 0, (619, 16, 627, 59), 'pairs_C6'),
    (2221, 0, (628, 16, 629, 46), 'gen_C6'),
    (2772, 0, (631, 1, 631, 8), 'C7'),
    (2221, 0, (631, 16, 631, 30), 'NC*states + pairs_C7'),
    (2221, 1, (631, 16, 631, 23), 'NC*states'),
    (2221, 0, (632, 19, 632, 90), 'gen_C7'),
    (2221, 1, (632, 19, 632, 46), 'gen_C7'),
    (2221, 1, (632, 51, 632, 90), 'c7_ok'),
    (2221, 0, (633, 24, 633, 62), 'B_C7_START'),
    (2221, 0, (634, 24, 634, 58), 'B_C7_C4'),
    (2221, 0, (635, 16, 636, 52), 'gen_C7'),
    (2772, 0, (638, 1, 638, 8), 'C4'),
    (2221, 0, (638, 16, 638, 30), 'NC*states + pairs_C4'),
    (2221, 1, (638, 16, 638, 23), 'NC*states'),
    (2221, 0, (639, 16, 640, 68), 'gen_C4'),
    (2221, 1, (639, 23, 639, 66), 'gen_C4'),
    (2221, 2, (639, 24, 639, 66), 'gen_C4'),
    (2221, 3, (410, 22, 410, 59), 'gen_C4'),
    (2221, 4, (410, 41, 410, 59), 'c4_iter'),
    (2221, 4, (410, 31, 410, 38), 'gen_C4'),
    (2221, 3, (639, 37, 639, 65), 'c4_iter'),
    (2221, 0, (641, 16, 641, 47), 'gen_C4'),
    (2221, 0, (642, 16, 643, 52), 'gen_C4'),
    (2772, 0, (645, 1, 645, 8), 'C5'),
    (2221, 0, (645, 16, 645, 30), 'NC*states + pairs_C5'),
    (2221, 1, (645, 16, 645, 23), 'NC*states'),
    (2221, 0, (646, 16, 646, 51), 'gen_C5'),
    (2221, 0, (647, 16, 648, 52), 'gen_C5'),
    (2772, 0, (655, 1, 655, 14), 'PVCStart'),
    (2221, 0, (655, 22, 655, 42), 'NP*states + pairs_PVCStart'),
    (2221, 1, (655, 22, 655, 29), 'NP*states'),
    (2221, 0, (656, 22, 660, 73), 'gen_PVCStart'),
    (2221, 0, (661, 22, 661, 64), 'gen_PVCStart'),
    (2221, 0, (662, 22, 663, 52), 'gen_PVCStart'),
    (2772, 0, (665, 1, 665, 19), 'PVCListedPVCs'),
    (2221, 0, (665, 27, 665, 52), 'NP*states + pairs_PVCListedPVCs'),
    (2221, 1, (665, 27, 665, 34), 'NP*states'),
    (2221, 0, (666, 30, 667, 85), 'gen_PVCListedPVCs'),
    (2221, 1, (666, 33, 666, 64), 'gen_PVCListedPVCs'),
    (2221, 1, (667, 33, 667, 85), 'pvcl_ok'),
    (2221, 2, (667, 33, 667, 80), 'pvcl_ok'),
    (2221, 3, (667, 65, 667, 79), 'pvcl_objs'),
    (2221, 4, (444, 22, 446, 58), 'pvcl_objs'),
    (2221, 5, (444, 25, 444, 37), 'pvcl_objs'),
    (2221, 5, (445, 25, 446, 58), 'pvcl_objs_pvc'),
    (2221, 6, (445, 28, 445, 51), 'pvcl_objs_pvc'),
    (2221, 6, (446, 28, 446, 58), 'pvcl_objs_spec'),
    (2221, 4, (667, 78, 667, 78), 'pvcl_objs'),
    (2221, 3, (667, 40, 667, 62), 'pvcl_ok'),
    (2221, 2, (667, 84, 667, 85), 'pvcl_ok'),
    (2221, 0, (668, 35, 668, 75), 'B_PVCL_START'),
    (2221, 0, (669, 35, 669, 78), 'B_PVCL_HAVE'),
    (2221, 0, (670, 27, 671, 72), 'gen_PVCListedPVCs'),
    (2772, 0, (673, 1, 673, 17), 'PVCHavePVCs'),
    (2221, 0, (673, 25, 673, 48), 'NP*states + pairs_PVCHavePVCs'),
    (2221, 1, (673, 25, 673, 32), 'NP*states'),
    (2221, 0, (674, 25, 686, 70), 'pairs_PVCHavePVCs'),
    (2221, 0, (687, 25, 688, 55), 'gen_PVCHavePVCs'),
    (2772, 0, (690, 1, 690, 13), 'PVCDone'),
    (2221, 0, (690, 21, 690, 40), 'NP*states + pairs_PVCDone'),
    (2221, 1, (690, 21, 690, 28), 'NP*states'),
    (2221, 0, (691, 21, 691, 58), 'gen_PVCDone'),
    (2221, 0, (692, 21, 693, 62), 'gen_PVCDone'),
    (2772, 0, (698, 1, 698, 14), 'APIStart'),
    (2221, 0, (698, 22, 698, 42), 'NS*states + en_APIStart'),
    (2221, 1, (698, 22, 698, 29), 'NS*states'),
    (2221, 0, (700, 33, 700, 57), 'B_API_CREATE + B_API_FORCE + B_API_GET + B_API_DELETE + B_API_UPDATE + B_API_ASSERT'),
    (2221, 0, (702, 52, 702, 102), 'create_exists'),
    (2221, 0, (703, 52, 703, 69), 'create_exists'),
    (2221, 0, (704, 52, 704, 103), 'B_API_CREATE - create_exists'),
    (2221, 0, (705, 52, 705, 99), 'B_API_CREATE - create_exists'),
    (2221, 0, (706, 44, 706, 67), 'B_API_FORCE + B_API_GET + B_API_DELETE + B_API_UPDATE + B_API_ASSERT'),
    (2221, 0, (707, 55, 707, 104), 'B_API_FORCE'),
    (2221, 1, (707, 74, 707, 104), 'force_iter'),
    (2221, 2, (390, 24, 390, 49), 'force_iter'),
    (2221, 3, (390, 24, 390, 34), 'force_iter'),
    (2221, 3, (390, 39, 390, 49), 'B_API_FORCE_REPLACE'),
    (2221, 2, (707, 86, 707, 86), 'force_iter'),
    (2221, 2, (707, 89, 707, 103), 'force_iter'),
    (2221, 1, (707, 64, 707, 71), 'B_API_FORCE'),
    (2221, 0, (708, 63, 713, 91), 'B_API_FORCE_REPLACE'),
    (2775, 1, (708, 83, 713, 91), 'B_API_FORCE_REPLACE', None),
    (2221, 2, (709, 75, 712, 79), 'force_setsz'),
    (2221, 3, (709, 78, 709, 108), 'force_setsz'),
    (2221, 4, (390, 24, 390, 49), 'force_setsz'),
    (2221, 5, (390, 24, 390, 34), 'force_setsz'),
    (2221, 5, (390, 39, 390, 49), 'force_same'),
    (2221, 4, (709, 90, 709, 90), 'force_setsz'),
    (2221, 4, (709, 93, 709, 107), 'force_setsz'),
    (2221, 3, (710, 79, 710, 100), 'force_same'),
    (2221, 3, (712, 79, 712, 79), 'force_setsz - force_same'),
    (2221, 2, (713, 83, 713, 90), 'B_API_FORCE_REPLACE'),
    (2221, 0, (714, 60, 714, 114), 'B_API_FORCE_CREATE'),
    (2221, 0, (715, 52, 715, 99), 'B_API_FORCE'),
    (2221, 0, (716, 55, 716, 76), 'B_API_GET + B_API_DELETE + B_API_UPDATE + B_API_ASSERT'),
    (2221, 0, (717, 66, 717, 115), 'B_API_GET'),
    (2221, 1, (717, 85, 717, 115), 'get_iter'),
    (2221, 2, (390, 24, 390, 49), 'get_iter'),
    (2221, 3, (390, 24, 390, 34), 'get_iter'),
    (2221, 3, (390, 39, 390, 49), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 2, (717, 97, 717, 97), 'get_iter'),
    (2221, 2, (717, 100, 717, 114), 'get_iter'),
    (2221, 1, (717, 75, 717, 82), 'B_API_GET'),
    (2221, 0, (718, 74, 720, 121), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 1, (718, 86, 720, 121), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 2, (718, 87, 718, 94), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 2, (718, 103, 719, 145), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 2, (718, 114, 719, 145), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 3, (719, 115, 719, 145), 'get_iter_found'),
    (2221, 4, (390, 24, 390, 49), 'get_iter_found'),
    (2221, 5, (390, 24, 390, 34), 'get_iter_found'),
    (2221, 5, (390, 39, 390, 49), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 4, (719, 127, 719, 127), 'get_iter_found'),
    (2221, 4, (719, 130, 719, 144), 'get_iter_found'),
    (2221, 3, (718, 127, 718, 134), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 2, (720, 103, 720, 120), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 0, (721, 74, 726, 102), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2775, 1, (721, 94, 726, 102), 'B_API_GET - B_API_GET_NOTFOUND', None),
    (2221, 2, (722, 86, 725, 90), 'get_setsz'),
    (2221, 3, (722, 89, 722, 120), 'get_setsz'),
    (2221, 4, (390, 24, 390, 49), 'get_setsz'),
    (2221, 5, (390, 24, 390, 34), 'get_setsz'),
    (2221, 5, (390, 39, 390, 49), 'get_same'),
    (2221, 4, (722, 101, 722, 101), 'get_setsz'),
    (2221, 4, (722, 104, 722, 119), 'get_setsz + get_same'),
    (2221, 3, (723, 90, 723, 99), 'get_same'),
    (2221, 3, (725, 90, 725, 90), 'get_setsz - get_same'),
    (2221, 2, (726, 94, 726, 101), 'B_API_GET - B_API_GET_NOTFOUND'),
    (2221, 0, (727, 74, 727, 124), 'B_API_GET_NOTFOUND'),
    (2221, 0, (728, 74, 728, 91), 'B_API_GET_NOTFOUND'),
    (2221, 0, (729, 66, 729, 90), 'B_API_DELETE + B_API_UPDATE + B_API_ASSERT'),
    (2221, 0, (730, 74, 730, 135), 'B_API_DELETE'),
    (2775, 1, (730, 86, 730, 135), 'B_API_DELETE', None),
    (2221, 2, (730, 103, 730, 134), 'del_setsz'),
    (2221, 3, (730, 104, 730, 134), 'del_setsz'),
    (2221, 4, (390, 24, 390, 49), 'del_setsz'),
    (2221, 5, (390, 24, 390, 34), 'del_setsz'),
    (2221, 5, (390, 39, 390, 49), 'del_same'),
    (2221, 4, (730, 116, 730, 116), 'del_setsz'),
    (2221, 4, (730, 119, 730, 133), 'del_setsz'),
    (2221, 2, (730, 93, 730, 100), 'B_API_DELETE'),
    (2221, 0, (731, 74, 731, 121), 'B_API_DELETE'),
    (2221, 0, (732, 77, 732, 101), 'B_API_UPDATE + B_API_ASSERT'),
    (2221, 0, (733, 88, 733, 156), 'B_API_UPDATE'),
    (2221, 1, (733, 108, 733, 155), 'upd_iter'),
    (2221, 2, (733, 108, 733, 138), 'upd_iter'),
    (2221, 3, (390, 24, 390, 49), 'upd_iter'),
    (2221, 4, (390, 24, 390, 34), 'upd_iter'),
    (2221, 4, (390, 39, 390, 49), 'upd_nmatch'),
    (2221, 3, (733, 120, 733, 120), 'upd_iter'),
    (2221, 3, (733, 123, 733, 137), 'upd_iter'),
    (2221, 2, (733, 143, 733, 155), 'upd_nmatch'),
    (2221, 1, (733, 97, 733, 104), 'B_API_UPDATE'),
    (2221, 0, (734, 96, 736, 131), 'B_API_UPDATE_OK'),
    (2221, 1, (734, 108, 736, 131), 'B_API_UPDATE_OK'),
    (2221, 2, (734, 108, 734, 157), 'B_API_UPDATE_OK'),
    (2221, 3, (734, 125, 734, 156), 'upd_setsz'),
    (2221, 4, (734, 126, 734, 156), 'upd_setsz'),
    (2221, 5, (390, 24, 390, 49), 'upd_setsz'),
    (2221, 6, (390, 24, 390, 34), 'upd_setsz'),
    (2221, 6, (390, 39, 390, 49), 'upd_same'),
    (2221, 5, (734, 138, 734, 138), 'upd_setsz'),
    (2221, 5, (734, 141, 734, 155), 'upd_setsz'),
    (2221, 3, (734, 115, 734, 122), 'B_API_UPDATE_OK'),
    (2775, 2, (736, 108, 736, 131), 'B_API_UPDATE_OK', '2*B_API_UPDATE_OK'),
    (2221, 0, (737, 96, 737, 143), 'B_API_UPDATE_OK'),
    (2221, 0, (738, 96, 738, 146), 'B_API_UPDATE_ERR'),
    (2221, 0, (739, 96, 739, 113), 'B_API_UPDATE_ERR'),
    (2221, 0, (742, 85, 743, 108), 'B_API_ASSERT'),
    (2221, 0, (699, 37, 699, 50), 'NS*states'),
    (2775, 1, (441, 19, 441, 73), 'NS*states', 'NS*states + B_API_CREATE + B_API_FORCE + B_API_GET + B_API_DELETE + B_API_UPDATE + B_API_ASSERT'),
    (2221, 2, (441, 43, 441, 72), 'NS*cov_req'),
    (2221, 2, (441, 26, 441, 40), 'NS*states'),
    (2221, 0, (744, 28, 744, 49), 'B_API_CREATE + B_API_FORCE + B_API_GET + B_API_DELETE + B_API_UPDATE + B_API_ASSERT'),
    (2221, 0, (746, 33, 747, 88), 'B_API_LIST'),
    (2221, 1, (746, 49, 747, 88), 'B_API_LIST'),
    (2221, 2, (746, 50, 746, 61), 'B_API_LIST'),
    (2221, 2, (746, 70, 746, 125), 'B_API_LIST'),
    (2775, 2, (746, 82, 746, 125), 'B_API_LIST', None),
    (2221, 3, (746, 99, 746, 124), 'list_setsz'),
    (2221, 3, (746, 89, 746, 96), 'B_API_LIST'),
    (2221, 2, (747, 70, 747, 87), 'B_API_LIST'),
    (2221, 0, (748, 33, 753, 61), 'B_API_LIST'),
    (2775, 1, (748, 53, 753, 61), 'B_API_LIST', None),
    (2221, 2, (749, 45, 752, 49), 'list_setsz'),
    (2221, 3, (749, 48, 749, 74), 'list_setsz'),
    (2221, 3, (750, 49, 750, 58), 'list_match'),
    (2221, 3, (752, 49, 752, 49), 'list_setsz - list_match'),
    (2221, 2, (753, 53, 753, 60), 'B_API_LIST'),
    (2221, 0, (745, 37, 745, 54), 'NS*states'),
    (2775, 1, (442, 23, 442, 85), 'NS*states', 'NS*states + B_API_LIST'),
    (2221, 2, (442, 51, 442, 84), 'NS*cov_lreq'),
    (2221, 2, (442, 30, 442, 48), 'NS*states'),
    (2221, 0, (754, 28, 754, 45), 'B_API_LIST'),
    (2221, 0, (755, 22, 755, 59), 'gen_APIStart'),
    (2221, 0, (756, 22, 756, 74), 'gen_APIStart'),
    (2774, 0, (776, 1, 776, 6), 'TypeOK'),
    (2221, 0, (778, 5, 781, 72), 'states'),
    (2221, 1, (778, 8, 778, 45), 'states'),
    (2221, 2, (778, 27, 778, 45), 'cov_api'),
    (2221, 2, (778, 17, 778, 24), 'states'),
    (2221, 1, (780, 8, 780, 60), 'states'),
    (2221, 2, (780, 34, 780, 60), 'cov_req'),
    (2221, 2, (780, 17, 780, 31), 'states'),
    (2221, 1, (781, 8, 781, 72), 'states'),
    (2221, 2, (781, 38, 781, 72), 'cov_lreq'),
    (2221, 3, (433, 5, 436, 29), 'cov_lreq'),
    (2221, 4, (433, 8, 433, 44), 'cov_lreq'),
    (2221, 4, (434, 8, 435, 39), 'cov_lreq'),
    (2221, 5, (434, 25, 435, 39), 'cov_objs'),
    (2221, 5, (434, 17, 434, 22), 'cov_lreq'),
    (2221, 4, (436, 8, 436, 29), 'cov_lreq'),
    (2221, 3, (781, 57, 781, 71), 'cov_lreq'),
    (2221, 2, (781, 17, 781, 35), 'states'),
    (2774, 0, (787, 1, 787, 14), 'OnlyOneVersion'),
    (2221, 0, (788, 5, 789, 51), 'states'),
    (2221, 1, (788, 29, 789, 51), 'cov_api2'),
    (2221, 2, (788, 32, 788, 38), 'cov_api2'),
    (2221, 2, (789, 32, 789, 51), 'cov_api2 - cov_api'),
    (2221, 1, (788, 19, 788, 26), 'states'),
)
# MC.out lines of the 2775 messages whose cost figure is not derived: the
# count is printed alone
COVERAGE_COST_UNKNOWN = (675, 783, 828, 966, 981)


def coverage_values(r, cov: Dict[str, int], procs=(1, 1, 1)) -> List[tuple]:
    """COVERAGE_LINES evaluated for one run: (code, depth, span, name, count,
    cost) per row; count / cost None where the message has none."""
    nc, np_, ns = procs
    env = dict(cov)
    env.update({"gen_" + a: v for a, v in r.act_gen.items()})
    env.update(init=r.init, P=nc + np_ + ns, NC=nc, NP=np_, NS=ns)
    out = []
    for row in COVERAGE_LINES:
        code, depth, span, formula = row[:4]
        if code == 2773:
            out.append((code, 0, span, formula, r.init, r.init))
        elif code == 2772:
            out.append((code, 0, span, formula, r.act_gen[formula], r.act_dist[formula]))
        elif code == 2774:
            out.append((code, 0, span, formula, None, None))
        else:
            cost = row[4] if code == 2775 else None
            out.append((code, depth, span, None, eval(formula, {"__builtins__": {}}, env),
                        None if cost is None else eval(cost, {"__builtins__": {}}, env)))
    return out


def coverage_messages(r, cov: Dict[str, int], procs=(1, 1, 1)) -> List[tuple]:
    """The coverage block between 2201 and 2202 with expression-level
    coverage: (code, body) in MC.out's order."""
    out = []
    for code, depth, span, name, count, cost in coverage_values(r, cov, procs):
        l1, c1, l2, c2 = span
        if code in (2773, 2772):
            out.append((code, f"{span_text(name, span)}: {cost}:{count}"))
        elif code == 2774:
            out.append((code, span_text(name, span)))
        else:
            body = f"  {'|' * depth}line {l1}, col {c1} to line {l2}, col {c2} of module KubeAPI: {count}"
            out.append((code, body if cost is None else f"{body}:{cost}"))
    return out


def span_text(name: str, span) -> str:
    l1, c1, l2, c2 = span
    return f"<{name} line {l1}, col {c1} to line {l2}, col {c2} of module KubeAPI>"


def outdegree_stats(hist) -> Optional[tuple]:
    """(average, minimum, maximum, 95th percentile) of TLC's outdegree (new
    states first reached from an expanded state) from a 16-bin histogram
    (the last bin holds 15 or more)."""
    total = sum(hist)
    if not total:
        return None
    avg = sum(k * v for k, v in enumerate(hist)) / total
    lo = min(k for k, v in enumerate(hist) if v)
    hi = max(k for k, v in enumerate(hist) if v)
    acc, p95 = 0, hi
    for k, v in enumerate(hist):
        acc += v
        if acc >= 0.95 * total:
            p95 = k
            break
    return round(avg), lo, hi, p95


def java_e(x: float) -> str:
    """TLC's rendering of a probability: one decimal, exponent without
    padding (MC.out:41-42 "3.7E-9", "9.9E-10")."""
    m, e = f"{x:.1E}".split("E")
    return f"{m}E{int(e)}"


def tstamp(t: float) -> str:
    return time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(t))


def messages(r, t_start: float, t_end: float, actual_fp_prob: Optional[float] = None,
             engine: str = "", ngpus: int = 1, symmetry: Optional[str] = None,
             coverage: Optional[Dict[str, int]] = None, procs=(1, 1, 1), recovered=None,
             checkpointed=None, constraints: Optional[List[str]] = None) -> List[tuple]:
    """TLC -tool messages (code, class, body) for one check's result, in the
    order of the reference run (MC.out:1-1108).  coverage (a
    CheckResult.coverage of a model with procs = (nc, np, ns)) adds the
    expression-level lines (2221, 2775, 2774) between the per-action ones, as
    TLC's -coverage prints them.  SANY's messages (2220/2219) are not
    produced: there is no TLA+ front end here.  recovered =
    (dir, CheckpointInfo) of a run started with -recover; checkpointed = (dir,
    CheckpointInfo, time) of the last checkpoint the run wrote."""
    out = []
    add = lambda code, text, cls=0: out.append((code, cls, text))  # noqa: E731
    add(2262, f"kubecheck (TLC-compatible counts) {engine}".rstrip())
    add(2187, f"Running breadth-first search Model-Checking with {ngpus} MI355X GPU(s) "
              f"(kubecheck ClaimSet FPSet, HBM StateQueue)."
              + (f" Symmetry set: {symmetry}." if symmetry else "")
              + (f" Constraints: {' '.join(constraints)} ({r.cut_state} generated states discarded by a state "
                 f"constraint, {r.cut_action} by an action constraint)." if constraints else ""))
    add(2185, f"Starting... ({tstamp(t_start)})")
    if recovered is not None:
        add(2197, f"Starting recovery from checkpoint {recovered[0]}/")
        add(2198, f"Recovery completed. {recovered[1].distinct} states examined. {recovered[1].n} states on queue.")
    else:
        add(2189, "Computing initial states...")
        add(2190, f"Finished computing initial states: {r.init} distinct states generated at {tstamp(t_start)}.")
    if checkpointed is not None:
        add(2195, f"Checkpointing of run {checkpointed[0]}")
        add(2196, f"Checkpointing completed at ({tstamp(checkpointed[2])})")
    d, g = r.distinct, r.generated
    minutes = max(t_end - t_start, 1e-9) / 60.0
    if r.error is None:
        body = ("Model checking completed. No error has been found.\n"
                "  Estimates of the probability that TLC did not check all reachable states\n"
                "  because two distinct states had the same fingerprint:\n"
                f"  calculated (optimistic):  val = {java_e(d * (g - d) / 2**64)}")
        if actual_fp_prob is not None:
            body += f"\n  based on the actual fingerprints:  val = {java_e(actual_fp_prob)}"
        add(2193, body)
    else:
        if r.error == "invariant":
            add(2110, f"Invariant {r.error_invariant} is violated.", 1)
        elif r.error == "assertion":
            add(2132, f"The first argument of Assert evaluated to FALSE (action {r.error_action}).", 1)
        elif r.error == "action_property":
            # (the behaviour below is the path to s, then the step's s')
            add(2112, f"Action property {r.error_property} is violated.", 1)
        else:
            add(2114, "Deadlock reached.", 1)
        add(2121, "The behavior up to this point is:", 1)
        blocks = re.split(r"^State (\d+):$", r.trace_text, flags=re.M)[1:]
        for num, body in zip(blocks[0::2], blocks[1::2]):
            add(2217, f"{num}: {body.strip()}", 4)
    add(2201, f"The coverage statistics at {tstamp(t_end)}")
    if coverage is not None:
        for code, body in coverage_messages(r, coverage, procs):
            add(code, body)
    else:
        add(2773, f"{span_text('Init', INIT_SPAN)}: {r.init}:{r.init}")
        for name, span in ACTION_SPANS.items():
            add(2772, f"{span_text(name, span)}: {r.act_dist[name]}:{r.act_gen[name]}")
    add(2202, "End of statistics.")
    add(2200, f"Progress({r.depth}) at {tstamp(t_end)}: {g:,} states generated ({int(g / minutes):,} s/min), "
              f"{d:,} distinct states found ({int(d / minutes):,} ds/min), {r.queue_left:,} states left on queue.")
    add(2199, f"{g} states generated, {d} distinct states found, {r.queue_left} states left on queue.")
    add(2194, f"The depth of the complete state graph search is {r.depth}.")
    st = outdegree_stats(getattr(r, "outdeg_hist", []) or [])
    if st:
        add(2268, f"The average outdegree of the complete state graph is {st[0]} (minimum is {st[1]}, "
                  f"the maximum {st[2]} and the 95th percentile is {st[3]}).")
    add(2186, f"Finished in {int(round((t_end - t_start) * 1000))}ms at ({tstamp(t_end)})")
    return out


SIM_DEFAULT_WALKS = 65536   # TLC's -simulate runs until stopped; kubecheck needs a bound
SIM_DEFAULT_DEPTH = 100     # TLC's -depth default


def sim_messages(r, num_init: int, seed: int, num_walks: int, depth: int, t_start: float, t_end: float,
                 engine: str = "") -> List[tuple]:
    """-tool messages (code, class, body) for one simulation run.  The
    violation reports (2110/2132/2114, 2121, 2217) and the coverage block
    (2201/2773/2772/2202, the steps per action in the place of both counts)
    have the bodies the BFS prints.  The simulate-specific lines (the 2187
    start banner, the 2210 totals line: their codes and their wording) are
    kubecheck's own: the reference holds no simulation output, so nothing here
    claims to match what TLC prints in this mode."""
    out = []
    add = lambda code, text, cls=0: out.append((code, cls, text))  # noqa: E731
    add(2262, f"kubecheck (simulation mode) {engine}".rstrip())
    add(2187, f"Running Random Simulation with seed {seed}: {num_walks} behaviors of at most {depth} states "
              f"on 1 MI355X GPU.")
    add(2185, f"Starting... ({tstamp(t_start)})")
    if r.error is not None:
        if r.error == "invariant":
            add(2110, f"Invariant {r.error_invariant} is violated.", 1)
        elif r.error == "assertion":
            add(2132, f"The first argument of Assert evaluated to FALSE (action {r.error_action}).", 1)
        else:
            add(2114, "Deadlock reached.", 1)
        add(2121, "The behavior up to this point is:", 1)
        blocks = re.split(r"^State (\d+):$", r.trace_text, flags=re.M)[1:]
        for num, body in zip(blocks[0::2], blocks[1::2]):
            add(2217, f"{num}: {body.strip()}", 4)
    add(2201, f"The coverage statistics at {tstamp(t_end)}")
    add(2773, f"{span_text('Init', INIT_SPAN)}: {num_init}:{num_init}")
    for name, span in ACTION_SPANS.items():
        add(2772, f"{span_text(name, span)}: {r.act_steps[name]}:{r.act_steps[name]}")
    add(2202, "End of statistics.")
    line = (f"{r.steps} steps taken in {num_walks} behaviors (walk {r.error_walk} is the one reported): "
            if r.error is not None else f"{r.steps} steps taken in {num_walks} behaviors: ")
    line += (f"{r.walks_error} ended in an error, {r.walks_depth} at the depth limit, "
             f"{r.walks_terminated} terminated")
    if r.fpset_slots:
        line += f"; {r.distinct_visited} distinct states visited"
    add(2210, line + ".")
    add(2186, f"Finished in {int(round((t_end - t_start) * 1000))}ms at ({tstamp(t_end)})")
    return out


FAIRNESS_TEXT = {"next": "WF_vars(Next)", "process": "weak fairness of every process"}


def live_start_message(name: str, fairness: str, distinct: int, t: float) -> str:
    """The body of the 2192 line that opens a property's check."""
    return (f"Checking temporal property {name} under {FAIRNESS_TEXT[fairness]} for the complete state space "
            f"with {distinct} total distinct states at ({tstamp(t)})")


def live_messages(r) -> List[tuple]:
    """-tool messages (code, class, body) for a violated temporal property (a
    kubecheck.LiveResult): 2116, 2264, the 2217 states of the counterexample,
    then 2122 "Back to state N" or 2218 "Stuttering".  The reference holds no
    liveness output, so these codes and their wording claim no match with
    TLC's."""
    out = []
    add = lambda code, text, cls=0: out.append((code, cls, text))  # noqa: E731
    add(2116, "Temporal properties were violated.", 1)
    add(2264, "The following behavior constitutes a counter-example:", 1)
    blocks = re.split(r"^State (\d+):$", r.trace_text, flags=re.M)[1:]
    for num, body in zip(blocks[0::2], blocks[1::2]):
        add(2217, f"{num}: {body.strip()}", 4)
    if r.kind == "back-to-state":
        add(2122, f"{r.trace_len + 1}: Back to state {r.loop_start + 1}", 4)
    else:
        add(2218, f"{r.trace_len + 1}: Stuttering", 4)
    return out


def split_simulate(argv: List[str]):
    """Take TLC's `-simulate [num=N]` out of argv: (rest, simulate?, N or None).
    The optional argument is TLC's comma-separated list; only num= is known."""
    rest, sim, num = [], False, None
    i = 0
    while i < len(argv):
        if argv[i] != "-simulate":
            rest.append(argv[i])
            i += 1
            continue
        sim = True
        i += 1
        if i < len(argv) and "=" in argv[i] and not argv[i].startswith("-"):
            for item in argv[i].split(","):
                m = re.fullmatch(r"num=(\d+)", item)
                if not m or int(m.group(1)) < 1:
                    raise CfgError(f"-simulate {argv[i]}: expected num=N with N >= 1")
                num = int(m.group(1))
            i += 1
    return rest, sim, num


def split_coverage(argv: List[str]):
    """Take TLC's `-coverage [minutes]` out of argv: (rest, coverage?).  TLC's
    argument is the interval of its periodic reports, which are not printed
    here: an integer after the flag is accepted and ignored."""
    rest, cov = [], False
    i = 0
    while i < len(argv):
        if argv[i] != "-coverage":
            rest.append(argv[i])
            i += 1
            continue
        cov = True
        i += 1
        if i < len(argv) and argv[i].isdigit():
            i += 1
    return rest, cov


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    argv = list(sys.argv[1:] if argv is None else argv)
    argv, simulate, num = split_simulate(argv)
    argv, coverage = split_coverage(argv)
    ap = argparse.ArgumentParser(prog="kubecheck.tlc", description=__doc__.split("\n\n")[0])
    ap.add_argument("-depth", type=int, default=SIM_DEFAULT_DEPTH,
                    help="-simulate: the most states in a behaviour (TLC's default 100)")
    ap.add_argument("-seed", type=int, default=None, help="-simulate: RNG seed (default: from the clock)")
    ap.add_argument("-continue", dest="cont", action="store_true",
                    help="-simulate: run every behaviour to its end after an error")
    ap.add_argument("spec", nargs="?", default="MC")
    ap.add_argument("-config", default=None)
    ap.add_argument("-defs", default=None, metavar="FILE",
                    help="`Name == expr` definitions of user invariants the cfg's INVARIANT list may name")
    ap.add_argument("-deadlock", action="store_true", help="do NOT check for deadlock (TLC flag)")
    ap.add_argument("-tool", action="store_true")
    ap.add_argument("-workers", default="1")
    ap.add_argument("-fp", type=int, default=None)
    ap.add_argument("-nc", type=int, default=1)
    ap.add_argument("-np", type=int, default=1)
    ap.add_argument("-ns", type=int, default=1)
    ap.add_argument("-variant", type=int, default=0)
    ap.add_argument("-device", type=int, default=0)
    ap.add_argument("-nocheckfps", action="store_true",
                    help="skip the 'based on the actual fingerprints' estimate (a sort of the seen-set)")
    ap.add_argument("-fairness", choices=("next", "process"), default=None,
                    help="temporal properties: WF_vars(Next) (the default) or weak fairness of every process")
    ap.add_argument("-checkpoint", type=float, default=0.0, metavar="MINUTES",
                    help="checkpoint whenever this many minutes have passed (TLC flag; 0 = none)")
    ap.add_argument("-checkpointlevels", type=int, default=0, metavar="N", help="checkpoint every N BFS levels")
    ap.add_argument("-metadir", default=None, help="where the checkpoint goes (TLC flag)")
    ap.add_argument("-recover", default=None, metavar="DIR", help="start from DIR's checkpoint (TLC flag)")
    a = ap.parse_args(argv)
    a.simulate, a.num = simulate, (num if num is not None else SIM_DEFAULT_WALKS)
    a.coverage = coverage
    if a.checkpoint < 0 or a.checkpointlevels < 0:
        raise CfgError("-checkpoint / -checkpointlevels: expected a number >= 0")
    a.checkpointing = bool(a.checkpoint > 0 or a.checkpointlevels > 0 or a.recover)
    if a.checkpointing and simulate:
        raise CfgError("-checkpoint / -recover with -simulate: a random walk has nothing to take up again")
    if a.checkpointing and coverage:
        raise CfgError("-checkpoint / -recover with -coverage: a checkpoint holds no coverage sums")
    if simulate and coverage:
        raise CfgError("-coverage with -simulate: expression-level coverage is counted by the BFS only")
    if simulate and a.fairness is not None:
        raise CfgError("-fairness goes with a PROPERTY list; -simulate checks no temporal property")
    a.fairness = a.fairness or "next"
    if simulate and not 1 <= a.depth <= 65535:
        raise CfgError(f"-depth {a.depth}: expected 1..65535")
    return a


def main(argv: Optional[List[str]] = None) -> int:
    try:
        a = parse_args(argv)
    except CfgError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1

    cfg_path = a.config or f"{a.spec}.cfg"
    if not os.path.exists(cfg_path):
        print(f"Error: cannot read model config {cfg_path}", file=sys.stderr)
        return 1
    tla_path = os.path.join(os.path.dirname(os.path.abspath(cfg_path)), f"{a.spec}.tla")
    defs = parse_defs(open(tla_path).read()) if os.path.exists(tla_path) else {}
    parsed = parse_cfg(open(cfg_path).read(), defs)
    user_inv = {}
    user_props: Dict[str, str] = {}
    if a.defs:
        from . import pred
        if not os.path.exists(a.defs):
            print(f"Error: cannot read the definitions {a.defs}", file=sys.stderr)
            return 1
        try:
            user_defs = pred.parse_definitions(open(a.defs).read())
        except pred.PredError as e:
            raise CfgError(f"-defs {a.defs}: {e}") from None
        parsed, user_inv = split_user_invariants(parsed, user_defs, (a.nc, a.np, a.ns), a.simulate, a.coverage,
                                                 a.checkpointing)
        user_props = split_user_properties(parsed, user_defs, (a.nc, a.np, a.ns))
    try:
        kw, props = check_from_cfg(parsed, a.simulate, a.coverage, a.checkpointing, user_props)
    except CfgError as e:
        # (a refused combination with the checkpoint flags or with a cfg's
        # constraints ends in an Error line; the older refusals raise, as they did)
        if not (a.checkpointing or parsed["constraints"] or parsed["action_constraints"] or
                any(x in ACTION_PROPERTY_NAMES for x in parsed["properties"])):
            raise
        print(f"Error: {e}", file=sys.stderr)
        return 1

    import kubecheck

    mc_cfg = kubecheck.ModelConfig(nc=a.nc, np=a.np, ns=a.ns, variant=a.variant, device=a.device,
                                   check_deadlock=not a.deadlock, **kw)
    t0 = time.time()
    if a.simulate:
        seed = a.seed if a.seed is not None else time.time_ns()
        with kubecheck.Simulator(mc_cfg, seed=seed, num_walks=a.num, depth=a.depth, count_distinct=True,
                                 stop_on_error=not a.cont) as sim:
            r = sim.run()
            seed = sim.seed
        num_init = len(kubecheck.Spec(mc_cfg).init())
        for code, cls, body in sim_messages(r, num_init, seed, a.num, a.depth, t0, t0 + r.seconds,
                                            kubecheck.load().kc_build_info().decode()):
            print(msg(code, body, cls, a.tool), flush=True)
        return 0 if r.error is None else 12
    recovered = checkpointed = None
    metadir = a.metadir or a.recover or os.path.join(os.path.dirname(os.path.abspath(cfg_path)), "states")
    with kubecheck.ModelChecker(mc_cfg, coverage=a.coverage) as mc:
        try:
            if user_inv:
                mc.set_invariants(user_inv)
            if a.recover:
                mc.recover(a.recover)
                recovered = (a.recover.rstrip("/"), kubecheck.checkpoint_info(a.recover))
            if a.checkpoint > 0 or a.checkpointlevels > 0:
                os.makedirs(metadir, exist_ok=True)
                mc.set_checkpoint(metadir, every_levels=a.checkpointlevels, every_seconds=a.checkpoint * 60.0)
        except kubecheck.KubecheckError as e:
            print(f"Error: {e}", file=sys.stderr)
            return 1
        r = mc.run()
        prob = None if (a.nocheckfps or r.error is not None) else mc.check_fps()[1]
    t1 = t0 + r.seconds
    # the last checkpoint this run wrote, if any
    ck_file = os.path.join(metadir, "checkpoint.kc")
    if (a.checkpoint > 0 or a.checkpointlevels > 0) and os.path.exists(ck_file) and os.path.getmtime(ck_file) >= t0 - 1:
        info = kubecheck.checkpoint_info(metadir)
        if recovered is None or info.level > recovered[1].level:
            checkpointed = (metadir.rstrip("/"), info, os.path.getmtime(ck_file))
    out = messages(r, t0, t1, prob, kubecheck.load().kc_build_info().decode(), kubecheck.device_count(),
                   parsed["symmetry"], coverage=r.coverage if a.coverage else None, procs=(a.nc, a.np, a.ns),
                   recovered=recovered, checkpointed=checkpointed,
                   constraints=(parsed["constraints"] + parsed["action_constraints"]) or None)
    if not props or r.error is not None:
        for code, cls, body in out:
            print(msg(code, body, cls, a.tool), flush=True)
        return 0 if r.error is None else 12
    # temporal properties, in cfg order, between the BFS block and its 2186 line
    for code, cls, body in out[:-1]:
        print(msg(code, body, cls, a.tool), flush=True)
    rc = 0
    for name in props:
        print(msg(2192, live_start_message(name, a.fairness, r.distinct, time.time()), 0, a.tool), flush=True)
        # (the liveness phase has no part in the action properties: the BFS checked them)
        which = dict(formula=user_props[name], name=name) if name in user_props else dict(property=name)
        with kubecheck.LivenessChecker(dataclasses.replace(mc_cfg, action_properties=0), fairness=a.fairness,
                                       **which) as lc:
            lr = lc.run()
        t1 += lr.seconds
        if lr.error is not None or (lr.states, lr.edges) != (r.distinct, r.generated - r.init):
            print(f"Error: the liveness graph ({lr.states} states, {lr.edges} edges, error {lr.error}) is not "
                  f"the BFS's ({r.distinct}, {r.generated - r.init})", file=sys.stderr)
            return 1
        if lr.violated:
            for code, cls, body in live_messages(lr):
                print(msg(code, body, cls, a.tool), flush=True)
            rc = 13
            break
    print(msg(2186, f"Finished in {int(round((t1 - t0) * 1000))}ms at ({tstamp(t1)})", 0, a.tool), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
