"""TLC-style command line for the KubeAPI model checker.

    python -m kubecheck.tlc [-config MC.cfg] [-deadlock] [-tool] [-nc N -np N -ns N]
                            [-variant V] [-workers N] [-fp K]
                            [-simulate [num=N]] [-depth D] [-seed S] [-continue]
                            [-fairness next|process] [MC]

Reads the same inputs as the reference's toolbox run: a TLC model config
(KubeAPI.toolbox/Model_1/MC.cfg:1-16 — CONSTANT assignments, either direct
`X = TRUE` or TLC's `X <- def` indirection resolved through MC.tla:5-12;
SPECIFICATION; INVARIANT) and prints TLC's `-tool` message stream
(@!@!@STARTMSG code:class ... @!@!@ENDMSG code) for the messages the
reference run shows (MC.out: 2262, 2187, 2185, 2189/2190, 2193 with both
collision estimates, 2201/2773/2772/2202 coverage with TLC's source spans,
2200 progress, 2199, 2194, 2268 outdegree, 2186) plus violation reports.
SANY's messages (2220/2219) and expression-level coverage (2221) are not
produced (no TLA+ front end).  The model check itself
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

`-fairness process` checks the properties under weak
fairness of every process (PlusCal's `fair process`; a .cfg cannot say this,
so it is an option) instead of WF_vars(Next), the default; the 2192 line names
the fairness assumed.  It is refused together with -simulate.
"""
from __future__ import annotations

import argparse
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
                 "symmetry": None}
    i, section = 0, None
    keywords = {"CONSTANT", "CONSTANTS", "SPECIFICATION", "INVARIANT", "INVARIANTS",
                "PROPERTY", "PROPERTIES", "INIT", "NEXT", "SYMMETRY"}
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
    return kw


def check_from_cfg(cfg: dict, simulate: bool = False):
    """model_from_cfg for a cfg that may list temporal properties: (ModelConfig
    kwargs, the PROPERTY names in cfg order).  The names must be kubecheck's
    PROPERTIES; simulation mode checks none."""
    from ._lib import PROPERTIES

    props = list(cfg["properties"])
    bad = [x for x in props if x not in PROPERTIES]
    if bad:
        raise CfgError(f"unknown temporal property(ies) {bad}; known: {PROPERTIES}")
    if props and simulate:
        raise CfgError("-simulate checks no temporal PROPERTY (liveness needs the whole state graph)")
    if cfg.get("symmetry") and props:
        raise CfgError(f"SYMMETRY {cfg['symmetry']} with a PROPERTY list: liveness checking under symmetry "
                       "reduction is unsound")
    if cfg.get("symmetry") and simulate:
        raise CfgError(f"SYMMETRY {cfg['symmetry']} with -simulate: a random walk has no seen-set to reduce")
    return model_from_cfg(dict(cfg, properties=[])), props


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
             engine: str = "", ngpus: int = 1, symmetry: Optional[str] = None) -> List[tuple]:
    """TLC -tool messages (code, class, body) for one check's result, in the
    order of the reference run (MC.out:1-1108).  SANY's (2220/2219) and the
    expression-level coverage (2221) are not produced: there is no TLA+ front
    end here."""
    out = []
    add = lambda code, text, cls=0: out.append((code, cls, text))  # noqa: E731
    add(2262, f"kubecheck (TLC-compatible counts) {engine}".rstrip())
    add(2187, f"Running breadth-first search Model-Checking with {ngpus} MI355X GPU(s) "
              f"(kubecheck ClaimSet FPSet, HBM StateQueue)."
              + (f" Symmetry set: {symmetry}." if symmetry else ""))
    add(2185, f"Starting... ({tstamp(t_start)})")
    add(2189, "Computing initial states...")
    add(2190, f"Finished computing initial states: {r.init} distinct states generated at {tstamp(t_start)}.")
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
        else:
            add(2114, "Deadlock reached.", 1)
        add(2121, "The behavior up to this point is:", 1)
        blocks = re.split(r"^State (\d+):$", r.trace_text, flags=re.M)[1:]
        for num, body in zip(blocks[0::2], blocks[1::2]):
            add(2217, f"{num}: {body.strip()}", 4)
    add(2201, f"The coverage statistics at {tstamp(t_end)}")
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


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    argv = list(sys.argv[1:] if argv is None else argv)
    argv, simulate, num = split_simulate(argv)
    ap = argparse.ArgumentParser(prog="kubecheck.tlc", description=__doc__.split("\n\n")[0])
    ap.add_argument("-depth", type=int, default=SIM_DEFAULT_DEPTH,
                    help="-simulate: the most states in a behaviour (TLC's default 100)")
    ap.add_argument("-seed", type=int, default=None, help="-simulate: RNG seed (default: from the clock)")
    ap.add_argument("-continue", dest="cont", action="store_true",
                    help="-simulate: run every behaviour to its end after an error")
    ap.add_argument("spec", nargs="?", default="MC")
    ap.add_argument("-config", default=None)
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
    a = ap.parse_args(argv)
    a.simulate, a.num = simulate, (num if num is not None else SIM_DEFAULT_WALKS)
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
    kw, props = check_from_cfg(parsed, a.simulate)

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
    with kubecheck.ModelChecker(mc_cfg) as mc:
        r = mc.run()
        prob = None if (a.nocheckfps or r.error is not None) else mc.check_fps()[1]
    t1 = t0 + r.seconds
    out = messages(r, t0, t1, prob, kubecheck.load().kc_build_info().decode(), kubecheck.device_count(),
                   parsed["symmetry"])
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
        with kubecheck.LivenessChecker(mc_cfg, name, fairness=a.fairness) as lc:
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
