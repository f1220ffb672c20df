"""kubecheck — MI355X-native BFS model checker for KubeAPI.tla.

Host-side mirror of the reference's checking surface (TLC 2.16 as run on
KubeAPI.toolbox/Model_1, MC.out:2-5):

* :class:`FPSet`        — tlc2.tool.fp.FPSet (put / contains / size / checkFPs),
                          backed by the HBM open-addressing set.
* :class:`StateQueue`   — tlc2.tool.queue.StateQueue over packed states in HBM.
* :class:`ModelChecker` — tlc2.TLC's BFS safety check of Spec with the Model_1
                          inputs (MC.cfg / MC.tla), reporting the same counts
                          (MC.out:1098), depth (:1101), per-action coverage
                          (:78-621) and counterexample traces.
* :class:`Simulator`    — tlc2.TLC -simulate: seeded random behaviours on the GPU,
                          each state checked like the BFS's; the reported walk
                          is replayed on the host (:meth:`Spec.sim_replay`).
* :class:`LivenessChecker` — tlc2.TLC's liveness check of the spec's temporal
                          properties under WF_vars(Next) or per-process weak
                          fairness (fair SCCs): the reachable graph, the
                          elimination and a lasso counterexample on the GPU.
* :mod:`kubecheck.tlc`  — TLC-style command line (``-config MC.cfg MC``) with
                          ``-tool`` message output.

All compute runs in libkubecheck.so (HIP, gfx950).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from ._lib import (ACTION_CONSTRAINTS, ACTION_PROPERTIES, ACTIONS, CKPT_SECTIONS, CUTS, ERR_KINDS, FAIRNESS, INSTANTIATIONS, INVARIANTS,
                   LIVE_FORMS, LIVE_KINDS, LIVE_USER, PROPERTIES, SIM_KINDS,
                   KcCheckpointInfo, KcCheckpointOptions, KcLiveConfig,
                   KcLiveResult, KcModelConfig, KcResult, KcSimConfig,
                   KcSimResult, KcSqueueConfig, KcSqueueStats, KubecheckError,
                   check, load)
from . import pred

__all__ = ["ModelConfig", "ModelChecker", "CheckResult", "FPSet", "StateQueue", "Spec",
           "Simulator", "SimResult", "SIM_KINDS", "LivenessChecker", "LiveResult", "PROPERTIES", "FAIRNESS",
           "KubecheckError", "ACTIONS", "load", "device_count", "stress_fps_dev", "stress_fp",
           "CheckpointInfo", "checkpoint_info", "ACTION_PROPERTIES", "pred", "UserInvariant"]


def device_count() -> int:
    return load().kc_device_count()


# ModelConfig.symmetry by name -> kc_model_config.symmetry
SYMMETRY_SETS = {"clients": 1, "controllers": 2, "actors": 3}


@dataclass
class ModelConfig:
    """A KubeAPI model: Model_1 is nc=np=ns=1 with both constants TRUE."""
    nc: int = 1                 # clients            (KubeAPI.tla:161)
    np: int = 1                 # PVC controllers    (KubeAPI.tla:225)
    ns: int = 1                 # API servers        (KubeAPI.tla:268)
    can_fail: bool = True       # REQUESTS_CAN_FAIL    (MC.tla:5-7)
    can_timeout: bool = True    # REQUESTS_CAN_TIMEOUT (MC.tla:10-12)
    check_deadlock: bool = True # KubeAPI___Model_1.launch:16
    variant: int = 0            # seeded bugs 1-5 (include/kubecheck.h); 0 = KubeAPI.tla as written
    device: int = 0
    keep_trace: bool = True
    max_levels: int = 0
    fpset_slots: int = 0
    chunk_states: int = 0
    verbose: int = 0
    timing: int = 0             # HIP-event timing (kernel_times()): 1 every kernel, 2 k_claim only
    invariants: int = 3         # MC.cfg INVARIANT: bit 0 TypeOK, bit 1 OnlyOneVersion (0 = none)
    # frontier spill (TLC's DiskStateQueue role): > 0 keeps the frontiers in a
    # StateQueue with this HBM budget; past it segments go to pinned host RAM
    # (frontier_host_bytes, 0 = unlimited), then to files in spill_dir
    frontier_hbm_bytes: int = 0
    frontier_host_bytes: int = 0
    frontier_segment_states: int = 0   # parents per chunk / states per segment (0 = 2^22)
    spill_dir: Optional[str] = None
    trace_host: bool = False    # the trace file (9 B per state) in pinned host RAM
    # seen-set spill (TLC's OffHeapDiskFPSet role): > 0 caps the seen-set's HBM;
    # older fingerprints go to sorted runs in pinned host RAM (seen_host_bytes,
    # 0 = unlimited), then to files in spill_dir
    seen_hbm_bytes: int = 0
    seen_host_bytes: int = 0
    # sharded runs at R > 1: claims in sequential-BFS order, so errors and
    # traces equal TLC -workers 1's (a per-level all-reduce and sort)
    tlc_order: bool = False
    # the first inserter of a state owns it (TLC -workers N semantics: same
    # counts and trace lengths, no settle passes; the winning copy of a
    # same-level duplicate is not deterministic).  The engine's in-HBM wide
    # levels and every counted level of the sharded loop (not with tlc_order
    # or the seen-set spill there); CheckResult.claim_mode says what ran
    first_claim: bool = False
    # symmetry reduction (TLC's SYMMETRY): 0 (off), "clients", "controllers" or
    # "actors" (both), or the mask itself (bit 0 clients, bit 1 controllers).
    # The seen-set keeps one fingerprint per permutation orbit, so distinct,
    # level_width and act_dist count orbits; frontier states and traces stay
    # real states.  The single-GPU engine only (include/kubecheck.h).
    symmetry: Union[int, str] = 0
    # constraints (TLC's CONSTRAINT / ACTION_CONSTRAINT): a
    # successor outside them is generated, then discarded (after its invariant
    # check) without a seen-set lookup.  Build-defined vocabulary:
    # StoredAtMost<k> = constraint_stored=k (Cardinality(apiState) <= k),
    # InFlightAtMost<k> = constraint_inflight=k (pending requests + pending
    # list requests <= k); -1 = off.  action_constraints: 0, a name of
    # ACTION_CONSTRAINTS ("ServeClientsFirst"), a list of names, or the mask.
    # The single-GPU in-HBM BFS only (include/kubecheck.h).
    constraint_stored: int = -1
    constraint_inflight: int = -1
    action_constraints: Union[int, str, Sequence[str]] = 0
    # action properties (TLC's PROPERTY [][A]_vars, a step invariant;
    # DESIGN.md §4.12): checked on every step the BFS generates, into seen
    # states too.  0 / (), a name of ACTION_PROPERTIES ("NoBlindUpdate",
    # "OneReplyPerStep", "StoreNeverShrinks"), a sequence of names, or the
    # mask.  The single-GPU in-HBM BFS only (include/kubecheck.h).
    action_properties: Union[int, str, Sequence[str]] = 0

    @property
    def action_properties_mask(self) -> int:
        a = self.action_properties
        if isinstance(a, str):
            a = [a]
        if isinstance(a, (list, tuple)):
            m = 0
            for name in a:
                if name not in ACTION_PROPERTIES:
                    raise ValueError(f"action property {name!r}: expected " + ", ".join(ACTION_PROPERTIES))
                m |= ACTION_PROPERTIES[name]
            return m
        a = int(a or 0)
        if a & ~sum(ACTION_PROPERTIES.values()):
            raise ValueError(f"action_properties {a}: the mask has bits 0..2 ({', '.join(ACTION_PROPERTIES)})")
        return a

    @property
    def action_constraints_mask(self) -> int:
        a = self.action_constraints
        if isinstance(a, str):
            a = [a]
        if isinstance(a, (list, tuple)):
            m = 0
            for name in a:
                if name not in ACTION_CONSTRAINTS:
                    raise ValueError(f"action constraint {name!r}: expected " + ", ".join(ACTION_CONSTRAINTS))
                m |= ACTION_CONSTRAINTS[name]
            return m
        a = int(a or 0)
        if a & ~sum(ACTION_CONSTRAINTS.values()):
            raise ValueError(f"action_constraints {a}: the mask has bit 0 (ServeClientsFirst) only")
        return a

    @property
    def symmetry_mask(self) -> int:
        s = self.symmetry
        if isinstance(s, str):
            if s not in SYMMETRY_SETS:
                raise ValueError(f"symmetry {s!r}: expected 0, " + ", ".join(repr(k) for k in SYMMETRY_SETS))
            return SYMMETRY_SETS[s]
        s = int(s or 0)
        if s & ~3:
            raise ValueError(f"symmetry {s}: the mask is 0..3 (bit 0 clients, bit 1 controllers)")
        return s

    def to_c(self) -> KcModelConfig:
        c = KcModelConfig()
        for f in KcModelConfig._fields_:
            if f[0] == "spill_dir":
                continue
            if f[0] == "symmetry":
                c.symmetry = self.symmetry_mask
                continue
            if f[0] == "action_constraints":
                c.action_constraints = self.action_constraints_mask
                continue
            if f[0] == "action_properties":
                c.action_properties = self.action_properties_mask
                continue
            setattr(c, f[0], int(getattr(self, f[0])))
        # the C string must outlive the engine's use of the config (copied at create)
        c.spill_dir = self.spill_dir.encode() if self.spill_dir else None
        return c

    @property
    def name(self) -> str:
        return f"KubeAPI(nc={self.nc},np={self.np},ns={self.ns})"


@dataclass
class UserInvariant:
    """One user-defined invariant of a run (ModelChecker(invariants=...))."""
    name: str
    violations: int          # states violating it in the level that ended the run (0 when it holds)
    states_evaluated: int    # states the run expanded, each evaluated once


@dataclass
class CheckResult:
    init: int
    generated: int
    distinct: int
    queue_left: int
    depth: int
    complete: bool
    act_gen: Dict[str, int]
    act_dist: Dict[str, int]
    level_width: List[int]
    error: Optional[str]              # None, "assertion", "invariant", "deadlock"
    error_action: Optional[str]
    error_self: int
    error_invariant: Optional[str]
    error_level: int
    trace_len: int
    seconds: float
    collision_optimistic: float
    fpset_slots: int
    peak_frontier: int
    fpset_probes: int = 0
    batch_inserts: int = 0
    levels_chunks: int = 0
    outdeg_hist: List[int] = field(default_factory=list)
    frontier_spilled_bytes: int = 0
    frontier_reloaded_bytes: int = 0
    frontier_peak_hbm_bytes: int = 0
    seen: Dict[str, float] = field(default_factory=dict)   # seen-set spill statistics (seen_* fields)
    cand_overflow_records: int = 0
    cand_buffer_peak_bytes: int = 0
    deferred_states: int = 0       # frontier states rebuilt inside k_claim (deferred frontier)
    defer_fallback: bool = False   # the run was redone on the materialising path
    defer_redo_level: int = 0      # ... starting from this level (1 = Init; 0 = no redo)
    narrow_levels: int = 0         # levels run by the device-driven narrow kernel
    claim_mode: str = "minimum"    # the claims that ran: "minimum" (sequential-BFS / rank-major), "first", "tlc"
    cut_state: int = 0             # constraints: successors (and Init states) discarded by a state constraint
    cut_action: int = 0            # ... that passed those and were discarded by an action constraint
    # action properties: the violated one's name (error == "action_property"),
    # the steps checked (= generated - init) and, by name, the steps that
    # violate each, over the levels up to and including the first with one
    error_property: Optional[str] = None
    step_checked: int = 0
    step_violations: Dict[str, int] = field(default_factory=dict)
    trace: List[List[int]] = field(default_factory=list)
    trace_text: str = ""
    # expression-level coverage (run(coverage=True)): base counter name -> its
    # sum over the states expanded; None when off or after an error
    coverage: Optional[Dict[str, int]] = None
    # user-defined invariants (ModelChecker(invariants=...)), in the order given
    user_invariants: List[UserInvariant] = field(default_factory=list)

    @property
    def distinct_per_sec(self) -> float:
        return self.distinct / self.seconds if self.seconds > 0 else 0.0


CLAIM_MODES = {0: "minimum", 1: "first", 2: "tlc"}
_AP_NAMES = {b.bit_length() - 1: n for n, b in ACTION_PROPERTIES.items()}   # bit index -> name


def cover_names() -> List[str]:
    """Names of the coverage base counters, in the order of the C-ABI's vector."""
    lib = load()
    return [lib.kc_cover_name(i).decode() for i in range(lib.kc_cover_count())]


def _result(r: KcResult) -> CheckResult:
    return CheckResult(
        init=r.init, generated=r.generated, distinct=r.distinct, queue_left=r.queue_left,
        depth=r.depth, complete=bool(r.complete),
        act_gen={a: int(r.act_gen[i]) for i, a in enumerate(ACTIONS)},
        act_dist={a: int(r.act_dist[i]) for i, a in enumerate(ACTIONS)},
        level_width=[int(r.level_width[i]) for i in range(r.nlevels)],
        error=ERR_KINDS.get(r.err_kind),
        error_action=ACTIONS[r.err_action] if 0 <= r.err_action < len(ACTIONS) else None,
        error_self=r.err_self,
        error_invariant=INVARIANTS.get(r.err_invariant) if r.err_kind != 4 else None,
        error_property=_AP_NAMES.get(r.err_invariant) if r.err_kind == 4 else None,
        step_checked=int(r.step_checked),
        step_violations={n: int(r.step_violations[b.bit_length() - 1]) for n, b in ACTION_PROPERTIES.items()},
        error_level=r.err_level, trace_len=r.trace_len, seconds=r.seconds,
        collision_optimistic=r.collision_optimistic, fpset_slots=r.fpset_slots,
        peak_frontier=r.peak_frontier, fpset_probes=r.fpset_probes,
        batch_inserts=r.batch_inserts, levels_chunks=r.levels_chunks,
        outdeg_hist=[int(x) for x in r.outdeg_hist],
        frontier_spilled_bytes=r.frontier_spilled_bytes, frontier_reloaded_bytes=r.frontier_reloaded_bytes,
        frontier_peak_hbm_bytes=r.frontier_peak_hbm_bytes,
        seen={f[0][5:]: getattr(r, f[0]) for f in KcResult._fields_ if f[0].startswith("seen_")},
        cand_overflow_records=r.cand_overflow_records, cand_buffer_peak_bytes=r.cand_buffer_peak_bytes,
        deferred_states=r.deferred_states, defer_fallback=bool(r.defer_fallback),
        defer_redo_level=int(r.defer_redo_level), narrow_levels=int(r.narrow_levels),
        claim_mode=CLAIM_MODES.get(r.claim_mode, str(r.claim_mode)),
        cut_state=int(r.cut_state), cut_action=int(r.cut_action))


@dataclass
class CheckpointInfo:
    """The header of a checkpoint file (include/kubecheck.h "Checkpoint")."""
    version: int
    file_bytes: int
    nc: int
    np: int
    ns: int
    can_fail: bool
    can_timeout: bool
    check_deadlock: bool
    variant: int
    invariants: int
    symmetry: int                  # the effective mask
    state_words: int
    keep_trace: bool
    claim_mode: str                # the claims of the run that wrote it
    level: int                     # the BFS level whose top was saved
    nlevels: int
    level_gidx: int
    n: int                         # frontier width
    cand: int
    cand_total: int
    init: int
    distinct: int
    peak_frontier: int
    sections: Dict[str, Dict[str, int]]   # name -> offset, bytes, sum, xor (absent sections left out)


def checkpoint_info(dir: str) -> CheckpointInfo:
    """Read and fully validate DIR/checkpoint.kc on the host (no GPU needed).
    Raises KubecheckError: -2 no file, -22 not a checkpoint or an unknown
    version, -5 truncated, inconsistent or failing a checksum."""
    r = KcCheckpointInfo()
    check("kc_checkpoint_info", load().kc_checkpoint_info(os.fsencode(dir), C.byref(r)))
    sections = {name: {"offset": int(r.section_offset[i]), "bytes": int(r.section_bytes[i]),
                       "sum": int(r.section_sum[i]), "xor": int(r.section_xor[i])}
                for i, name in enumerate(CKPT_SECTIONS) if r.section_bytes[i]}
    return CheckpointInfo(
        version=r.version, file_bytes=r.file_bytes, nc=r.nc, np=r.np, ns=r.ns, can_fail=bool(r.can_fail),
        can_timeout=bool(r.can_timeout), check_deadlock=bool(r.check_deadlock), variant=r.variant,
        invariants=r.invariants, symmetry=r.symmetry, state_words=r.state_words, keep_trace=bool(r.keep_trace),
        claim_mode=CLAIM_MODES.get(r.claim_mode, str(r.claim_mode)), level=r.level, nlevels=r.nlevels,
        level_gidx=r.level_gidx, n=r.n, cand=r.cand, cand_total=r.cand_total, init=r.init, distinct=r.distinct,
        peak_frontier=r.peak_frontier, sections=sections)


class ModelChecker:
    """BFS safety checker (TLC's ModelChecker for this spec) on one GPU."""

    def __init__(self, cfg: Optional[ModelConfig] = None, *, coverage: bool = False,
                 invariants: Optional[Dict[str, str]] = None, **kw):
        """invariants: {name: predicate text} (kubecheck.pred), checked on
        every state the run expands next to the cfg's built-in ones."""
        self.cfg = cfg or ModelConfig(**kw)
        self._lib = load()
        self._h = C.c_void_p()
        self._c = self.cfg.to_c()
        check("kc_engine_create", self._lib.kc_engine_create(C.byref(self._c), C.byref(self._h)))
        self.tuple_words = self._lib.kc_spec_tuple_words(self.cfg.nc, self.cfg.np, self.cfg.ns)
        self._coverage = False
        self._user_invariants: List[str] = []
        if coverage:
            self.set_coverage(True)
        if invariants:
            self.set_invariants(invariants)

    @property
    def instantiation(self) -> str:
        """The model type the engine was built from: "plain", "symmetry",
        "constraints" or "action_properties" (a value of INSTANTIATIONS)."""
        return INSTANTIATIONS[check("kc_engine_instantiation", self._lib.kc_engine_instantiation(self._h))]

    def set_coverage(self, on: bool) -> None:
        """Count expression-level coverage (TLC's -coverage) in the runs that
        follow.  Refused under symmetry reduction and with the spill options."""
        check("kc_engine_set_coverage", self._lib.kc_engine_set_coverage(self._h, int(bool(on))))
        self._coverage = bool(on)

    def set_invariants(self, invariants: Optional[Dict[str, str]]) -> None:
        """Compile {name: predicate text or AST} for this model and check them in
        the runs that follow (at most 8; None or {} turns them off).  Raises
        pred.PredError for a predicate that does not compile, KubecheckError
        where the engine refuses (symmetry, constraints, action properties,
        coverage, checkpoints, the spill options)."""
        if not invariants:
            check("kc_engine_set_invariants", self._lib.kc_engine_set_invariants(self._h, None, 0))
            self._user_invariants = []
            return
        prog = pred.compile_invariants(invariants, self.cfg.nc, self.cfg.np, self.cfg.ns)
        words = (C.c_uint64 * len(prog.words))(*prog.words)
        check("kc_engine_set_invariants", self._lib.kc_engine_set_invariants(self._h, words, prog.n_instr))
        self._user_invariants = list(prog.names)

    def capture_level(self, level: int) -> None:
        check("kc_engine_capture_level", self._lib.kc_engine_capture_level(self._h, level))

    def run(self, coverage: Optional[bool] = None) -> CheckResult:
        """coverage: True / False switches it for this and later runs; None keeps the setting."""
        if coverage is not None and bool(coverage) != self._coverage:
            self.set_coverage(coverage)
        r = KcResult()
        check("kc_engine_run", self._lib.kc_engine_run(self._h, C.byref(r)))
        res = _result(r)
        if self._user_invariants:
            n = 1 + len(self._user_invariants)
            out = (C.c_uint64 * n)()
            check("kc_engine_invariant_stats", self._lib.kc_engine_invariant_stats(self._h, out, n))
            res.user_invariants = [UserInvariant(name, int(out[1 + k]), int(out[0]))
                                   for k, name in enumerate(self._user_invariants)]
            if r.err_kind == 2 and r.err_invariant >= 3:
                res.error_invariant = self._user_invariants[r.err_invariant - 3]
        if self._coverage and res.error is None:
            n = self._lib.kc_cover_count()
            out = (C.c_uint64 * n)()
            check("kc_engine_coverage", self._lib.kc_engine_coverage(self._h, out, n))
            res.coverage = {k: int(out[i]) for i, k in enumerate(cover_names())}
        if res.error is not None and res.trace_len:
            res.trace = [self.trace_tuple(i) for i in range(res.trace_len)]
            n = self._lib.kc_engine_trace_text(self._h, None, 0)
            buf = C.create_string_buffer(n)
            self._lib.kc_engine_trace_text(self._h, buf, n)
            res.trace_text = buf.value.decode()
        return res

    def trace_tuple(self, i: int) -> List[int]:
        out = (C.c_uint64 * self.tuple_words)()
        check("kc_engine_trace_tuple", self._lib.kc_engine_trace_tuple(self._h, i, out))
        return list(out)

    def level_tuples(self, level: int) -> np.ndarray:
        n = check("kc_engine_level_tuples", self._lib.kc_engine_level_tuples(self._h, level, None, 0))
        out = np.zeros((n, self.tuple_words), dtype=np.uint64)
        check("kc_engine_level_tuples", self._lib.kc_engine_level_tuples(
            self._h, level, out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out

    # ---- checkpoint / recover (TLC's -checkpoint / -recover; include/kubecheck.h "Checkpoint")
    def checkpoint(self, dir: str) -> None:
        """Write DIR/checkpoint.kc from the state the last run() left; that
        run must have stopped at max_levels with states on the queue."""
        check("kc_engine_checkpoint", self._lib.kc_engine_checkpoint(self._h, os.fsencode(dir)))

    def recover(self, dir: str) -> None:
        """Arm the next run() to start from DIR/checkpoint.kc instead of Init.
        What that run reports is cumulative, as if it had never stopped."""
        check("kc_engine_recover", self._lib.kc_engine_recover(self._h, os.fsencode(dir)))

    def set_checkpoint(self, dir: Optional[str], every_levels: int = 0, every_seconds: float = 0.0,
                       stage_bytes: int = 0) -> None:
        """Make run() checkpoint into DIR every `every_levels` levels and / or
        every `every_seconds` seconds (each replaces the one before);
        stage_bytes sizes the two pinned staging buffers of every checkpoint
        and recovery of this checker.  dir=None with no period switches run()'s
        checkpoints off."""
        if dir is None and not every_levels and not every_seconds and not stage_bytes:
            check("kc_engine_set_checkpoint", self._lib.kc_engine_set_checkpoint(self._h, None))
            return
        self._ckpt_dir = os.fsencode(dir) if dir is not None else None
        opt = KcCheckpointOptions(self._ckpt_dir, int(every_levels), float(every_seconds), int(stage_bytes))
        check("kc_engine_set_checkpoint", self._lib.kc_engine_set_checkpoint(self._h, C.byref(opt)))

    def kernel_times(self):
        ms = (C.c_double * 4)()
        cnt = (C.c_uint64 * 4)()
        check("kc_engine_kernel_times", self._lib.kc_engine_kernel_times(self._h, ms, cnt))
        names = ["expand", "resolve", "scan", "emit"]
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(names)}

    def check_fps(self):
        """TLC checkFPs on the last run's seen-set: (min gap, 1/min gap)."""
        gap, prob = C.c_uint64(), C.c_double()
        check("kc_engine_check_fps", self._lib.kc_engine_check_fps(self._h, C.byref(gap), C.byref(prob)))
        return int(gap.value), prob.value

    def narrow_times(self):
        """(ms, launches, levels) of the narrow-level kernel in the last run."""
        ms, n, lv = C.c_double(), C.c_uint64(), C.c_uint64()
        check("kc_engine_narrow_times", self._lib.kc_engine_narrow_times(self._h, C.byref(ms), C.byref(n),
                                                                          C.byref(lv)))
        return ms.value, int(n.value), int(lv.value)

    def close(self) -> None:
        if self._h:
            self._lib.kc_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class SimResult:
    """Result of one simulation run (kc_sim_result)."""
    steps: int
    act_steps: Dict[str, int]
    walks_error: int
    walks_depth: int
    walks_terminated: int
    distinct_visited: int
    error: Optional[str]              # None, "assertion", "invariant", "deadlock"
    error_action: Optional[str]
    error_self: int
    error_invariant: Optional[str]
    trace_len: int
    error_walk: int
    seconds: float
    kernel_ms: float
    launches: int = 0
    fpset_slots: int = 0
    trace: List[List[int]] = field(default_factory=list)   # the error walk, replayed on the host
    trace_actions: List[Optional[str]] = field(default_factory=list)
    trace_text: str = ""


class Simulator:
    """Simulation mode (TLC's -simulate) on one GPU: `num_walks` seeded random
    behaviours of at most `depth` states, each state checked against the
    invariants, the Asserts and deadlock (include/kubecheck.h, "Simulation").
    The result depends on (model, seed, num_walks, depth) only."""

    def __init__(self, cfg: Optional[ModelConfig] = None, *, seed: int = 0, num_walks: int = 65536,
                 depth: int = 100, steps_per_launch: int = 0, count_distinct: bool = False,
                 stop_on_error: bool = False, **kw):
        self.cfg = cfg or ModelConfig(**kw)
        self.seed, self.num_walks, self.depth = int(seed) & (2**64 - 1), int(num_walks), int(depth)
        self._lib = load()
        self._h = C.c_void_p()
        self._c = self.cfg.to_c()
        self._s = KcSimConfig(self.seed, self.num_walks & (2**64 - 1), self.depth, int(steps_per_launch),
                              int(count_distinct), int(stop_on_error))
        check("kc_sim_create", self._lib.kc_sim_create(C.byref(self._c), C.byref(self._s), C.byref(self._h)))
        self.tuple_words = self._lib.kc_spec_tuple_words(self.cfg.nc, self.cfg.np, self.cfg.ns)

    def run(self) -> SimResult:
        r = KcSimResult()
        check("kc_sim_run", self._lib.kc_sim_run(self._h, C.byref(r)))
        res = SimResult(
            steps=r.steps, act_steps={a: int(r.act_steps[i]) for i, a in enumerate(ACTIONS)},
            walks_error=r.walks_error, walks_depth=r.walks_depth, walks_terminated=r.walks_terminated,
            distinct_visited=r.distinct_visited, error=ERR_KINDS.get(r.err_kind),
            error_action=ACTIONS[r.err_action] if 0 <= r.err_action < len(ACTIONS) else None,
            error_self=r.err_self, error_invariant=INVARIANTS.get(r.err_invariant),
            trace_len=r.trace_len, error_walk=r.err_walk, seconds=r.seconds, kernel_ms=r.kernel_ms,
            launches=r.launches, fpset_slots=r.fpset_slots)
        if res.error is not None:
            res.trace, res.trace_actions = self.trace(res.error_walk)
            n = check("kc_sim_trace_text", self._lib.kc_sim_trace_text(self._h, res.error_walk, None, 0))
            buf = C.create_string_buffer(n)
            check("kc_sim_trace_text", self._lib.kc_sim_trace_text(self._h, res.error_walk, buf, n))
            res.trace_text = buf.value.decode()
        return res

    def walks(self):
        """(kind, length, final tuple) of every walk of the last run, as numpy
        arrays; kinds are _lib.SIM_KINDS' keys."""
        kind = np.zeros(self.num_walks, dtype=np.uint32)
        length = np.zeros(self.num_walks, dtype=np.uint32)
        final = np.zeros((self.num_walks, self.tuple_words), dtype=np.uint64)
        u32 = C.POINTER(C.c_uint32)
        check("kc_sim_walks", self._lib.kc_sim_walks(self._h, kind.ctypes.data_as(u32),
                                                     length.ctypes.data_as(u32), _u64(final)))
        return kind, length, final

    def trace(self, walk: int):
        """The behaviour of `walk`, replayed on the host and checked against the
        device's record: (states as canonical tuples, the action that led to
        each; None for the Init state)."""
        walk = int(walk)
        n = check("kc_sim_trace", self._lib.kc_sim_trace(self._h, walk, None, None, 0))
        out = np.zeros((n, self.tuple_words), dtype=np.uint64)
        acts = (C.c_int * n)()
        check("kc_sim_trace", self._lib.kc_sim_trace(self._h, walk, _u64(out), acts, n))
        return [[int(x) for x in row] for row in out], [ACTIONS[a] if a >= 0 else None for a in acts]

    def close(self) -> None:
        if self._h:
            self._lib.kc_sim_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class LiveResult:
    """Result of one liveness check (kc_live_result)."""
    property: str
    states: int                       # the reachable graph: the BFS's distinct,
    edges: int                        # ... generated - init
    init: int
    depth: int
    stay_states: int                  # |S|
    live_states: int                  # |L|
    live_terminal: int                # terminal states in L
    rounds: int                       # trim launches, the last (empty) one included
    error: Optional[str]              # None, or "assertion": met while building the graph, no verdict
    error_action: Optional[str]
    error_self: int
    violated: bool
    kind: Optional[str]               # None, "back-to-state", "stuttering"
    prefix_len: int
    trace_len: int
    loop_start: int                   # 0-based index the last state steps back to; -1 if stuttering
    seconds: float
    build_ms: float
    trim_ms: float
    trace: List[List[int]] = field(default_factory=list)
    trace_actions: List[Optional[str]] = field(default_factory=list)
    trace_text: str = ""
    fairness: str = "next"            # a name of FAIRNESS; the fields below are 0 under "next"
    sccs: int = 0                     # SCCs of more than one state in S
    fair_sccs: int = 0                # ... that are fair
    fair_states: int = 0              # |F|
    scc_rounds: int = 0               # launches of the SCC and closure phases that end in a counter read
    scc_ms: float = 0.0
    formula: Optional[str] = None     # a user formula's text; the fields below are 0 for a built-in property
    trigger_stay: int = 0             # |S /\ T|: stay states in the trigger set
    trigger_live: int = 0             # |L /\ T|: violated iff not 0


class LivenessChecker:
    """A temporal property of KubeAPI.tla on one GPU (include/kubecheck.h,
    "Liveness"): the reachable graph, the elimination of the states no fair
    behaviour can stay in, and a lasso counterexample.  `property` is a name of
    PROPERTIES or its index; `fairness` a name of FAIRNESS: "next" is
    WF_vars(Next), "process" weak fairness of every process (PlusCal's `fair
    process`), decided on the fair SCCs of the stay states.

    `formula` instead of `property` checks a temporal formula of the user's:
    P ~> Q, [](P => <>Q), []<>Q or <>Q over predicates of kubecheck.pred
    (pred.parse_temporal), reported under `name`; set_formula()
    gives such a handle another one.  `program=(form, program)` does the same
    with a compiled pair of predicates (pred.compile_temporal).  property=-1
    alone is refused by the library: a handle never lacks its formula."""

    def __init__(self, cfg: Optional[ModelConfig] = None, property=None,
                 max_states: Optional[int] = None, fairness: str = "next", *, formula: Optional[str] = None,
                 name: Optional[str] = None, program=None, **kw):
        if fairness not in FAIRNESS:
            raise ValueError(f"unknown fairness {fairness!r}; known: {FAIRNESS}")
        self.fairness = fairness
        self.cfg = cfg or ModelConfig(**kw)
        if (formula is not None) + (property is not None) + (program is not None) > 1:
            raise ValueError("LivenessChecker: give `property` (a built-in) or `formula` (or `program`), not both")
        self.formula = formula
        self.name = name
        compiled = program
        if formula is not None:
            # compiled before anything is allocated: a bad formula is a pred.PredError
            compiled = pred.compile_temporal(formula, self.cfg.nc, self.cfg.np, self.cfg.ns)
        if compiled is not None:
            property = LIVE_USER
        elif property is None:
            property = "ReconcileCompletes"
        if isinstance(property, str):
            if property not in PROPERTIES:
                raise ValueError(f"unknown property {property!r}; known: {PROPERTIES}")
            property = PROPERTIES.index(property)
        self.property = int(property)
        self._lib = load()
        self._h = C.c_void_p()
        self._c = self.cfg.to_c()
        self._l = KcLiveConfig(self.property, int(max_states or 0), FAIRNESS.index(fairness))
        if compiled is not None:
            form, arr, n_instr = self._program_args(*compiled)
            check("kc_live_create_formula", self._lib.kc_live_create_formula(
                C.byref(self._c), C.byref(self._l), form, arr, n_instr, C.byref(self._h)))
        else:
            check("kc_live_create", self._lib.kc_live_create(C.byref(self._c), C.byref(self._l), C.byref(self._h)))
        self.tuple_words = self._lib.kc_spec_tuple_words(self.cfg.nc, self.cfg.np, self.cfg.ns)

    @staticmethod
    def _program_args(form, program):
        if isinstance(form, str):
            form = LIVE_FORMS.index(form)
        words = list(program.words if hasattr(program, "words") else program)
        return int(form), (C.c_uint64 * max(1, len(words)))(*words), len(words) // 2

    def set_formula(self, formula: str, name: Optional[str] = None) -> None:
        """The formula the runs that follow check (a handle made with `formula` or `program`)."""
        self.set_program(*pred.compile_temporal(formula, self.cfg.nc, self.cfg.np, self.cfg.ns))
        self.formula, self.name = formula, name if name is not None else self.name

    def set_program(self, form, program) -> None:
        """kc_live_set_formula with a compiled program (a pred.Program or its
        words): form 0 / "leads-to" or 1 / "eventually"; exactly two predicates,
        END 0 = P and END 1 = Q.  KubecheckError -22 where the library refuses."""
        form, arr, n_instr = self._program_args(form, program)
        check("kc_live_set_formula", self._lib.kc_live_set_formula(self._h, form, arr, n_instr))

    def run(self) -> LiveResult:
        r = KcLiveResult()
        check("kc_live_run", self._lib.kc_live_run(self._h, C.byref(r)))
        ts, tl = C.c_uint64(), C.c_uint64()
        check("kc_live_trigger_counts", self._lib.kc_live_trigger_counts(self._h, C.byref(ts), C.byref(tl)))
        user = self.property == LIVE_USER
        res = LiveResult(
            property=(self.name or "formula") if user else PROPERTIES[self.property],
            states=r.states, edges=r.edges, init=r.init, depth=r.depth,
            stay_states=r.stay_states, live_states=r.live_states, live_terminal=r.live_terminal,
            rounds=r.rounds, error=ERR_KINDS.get(r.err_kind),
            error_action=ACTIONS[r.err_action] if 0 <= r.err_action < len(ACTIONS) else None,
            error_self=r.err_self, violated=bool(r.violated), kind=LIVE_KINDS.get(r.kind),
            prefix_len=r.prefix_len, trace_len=r.trace_len, loop_start=r.loop_start, seconds=r.seconds,
            build_ms=r.build_ms, trim_ms=r.trim_ms, fairness=self.fairness, sccs=r.sccs, fair_sccs=r.fair_sccs,
            fair_states=r.fair_states, scc_rounds=r.scc_rounds, scc_ms=r.scc_ms,
            formula=self.formula if user else None, trigger_stay=ts.value, trigger_live=tl.value)
        if res.violated:
            n = res.trace_len
            out = np.zeros((n, self.tuple_words), dtype=np.uint64)
            acts = (C.c_int * n)()
            check("kc_live_trace", self._lib.kc_live_trace(self._h, _u64(out), acts, n))
            res.trace = [[int(x) for x in row] for row in out]
            res.trace_actions = [ACTIONS[a] if a >= 0 else None for a in acts]
            nb = check("kc_live_trace_text", self._lib.kc_live_trace_text(self._h, None, 0))
            buf = C.create_string_buffer(nb)
            check("kc_live_trace_text", self._lib.kc_live_trace_text(self._h, buf, nb))
            res.trace_text = buf.value.decode()
        return res

    def alive(self):
        """Every state of the last run's graph in discovery order (canonical
        tuples) and its final alive bit (True = in L), as numpy arrays."""
        n = check("kc_live_alive", self._lib.kc_live_alive(self._h, None, None, 0))
        tuples = np.zeros((n, self.tuple_words), dtype=np.uint64)
        bits = np.zeros(n, dtype=np.uint8)
        check("kc_live_alive", self._lib.kc_live_alive(self._h, _u64(tuples),
                                                       bits.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        return tuples, bits.astype(bool)

    def edge_procs(self):
        """Every edge of the last run's graph (fairness="process" only): source
        and target discovery indices and the process that takes the step, as
        numpy arrays."""
        n = check("kc_live_edge_procs", self._lib.kc_live_edge_procs(self._h, None, None, None, 0))
        src, dst = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        proc = np.zeros(n, dtype=np.uint8)
        u32 = C.POINTER(C.c_uint32)
        check("kc_live_edge_procs", self._lib.kc_live_edge_procs(
            self._h, src.ctypes.data_as(u32), dst.ctypes.data_as(u32), proc.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        return src, dst, proc

    def close(self) -> None:
        if self._h:
            self._lib.kc_live_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream(stream):
    return C.c_void_p(stream.cuda_stream if stream is not None else 0)


def stress_fps_dev(seed: int, kind: int, n_ins: int, start: int, n: int, out, stream=None) -> None:
    """Stress stream entries [start, start+n) into a device tensor
    (kind 0 = inserts, 1 = lookups; kc_stress_fps_dev)."""
    check("kc_stress_fps_dev", load().kc_stress_fps_dev(seed, kind, n_ins, start, n,
                                                         C.c_void_p(out.data_ptr()), _stream(stream)))


def stress_fp(seed: int, kind: int, n_ins: int, i: int) -> int:
    return int(load().kc_stress_fp(seed, kind, n_ins, i))


def _u64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


class FPSet:
    """tlc2.tool.fp.FPSet on HBM.  put() returns True iff fp was already present."""

    def __init__(self, capacity: int = 1 << 20, device: int = 0):
        self._lib = load()
        self._h = C.c_void_p()
        check("kc_fpset_create", self._lib.kc_fpset_create(int(capacity), device, C.byref(self._h)))

    def put_batch(self, fps) -> np.ndarray:
        a = np.ascontiguousarray(fps, dtype=np.uint64)
        seen = np.zeros(a.shape[0], dtype=np.uint8)
        check("kc_fpset_put_batch", self._lib.kc_fpset_put_batch(
            self._h, _u64(a), a.shape[0], seen.ctypes.data_as(C.POINTER(C.c_uint8))))
        return seen.astype(bool)

    def contains_batch(self, fps) -> np.ndarray:
        a = np.ascontiguousarray(fps, dtype=np.uint64)
        seen = np.zeros(a.shape[0], dtype=np.uint8)
        check("kc_fpset_contains_batch", self._lib.kc_fpset_contains_batch(
            self._h, _u64(a), a.shape[0], seen.ctypes.data_as(C.POINTER(C.c_uint8))))
        return seen.astype(bool)

    def put(self, fp: int) -> bool:
        """TLC FPSet.put(long): thread-safe; concurrent callers are
        flat-combined into one batch launch (kc_fpset_put)."""
        seen = C.c_int()
        check("kc_fpset_put", self._lib.kc_fpset_put(self._h, int(fp) & (2**64 - 1), C.byref(seen)))
        return bool(seen.value)

    def contains(self, fp: int) -> bool:
        seen = C.c_int()
        check("kc_fpset_contains", self._lib.kc_fpset_contains(self._h, int(fp) & (2**64 - 1), C.byref(seen)))
        return bool(seen.value)

    def combine_rounds(self) -> int:
        """Batches launched so far by put()/contains()."""
        return int(self._lib.kc_fpset_combine_rounds(self._h))

    # -- device-resident batches (torch tensors of int64 on this set's GPU)
    def insert_count_dev(self, fps, n: int, stream=None) -> int:
        """Insert the first n fps of a device tensor; returns how many were new."""
        out = C.c_uint64()
        check("kc_fpset_insert_count_dev", self._lib.kc_fpset_insert_count_dev(
            self._h, C.c_void_p(fps.data_ptr()), n, C.byref(out), _stream(stream)))
        return int(out.value)

    def contains_count_dev(self, fps, n: int, stream=None) -> int:
        out = C.c_uint64()
        check("kc_fpset_contains_count_dev", self._lib.kc_fpset_contains_count_dev(
            self._h, C.c_void_p(fps.data_ptr()), n, C.byref(out), _stream(stream)))
        return int(out.value)

    def partition_dev(self, fps, n: int, world: int, out, stream=None) -> List[int]:
        """Stable counting sort of n device fps by owner rank into `out`;
        returns the per-owner counts."""
        counts = (C.c_uint64 * world)()
        check("kc_fpset_partition_dev", self._lib.kc_fpset_partition_dev(
            self._h, C.c_void_p(fps.data_ptr()), n, world, C.c_void_p(out.data_ptr()), counts,
            _stream(stream)))
        return [int(x) for x in counts]

    def size(self) -> int:
        return int(self._lib.kc_fpset_size(self._h))

    def capacity(self) -> int:
        return int(self._lib.kc_fpset_capacity(self._h))

    def checkFPs(self) -> float:
        gap = C.c_uint64()
        prob = C.c_double()
        check("kc_fpset_check_fps", self._lib.kc_fpset_check_fps(self._h, C.byref(gap), C.byref(prob)))
        self.min_gap = gap.value
        return prob.value

    def stress(self, seed: int, n: int, batch: int, n_lookup: int):
        ti, tl, found = C.c_double(), C.c_double(), C.c_uint64()
        check("kc_fpset_stress", self._lib.kc_fpset_stress(
            self._h, seed, n, batch, n_lookup, C.byref(ti), C.byref(tl), C.byref(found)))
        return ti.value, tl.value, found.value

    def close(self) -> None:
        if self._h:
            self._lib.kc_fpset_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StateQueue:
    """tlc2.tool.queue.StateQueue (the recorded run's DiskStateQueue,
    MC.out:5): a FIFO of fixed-width packed states in segments over HBM,
    pinned host RAM past `hbm_bytes`, and spill files in `spill_dir` past
    `host_bytes` (include/kubecheck.h kc_squeue_*).  Host-array calls are
    synchronous; the ``*_dev`` calls take device pointers or CUDA tensors and
    an optional HIP stream (None = the queue's own stream, ordered with the
    default stream)."""

    def __init__(self, state_words: int, capacity: int = 0, device: int = 0, *, segment_states: int = 0,
                 hbm_bytes: int = 0, host_bytes: int = 0, spill_dir: Optional[str] = None):
        self._lib = load()
        self.words = state_words
        self._h = C.c_void_p()
        if capacity and not (segment_states or hbm_bytes or host_bytes or spill_dir):
            check("kc_squeue_create", self._lib.kc_squeue_create(state_words, capacity, device, C.byref(self._h)))
            return
        c = KcSqueueConfig(state_words=state_words, device=device, segment_states=segment_states or capacity,
                           hbm_bytes=hbm_bytes, host_bytes=host_bytes,
                           spill_dir=spill_dir.encode() if spill_dir else None)
        check("kc_squeue_create2", self._lib.kc_squeue_create2(C.byref(c), C.byref(self._h)))

    @staticmethod
    def _ptr(x) -> int:
        return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)

    @staticmethod
    def _st(stream):
        if stream is None:
            return None
        return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))

    def enqueue(self, states: np.ndarray) -> None:
        a = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, self.words)
        check("kc_squeue_enqueue", self._lib.kc_squeue_enqueue(self._h, _u64(a), a.shape[0]))

    def dequeue(self, max_n: int) -> np.ndarray:
        out = np.zeros((max_n, self.words), dtype=np.uint64)
        n = C.c_size_t()
        check("kc_squeue_dequeue", self._lib.kc_squeue_dequeue(self._h, _u64(out), max_n, C.byref(n)))
        return out[: n.value]

    def enqueue_dev(self, states, n: Optional[int] = None, stream=None) -> None:
        """Append n states from device memory (a CUDA tensor of n x words
        64-bit values, or a device pointer with n given)."""
        if n is None:
            n = states.numel() // self.words
        check("kc_squeue_enqueue_dev",
              self._lib.kc_squeue_enqueue_dev(self._h, C.c_void_p(self._ptr(states)), n, self._st(stream)))

    def dequeue_dev(self, out, max_n: int, stream=None) -> int:
        """Move up to max_n head states into device memory; returns the count."""
        got = C.c_size_t()
        check("kc_squeue_dequeue_dev", self._lib.kc_squeue_dequeue_dev(
            self._h, C.c_void_p(self._ptr(out)), max_n, C.byref(got), self._st(stream)))
        return got.value

    def reserve_dev(self, n: int, stream=None) -> int:
        """Device pointer to n writable states at the tail (then commit)."""
        p = C.c_void_p()
        check("kc_squeue_reserve_dev", self._lib.kc_squeue_reserve_dev(self._h, n, C.byref(p), self._st(stream)))
        return int(p.value)

    def commit(self, n: int, stream=None) -> None:
        check("kc_squeue_commit", self._lib.kc_squeue_commit(self._h, n, self._st(stream)))

    def front_dev(self, offset: int, max_n: int, stream=None):
        """(device pointer, count) of a contiguous run `offset` states after
        the head; count may be < max_n at a segment end."""
        p = C.c_void_p()
        got = C.c_size_t()
        check("kc_squeue_front_dev", self._lib.kc_squeue_front_dev(
            self._h, offset, max_n, C.byref(p), C.byref(got), self._st(stream)))
        return int(p.value or 0), got.value

    def pop(self, n: int, stream=None) -> None:
        check("kc_squeue_pop", self._lib.kc_squeue_pop(self._h, n, self._st(stream)))

    def peek(self, offset: int, n: int) -> np.ndarray:
        out = np.zeros((n, self.words), dtype=np.uint64)
        check("kc_squeue_peek", self._lib.kc_squeue_peek(self._h, offset, n, _u64(out), None))
        return out

    def stats(self) -> Dict[str, int]:
        st = KcSqueueStats()
        check("kc_squeue_get_stats", self._lib.kc_squeue_get_stats(self._h, C.byref(st)))
        return {f[0]: int(getattr(st, f[0])) for f in KcSqueueStats._fields_}

    def size(self) -> int:
        return int(self._lib.kc_squeue_size(self._h))

    def close(self) -> None:
        if self._h:
            self._lib.kc_squeue_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Spec:
    """Host access to the lowered spec (canonical tuples; no GPU needed)."""

    def __init__(self, cfg: Optional[ModelConfig] = None, **kw):
        self.cfg = cfg or ModelConfig(**kw)
        self._lib = load()
        self._c = self.cfg.to_c()
        self.tuple_words = check("kc_spec_tuple_words",
                                 self._lib.kc_spec_tuple_words(self.cfg.nc, self.cfg.np, self.cfg.ns))
        self.state_words = check("kc_spec_state_words",
                                 self._lib.kc_spec_state_words(self.cfg.nc, self.cfg.np, self.cfg.ns))

    def init(self) -> np.ndarray:
        n = check("kc_spec_init", self._lib.kc_spec_init(C.byref(self._c), None, 0))
        out = np.zeros((n, self.tuple_words), dtype=np.uint64)
        self._lib.kc_spec_init(C.byref(self._c), _u64(out), n)
        return out

    def successors(self, tup):
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        cap = 64
        acts = (C.c_int * cap)()
        out = np.zeros((cap, self.tuple_words), dtype=np.uint64)
        fail = C.c_int(-1)
        n = self._lib.kc_spec_successors(C.byref(self._c), _u64(t), acts, _u64(out), cap, C.byref(fail))
        if n == -2:
            return None, ACTIONS[fail.value]
        check("kc_spec_successors", n)
        return [(ACTIONS[acts[i]], out[i]) for i in range(n)], None

    def cover(self, tuples) -> Dict[str, int]:
        """Coverage base counters summed over canonical tuples (n x tuple_words),
        each taken as a state the BFS expands: the host definition of
        CheckResult.coverage."""
        t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, self.tuple_words)
        n = self._lib.kc_cover_count()
        out = (C.c_uint64 * n)()
        check("kc_spec_cover", self._lib.kc_spec_cover(C.byref(self._c), _u64(t), t.shape[0], out))
        return {k: int(out[i]) for i, k in enumerate(cover_names())}

    def eval_invariant(self, expr, tuples) -> np.ndarray:
        """A user-defined invariant (predicate text or AST) on canonical tuples
        (n x tuple_words), compiled and run on the host through the code k_pred
        runs: one bool per tuple, True where it holds."""
        prog = pred.compile_invariants([expr], self.cfg.nc, self.cfg.np, self.cfg.ns)
        words = (C.c_uint64 * len(prog.words))(*prog.words)
        t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, self.tuple_words)
        out = np.zeros(t.shape[0], dtype=bool)
        for i in range(t.shape[0]):
            out[i] = check("kc_pred_eval", self._lib.kc_pred_eval(C.byref(self._c), words, prog.n_instr, _u64(t[i]))) == 0
        return out

    def check_invariants(self, tup) -> Optional[str]:
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        r = self._lib.kc_spec_check(C.byref(self._c), _u64(t))
        if r < -1:
            check("kc_spec_check", r)
        return INVARIANTS.get(r)

    def fingerprint(self, tup) -> int:
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        fp = C.c_uint64()
        check("kc_spec_fingerprint", self._lib.kc_spec_fingerprint(C.byref(self._c), _u64(t), C.byref(fp)))
        return fp.value

    def fingerprint_own(self, tup) -> int:
        """The fingerprint of the sharded path: fingerprint() with the owner
        projection in its top bits (kc_shard_owner reads the owner from it)."""
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        fp = C.c_uint64()
        check("kc_spec_fingerprint_own", self._lib.kc_spec_fingerprint_own(C.byref(self._c), _u64(t), C.byref(fp)))
        return fp.value

    def fingerprint_sym(self, tup) -> int:
        """The fingerprint the engine stores under cfg.symmetry: the minimum
        of fingerprint() over the state's permutation orbit."""
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        fp = C.c_uint64()
        check("kc_spec_fingerprint_sym", self._lib.kc_spec_fingerprint_sym(C.byref(self._c), _u64(t), C.byref(fp)))
        return fp.value

    def permute(self, tup, perm) -> np.ndarray:
        """The state with actor a moved to index perm[a] (clients among
        themselves, controllers among themselves)."""
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        if len(perm) != self.cfg.nc + self.cfg.np:
            raise ValueError(f"perm has {len(perm)} entries, the model {self.cfg.nc + self.cfg.np} actors")
        p = (C.c_int * len(perm))(*[int(x) for x in perm])
        out = np.zeros(self.tuple_words, dtype=np.uint64)
        check("kc_spec_permute", self._lib.kc_spec_permute(C.byref(self._c), _u64(t), p, _u64(out)))
        return out

    def sym_selftest_fps(self, tuples) -> np.ndarray:
        """fingerprint_sym of every row of `tuples`, computed on the GPU by
        the device code the engine's kernels call (test harness)."""
        t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, self.tuple_words)
        out = np.zeros(len(t), dtype=np.uint64)
        check("kc_sym_selftest_fps", self._lib.kc_sym_selftest_fps(C.byref(self._c), _u64(t), len(t), _u64(out)))
        return out

    def in_model(self, tup_s, tup_x, action) -> Optional[str]:
        """Under cfg's constraints, is successor tup_x of tup_s (made by
        `action`, a name of ACTIONS or its id) in the model?  None (in),
        "state" or "action" (the kind of constraint that cuts it).  tup_s may
        be None for an Init state when no action constraint is set (host; no GPU)."""
        x = np.ascontiguousarray(tup_x, dtype=np.uint64)
        s = None if tup_s is None else np.ascontiguousarray(tup_s, dtype=np.uint64)
        a = ACTIONS.index(action) if isinstance(action, str) else int(action)
        return CUTS[check("kc_spec_in_model", self._lib.kc_spec_in_model(
            C.byref(self._c), None if s is None else _u64(s), _u64(x), a))]

    def step_violations(self, tup_s, tup_x, action) -> int:
        """The mask of cfg's action properties (ACTION_PROPERTIES bits) that the
        step tup_s -> tup_x, made by `action` (a name of ACTIONS or its id),
        violates; 0 when the tuples are equal (host; no GPU)."""
        s = np.ascontiguousarray(tup_s, dtype=np.uint64)
        x = np.ascontiguousarray(tup_x, dtype=np.uint64)
        a = ACTIONS.index(action) if isinstance(action, str) else int(action)
        return check("kc_spec_step_violations", self._lib.kc_spec_step_violations(C.byref(self._c), _u64(s), _u64(x), a))

    def act_selftest(self, tuples_s, tuples_x, actions) -> np.ndarray:
        """kc_spec_step_violations' mask for every (parent, successor, action
        id) triple, computed on the GPU by the device code the engine's
        kernels call (test harness)."""
        s = np.ascontiguousarray(tuples_s, dtype=np.uint64).reshape(-1, self.tuple_words)
        x = np.ascontiguousarray(tuples_x, dtype=np.uint64).reshape(-1, self.tuple_words)
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if not (len(s) == len(x) == len(a)):
            raise ValueError("act_selftest: parents, successors and actions differ in length")
        out = np.zeros(len(a), dtype=np.int32)
        ip = C.POINTER(C.c_int)
        check("kc_act_selftest", self._lib.kc_act_selftest(C.byref(self._c), _u64(s), _u64(x), a.ctypes.data_as(ip),
                                                           len(a), out.ctypes.data_as(ip)))
        return out

    def con_selftest(self, tuples_s, tuples_x, actions) -> np.ndarray:
        """kc_spec_in_model's answer (0 in, 1 state-cut, 2 action-cut) for every
        (parent, successor, action id) triple, computed on the GPU by the
        device code the engine's kernels call (test harness)."""
        s = np.ascontiguousarray(tuples_s, dtype=np.uint64).reshape(-1, self.tuple_words)
        x = np.ascontiguousarray(tuples_x, dtype=np.uint64).reshape(-1, self.tuple_words)
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if not (len(s) == len(x) == len(a)):
            raise ValueError("con_selftest: parents, successors and actions differ in length")
        out = np.zeros(len(a), dtype=np.int32)
        ip = C.POINTER(C.c_int)
        check("kc_con_selftest", self._lib.kc_con_selftest(C.byref(self._c), _u64(s), _u64(x), a.ctypes.data_as(ip),
                                                           len(a), out.ctypes.data_as(ip)))
        return out

    def fp_selfcheck(self, tup) -> int:
        """Successors whose incremental (kernel) fingerprint differs from the
        full one; 0 expected."""
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        return check("kc_spec_fp_selfcheck", self._lib.kc_spec_fp_selfcheck(C.byref(self._c), _u64(t)))

    @staticmethod
    def sim_rand(seed: int, walk: int, k: int) -> int:
        """r(walk, k) of the simulation RNG (kc_sim_rand)."""
        return int(load().kc_sim_rand(seed & (2**64 - 1), walk & (2**64 - 1), k & (2**64 - 1)))

    @staticmethod
    def sim_pick(r: int, n: int) -> int:
        """floor(r * n / 2^64) (kc_sim_pick)."""
        return int(load().kc_sim_pick(r & (2**64 - 1), n))

    def sim_replay(self, seed: int, depth: int, walk: int):
        """One simulated walk on the host (kc_sim_replay; no GPU): (states as
        canonical tuples, the action that led to each (None for Init), how it
        ended: a value of SIM_KINDS)."""
        kind = C.c_int()
        n = check("kc_sim_replay", self._lib.kc_sim_replay(C.byref(self._c), seed & (2**64 - 1), depth, walk,
                                                           None, None, 0, C.byref(kind)))
        out = np.zeros((n, self.tuple_words), dtype=np.uint64)
        acts = (C.c_int * n)()
        check("kc_sim_replay", self._lib.kc_sim_replay(C.byref(self._c), seed & (2**64 - 1), depth, walk,
                                                       _u64(out), acts, n, C.byref(kind)))
        return out, [ACTIONS[a] if a >= 0 else None for a in acts], SIM_KINDS[kind.value]

    def stay(self, property, tup) -> bool:
        """stay(tuple) of a temporal property (a name of PROPERTIES or its
        index) on the host (kc_live_stay; no GPU)."""
        prop = PROPERTIES.index(property) if isinstance(property, str) else int(property)
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        return bool(check("kc_live_stay", self._lib.kc_live_stay(C.byref(self._c), prop, _u64(t))))

    def step_process(self, tup, ordinal: int) -> int:
        """The process (actors 0 .. A-1, then the servers) that takes the step
        to successor `ordinal` of a state, in successors() order, on the host
        (kc_live_step_process; no GPU)."""
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        return check("kc_live_step_process", self._lib.kc_live_step_process(C.byref(self._c), _u64(t), int(ordinal)))

    def pack(self, tup) -> np.ndarray:
        t = np.ascontiguousarray(tup, dtype=np.uint64)
        out = np.zeros(self.state_words, dtype=np.uint64)
        check("kc_spec_pack", self._lib.kc_spec_pack(C.byref(self._c), _u64(t), _u64(out)))
        return out

    def unpack(self, packed) -> np.ndarray:
        p = np.ascontiguousarray(packed, dtype=np.uint64)
        out = np.zeros(self.tuple_words, dtype=np.uint64)
        check("kc_spec_unpack", self._lib.kc_spec_unpack(C.byref(self._c), _u64(p), _u64(out)))
        return out
