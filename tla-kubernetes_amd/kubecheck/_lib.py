"""ctypes binding of libkubecheck.so (include/kubecheck.h).

The library is built in-tree (tla-kubernetes_amd/csrc/Makefile ->
tla-kubernetes_amd/kubecheck/lib/libkubecheck.so).  There is no Python or CPU
fallback for the model checker: if the library is missing, importing the
product raises, and engine calls on a machine without a GPU fail with ENODEV.
"""
from __future__ import annotations

import ctypes as C
import os

LIB_PATH = os.environ.get("KUBECHECK_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libkubecheck.so")

KC_NACTIONS = 22
KC_MAX_LEVELS = 4096

ACTIONS = [
    "DoRequest", "DoReply", "DoListRequest", "DoListReply", "CStart", "C1", "C10", "C11",
    "c12", "C13", "C2", "C3", "C8", "C6", "C7", "C4", "C5", "PVCStart", "PVCListedPVCs",
    "PVCHavePVCs", "PVCDone", "APIStart",
]

# action constraints (kc_model_config.action_constraints bits), and what
# kc_spec_in_model / kc_con_selftest answer
ACTION_CONSTRAINTS = {"ServeClientsFirst": 1}
CUTS = {0: None, 1: "state", 2: "action"}
# kc_engine_instantiation
INSTANTIATIONS = {0: "plain", 1: "symmetry", 2: "constraints", 3: "action_properties"}
# action properties (kc_model_config.action_properties bits; a violated one's
# bit index is kc_result.err_invariant when err_kind is 4)
ACTION_PROPERTIES = {"NoBlindUpdate": 1, "OneReplyPerStep": 2, "StoreNeverShrinks": 4}

ERR_KINDS = {0: None, 1: "assertion", 2: "invariant", 3: "deadlock", 4: "action_property"}
INVARIANTS = {0: "TypeOK", 1: "OnlyOneVersion", 2: "NoLostUpdate"}


class KcModelConfig(C.Structure):
    _fields_ = [
        ("nc", C.c_int), ("np", C.c_int), ("ns", C.c_int),
        ("can_fail", C.c_int), ("can_timeout", C.c_int), ("check_deadlock", C.c_int),
        ("variant", C.c_int), ("device", C.c_int), ("keep_trace", C.c_int),
        ("max_levels", C.c_int), ("fpset_slots", C.c_uint64), ("chunk_states", C.c_uint64),
        ("verbose", C.c_int), ("timing", C.c_int), ("invariants", C.c_int),
        ("frontier_hbm_bytes", C.c_uint64), ("frontier_host_bytes", C.c_uint64),
        ("frontier_segment_states", C.c_uint64), ("spill_dir", C.c_char_p), ("trace_host", C.c_int),
        ("seen_hbm_bytes", C.c_uint64), ("seen_host_bytes", C.c_uint64),
        ("tlc_order", C.c_int),
        ("first_claim", C.c_int),
        ("symmetry", C.c_int),
        ("constraint_stored", C.c_int), ("constraint_inflight", C.c_int), ("action_constraints", C.c_int),
        ("action_properties", C.c_int),
    ]


class KcResult(C.Structure):
    _fields_ = [
        ("init", C.c_uint64), ("generated", C.c_uint64), ("distinct", C.c_uint64),
        ("queue_left", C.c_uint64), ("depth", C.c_int), ("complete", C.c_int),
        ("act_gen", C.c_uint64 * KC_NACTIONS), ("act_dist", C.c_uint64 * KC_NACTIONS),
        ("nlevels", C.c_int), ("level_width", C.c_uint64 * KC_MAX_LEVELS),
        ("err_kind", C.c_int), ("err_action", C.c_int), ("err_self", C.c_int),
        ("err_invariant", C.c_int), ("err_level", C.c_int), ("trace_len", C.c_int),
        ("seconds", C.c_double), ("collision_optimistic", C.c_double),
        ("fpset_slots", C.c_uint64), ("peak_frontier", C.c_uint64),
        ("fpset_probes", C.c_uint64), ("batch_inserts", C.c_uint64),
        ("levels_chunks", C.c_uint64), ("outdeg_hist", C.c_uint64 * 16),
        ("frontier_spilled_bytes", C.c_uint64), ("frontier_reloaded_bytes", C.c_uint64),
        ("frontier_peak_hbm_bytes", C.c_uint64),
        ("seen_flushes", C.c_uint64), ("seen_cold_fps", C.c_uint64), ("seen_cold_runs", C.c_uint64),
        ("seen_cold_queries", C.c_uint64), ("seen_cold_hits", C.c_uint64), ("seen_merges", C.c_uint64),
        ("seen_filter_tests", C.c_uint64), ("seen_filter_passed", C.c_uint64),
        ("seen_disk_bytes", C.c_uint64), ("seen_peak_hbm_bytes", C.c_uint64), ("seen_seconds", C.c_double),
        ("seen_flush_seconds", C.c_double), ("seen_merge_seconds", C.c_double), ("seen_check_seconds", C.c_double),
        ("cand_overflow_records", C.c_uint64), ("cand_buffer_peak_bytes", C.c_uint64),
        ("deferred_states", C.c_uint64), ("defer_fallback", C.c_uint64),
        ("defer_redo_level", C.c_uint64), ("narrow_levels", C.c_uint64),
        ("claim_mode", C.c_int),
        ("cut_state", C.c_uint64), ("cut_action", C.c_uint64),
        ("step_checked", C.c_uint64), ("step_violations", C.c_uint64 * 3),
    ]


KC_CKPT_SECTIONS = 5
CKPT_SECTIONS = ("COUNTERS", "FRONTIER", "FPS", "TRACE_PARENT", "TRACE_ORD")


class KcCheckpointInfo(C.Structure):
    _fields_ = [("version", C.c_uint64), ("file_bytes", C.c_uint64),
                ("nc", C.c_int), ("np", C.c_int), ("ns", C.c_int), ("can_fail", C.c_int), ("can_timeout", C.c_int),
                ("check_deadlock", C.c_int), ("variant", C.c_int), ("invariants", C.c_int), ("symmetry", C.c_int),
                ("state_words", C.c_int), ("keep_trace", C.c_int), ("claim_mode", C.c_int),
                ("level", C.c_int), ("nlevels", C.c_int),
                ("level_gidx", C.c_uint64), ("n", C.c_uint64), ("cand", C.c_uint64), ("cand_total", C.c_uint64),
                ("init", C.c_uint64), ("distinct", C.c_uint64), ("peak_frontier", C.c_uint64),
                ("section_offset", C.c_uint64 * KC_CKPT_SECTIONS), ("section_bytes", C.c_uint64 * KC_CKPT_SECTIONS),
                ("section_sum", C.c_uint64 * KC_CKPT_SECTIONS), ("section_xor", C.c_uint64 * KC_CKPT_SECTIONS)]


class KcCheckpointOptions(C.Structure):
    _fields_ = [("dir", C.c_char_p), ("every_levels", C.c_int), ("every_seconds", C.c_double),
                ("stage_bytes", C.c_uint64)]


KC_SIM_MAX_DEPTH = 65535
# how a simulated walk ended (kc_sim_walks / kc_sim_replay): ERR_KINDS' 1-3, then
SIM_KINDS = {0: "running", 1: "assertion", 2: "invariant", 3: "deadlock", 4: "depth", 5: "terminated"}


class KcSimConfig(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("num_walks", C.c_uint64), ("depth", C.c_int),
                ("steps_per_launch", C.c_int), ("count_distinct", C.c_int), ("stop_on_error", C.c_int)]


class KcSimResult(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("act_steps", C.c_uint64 * KC_NACTIONS),
                ("walks_error", C.c_uint64), ("walks_depth", C.c_uint64), ("walks_terminated", C.c_uint64),
                ("distinct_visited", C.c_uint64),
                ("err_kind", C.c_int), ("err_action", C.c_int), ("err_self", C.c_int),
                ("err_invariant", C.c_int), ("trace_len", C.c_int), ("err_walk", C.c_uint64),
                ("seconds", C.c_double), ("kernel_ms", C.c_double),
                ("launches", C.c_uint64), ("fpset_slots", C.c_uint64)]


# temporal properties kc_live_* checks (kc_live_config.property = the index)
PROPERTIES = ("ReconcileCompletes", "CleansUpProperly", "ClientRestarts", "SomeActorRestarts")
# kc_live_config.property of a user formula (kc_live_create_formula); the forms it takes
LIVE_USER = -1
LIVE_FORMS = ("leads-to", "eventually")
# how a liveness counterexample ends (kc_live_result.kind)
LIVE_KINDS = {0: None, 1: "back-to-state", 2: "stuttering"}


# the fairness condition a liveness check assumes (kc_live_config.fairness = the index)
FAIRNESS = ("next", "process")


class KcLiveConfig(C.Structure):
    _fields_ = [("property", C.c_int), ("max_states", C.c_uint64), ("fairness", C.c_int)]


class KcLiveResult(C.Structure):
    _fields_ = [("states", C.c_uint64), ("edges", C.c_uint64), ("init", C.c_uint64), ("depth", C.c_int),
                ("stay_states", C.c_uint64), ("live_states", C.c_uint64), ("live_terminal", C.c_uint64),
                ("rounds", C.c_uint64),
                ("err_kind", C.c_int), ("err_action", C.c_int), ("err_self", C.c_int),
                ("violated", C.c_int), ("kind", C.c_int), ("prefix_len", C.c_int),
                ("trace_len", C.c_int), ("loop_start", C.c_int),
                ("seconds", C.c_double), ("build_ms", C.c_double), ("trim_ms", C.c_double),
                ("sccs", C.c_uint64), ("fair_sccs", C.c_uint64), ("fair_states", C.c_uint64),
                ("scc_rounds", C.c_uint64), ("scc_ms", C.c_double)]


class KcSqueueConfig(C.Structure):
    _fields_ = [
        ("state_words", C.c_int), ("device", C.c_int), ("segment_states", C.c_uint64),
        ("hbm_bytes", C.c_uint64), ("host_bytes", C.c_uint64), ("spill_dir", C.c_char_p),
    ]


class KcSqueueStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "size", "segments", "seg_hbm", "seg_host", "seg_disk", "hbm_bytes", "host_bytes", "disk_bytes",
        "spilled_host_bytes", "spilled_disk_bytes", "reloaded_bytes", "peak_hbm_bytes")]


# (name, restype, argtypes) for every symbol of include/kubecheck.h
_P = C.c_void_p
_U64P = C.POINTER(C.c_uint64)

# kc_host_comm: the caller's collectives for kc_group_create_host
HC_ALL_GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64))
HC_EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_void_p, C.c_void_p)
HC_BROADCAST = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint64))
HC_ALL_REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64)


class KcHostComm(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("all_gather", HC_ALL_GATHER), ("exchange", HC_EXCHANGE),
                ("broadcast", HC_BROADCAST), ("all_reduce_sum", HC_ALL_REDUCE)]

_U8P = C.POINTER(C.c_uint8)
_IP = C.POINTER(C.c_int)
SIGNATURES = [
    ("kc_last_error", C.c_char_p, []),
    ("kc_abi_version", C.c_int, []),
    ("kc_build_info", C.c_char_p, []),
    ("kc_device_count", C.c_int, []),
    ("kc_fpset_create", C.c_int, [C.c_uint64, C.c_int, C.POINTER(_P)]),
    ("kc_fpset_destroy", None, [_P]),
    ("kc_fpset_put_batch", C.c_int, [_P, _U64P, C.c_size_t, _U8P]),
    ("kc_fpset_contains_batch", C.c_int, [_P, _U64P, C.c_size_t, _U8P]),
    ("kc_fpset_put_batch_dev", C.c_int, [_P, _P, C.c_size_t, _P, _P]),
    ("kc_fpset_contains_batch_dev", C.c_int, [_P, _P, C.c_size_t, _P, _P]),
    ("kc_fpset_size", C.c_uint64, [_P]),
    ("kc_fpset_capacity", C.c_uint64, [_P]),
    ("kc_fpset_check_fps", C.c_int, [_P, _U64P, C.POINTER(C.c_double)]),
    ("kc_fpset_stress", C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), _U64P]),
    ("kc_fpset_put", C.c_int, [_P, C.c_uint64, _IP]),
    ("kc_fpset_contains", C.c_int, [_P, C.c_uint64, _IP]),
    ("kc_fpset_combine_rounds", C.c_uint64, [_P]),
    ("kc_fpset_insert_count_dev", C.c_int, [_P, _P, C.c_size_t, _U64P, _P]),
    ("kc_fpset_contains_count_dev", C.c_int, [_P, _P, C.c_size_t, _U64P, _P]),
    ("kc_fpset_partition_dev", C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, _U64P, _P]),
    ("kc_stress_fps_dev", C.c_int, [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P]),
    ("kc_stress_fp", C.c_uint64, [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64]),
    ("kc_squeue_create", C.c_int, [C.c_int, C.c_uint64, C.c_int, C.POINTER(_P)]),
    ("kc_squeue_create2", C.c_int, [C.POINTER(KcSqueueConfig), C.POINTER(_P)]),
    ("kc_squeue_enqueue_dev", C.c_int, [_P, _P, C.c_size_t, _P]),
    ("kc_squeue_dequeue_dev", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    ("kc_squeue_reserve_dev", C.c_int, [_P, C.c_size_t, C.POINTER(_P), _P]),
    ("kc_squeue_commit", C.c_int, [_P, C.c_size_t, _P]),
    ("kc_squeue_front_dev", C.c_int, [_P, C.c_size_t, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_size_t), _P]),
    ("kc_squeue_pop", C.c_int, [_P, C.c_size_t, _P]),
    ("kc_squeue_peek", C.c_int, [_P, C.c_size_t, C.c_size_t, _U64P, _P]),
    ("kc_squeue_get_stats", C.c_int, [_P, C.POINTER(KcSqueueStats)]),
    ("kc_squeue_destroy", None, [_P]),
    ("kc_squeue_enqueue", C.c_int, [_P, _U64P, C.c_size_t]),
    ("kc_squeue_dequeue", C.c_int, [_P, _U64P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("kc_squeue_size", C.c_uint64, [_P]),
    ("kc_model_config_default", None, [C.POINTER(KcModelConfig)]),
    ("kc_engine_create", C.c_int, [C.POINTER(KcModelConfig), C.POINTER(_P)]),
    ("kc_engine_destroy", None, [_P]),
    ("kc_engine_run", C.c_int, [_P, C.POINTER(KcResult)]),
    ("kc_engine_trace_text", C.c_size_t, [_P, C.c_char_p, C.c_size_t]),
    ("kc_engine_trace_tuple", C.c_int, [_P, C.c_int, _U64P]),
    ("kc_engine_level_tuples", C.c_int64, [_P, C.c_int, _U64P, C.c_uint64]),
    ("kc_engine_capture_level", C.c_int, [_P, C.c_int]),
    ("kc_engine_set_coverage", C.c_int, [_P, C.c_int]),
    ("kc_engine_coverage", C.c_int, [_P, _U64P, C.c_int]),
    ("kc_engine_set_invariants", C.c_int, [_P, _U64P, C.c_int]),
    ("kc_engine_invariant_stats", C.c_int, [_P, _U64P, C.c_int]),
    ("kc_engine_kernel_times", C.c_int, [_P, C.POINTER(C.c_double), _U64P]),
    ("kc_engine_narrow_times", C.c_int, [_P, C.POINTER(C.c_double), _U64P, _U64P]),
    ("kc_engine_check_fps", C.c_int, [_P, _U64P, C.POINTER(C.c_double)]),
    ("kc_checkpoint_info", C.c_int, [C.c_char_p, C.POINTER(KcCheckpointInfo)]),
    ("kc_engine_checkpoint", C.c_int, [_P, C.c_char_p]),
    ("kc_engine_set_checkpoint", C.c_int, [_P, C.POINTER(KcCheckpointOptions)]),
    ("kc_engine_recover", C.c_int, [_P, C.c_char_p]),
    ("kc_ckpt_selftest", C.c_int, [C.c_int, C.c_int, C.c_uint64, _U64P, C.c_uint64, C.c_uint64, C.c_uint64, _U64P,
                                   _U64P]),
    ("kc_shard_create", C.c_int, [C.POINTER(KcModelConfig), C.c_int, C.c_int, C.POINTER(_P)]),
    ("kc_shard_destroy", None, [_P]),
    ("kc_shard_init", C.c_int, [_P, _U64P]),
    ("kc_shard_init_error", C.c_int, [_P, _U64P]),
    ("kc_shard_set_stream", C.c_int, [_P, _P]),
    ("kc_shard_expand", C.c_int, [_P, _U64P, _U64P]),
    ("kc_shard_record_bytes", C.c_uint64, [_P]),
    ("kc_shard_pack", C.c_int, [_P, _P]),
    ("kc_shard_insert", C.c_int, [_P, _P, C.c_uint64, _U64P, _U64P]),
    ("kc_shard_advance", C.c_int, [_P]),
    ("kc_shard_parent_key", C.c_int, [_P, C.c_int, C.c_uint64, _U64P]),
    ("kc_shard_frontier_tuple", C.c_int, [_P, C.c_uint64, _U64P]),
    ("kc_shard_result", C.c_int, [_P, C.POINTER(KcResult)]),
    ("kc_shard_claim_times", C.c_int, [_P, C.POINTER(C.c_double), _U64P, _U64P]),
    ("kc_shard_owner", C.c_int, [C.c_uint64, C.c_int]),
    ("kc_rccl_unique_id", C.c_int, [C.c_char_p]),
    ("kc_group_create_rccl", C.c_int, [_P, C.c_char_p, C.POINTER(_P)]),
    ("kc_group_create_local", C.c_int, [C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    ("kc_group_create_host", C.c_int, [_P, C.POINTER(KcHostComm), C.POINTER(_P)]),
    ("kc_group_destroy", None, [_P]),
    ("kc_group_run", C.c_int, [_P, C.POINTER(KcResult)]),
    ("kc_group_trace_tuple", C.c_int, [_P, C.c_int, _U64P]),
    ("kc_group_records_sent", C.c_uint64, [_P]),
    ("kc_exchange_plan", C.c_int, [C.c_int, C.c_int, _U64P, C.c_uint64, _U64P, C.c_int]),
    ("kc_cold_find_selftest", C.c_int64, [C.c_uint64, C.c_uint64]),
    ("kc_cold_find_keys_selftest", C.c_int, [_U64P, C.c_uint64, _U64P, C.c_uint64, C.c_uint64, _U8P]),
    ("kc_cold_key_selftest", C.c_int, [_U64P, _U64P, C.c_uint64, C.c_int, C.c_int]),
    ("kc_coldset_create", C.c_int, [C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.POINTER(_P)]),
    ("kc_coldset_add_run", C.c_int, [_P, _U64P, C.c_uint64]),
    ("kc_coldset_probe", C.c_int, [_P, _U64P, C.c_uint64, _U8P, _U64P]),
    ("kc_coldset_stats", C.c_int, [_P, _U64P]),
    ("kc_coldset_all_keys", C.c_int64, [_P, _U64P, C.c_uint64]),
    ("kc_coldset_clear", C.c_int, [_P]),
    ("kc_coldset_destroy", None, [_P]),
    ("kc_spill_selftest", C.c_int, [C.c_int, C.c_int, _U64P, C.c_uint64, _U64P, C.c_uint64, _U64P, C.c_uint64,
                                    C.c_uint64, _U64P, C.c_uint64, _U64P]),
    ("kc_emit_selftest", C.c_int, [C.c_int, C.POINTER(KcModelConfig), _U64P, C.c_uint64, _U64P, C.c_uint64, _U64P,
                                   C.c_uint64, _U64P, C.c_uint64, _U64P, C.c_uint64]),
    ("kc_claim_selftest", C.c_int, [C.c_int, C.POINTER(KcModelConfig), _U64P, C.c_uint64, _U64P, C.c_uint64, _U64P,
                                    C.c_uint64, _U64P, C.c_uint64, _U64P, C.c_uint64, _U64P, C.c_uint64]),
    ("kc_shard_selftest", C.c_int, [C.c_int, C.POINTER(KcModelConfig), _U64P, C.c_uint64, _U64P, C.c_uint64, _U64P,
                                    C.c_uint64, _U64P, C.c_uint64, _U64P, C.c_uint64, _U64P, C.c_uint64]),
    ("kc_probe_selftest", C.c_int, [C.c_int, C.c_uint64, _U64P, _U64P, C.c_uint64, C.c_uint32, C.c_int, _U64P,
                           _U64P, _U64P]),
    ("kc_sim_create", C.c_int, [C.POINTER(KcModelConfig), C.POINTER(KcSimConfig), C.POINTER(_P)]),
    ("kc_sim_destroy", None, [_P]),
    ("kc_sim_run", C.c_int, [_P, C.POINTER(KcSimResult)]),
    ("kc_sim_walks", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _U64P]),
    ("kc_sim_trace", C.c_int, [_P, C.c_uint64, _U64P, _IP, C.c_int]),
    ("kc_sim_trace_text", C.c_int64, [_P, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("kc_sim_rand", C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64]),
    ("kc_sim_pick", C.c_uint64, [C.c_uint64, C.c_uint64]),
    ("kc_sim_replay", C.c_int, [C.POINTER(KcModelConfig), C.c_uint64, C.c_int, C.c_uint64, _U64P, _IP, C.c_int,
                                _IP]),
    ("kc_live_create", C.c_int, [C.POINTER(KcModelConfig), C.POINTER(KcLiveConfig), C.POINTER(_P)]),
    ("kc_live_destroy", None, [_P]),
    ("kc_live_run", C.c_int, [_P, C.POINTER(KcLiveResult)]),
    ("kc_live_create_formula", C.c_int, [C.POINTER(KcModelConfig), C.POINTER(KcLiveConfig), C.c_int, _U64P, C.c_int,
                                         C.POINTER(_P)]),
    ("kc_live_set_formula", C.c_int, [_P, C.c_int, _U64P, C.c_int]),
    ("kc_live_trigger_counts", C.c_int, [_P, _U64P, _U64P]),
    ("kc_live_mark_selftest", C.c_int, [_U64P, C.c_uint64, _U64P, C.c_int, _U64P, _U64P, _U64P, C.c_uint64, _U64P, _U64P,
                                        _U64P, C.c_uint64, _U64P, C.c_uint64]),
    ("kc_live_trace", C.c_int, [_P, _U64P, _IP, C.c_int]),
    ("kc_live_trace_text", C.c_int64, [_P, C.c_char_p, C.c_size_t]),
    ("kc_live_alive", C.c_int, [_P, _U64P, _U8P, C.c_uint64]),
    ("kc_live_stay", C.c_int, [C.POINTER(KcModelConfig), C.c_int, _U64P]),
    ("kc_live_edge_procs", C.c_int64, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _U8P, C.c_uint64]),
    ("kc_live_step_process", C.c_int, [C.POINTER(KcModelConfig), _U64P, C.c_int]),
    ("kc_live_selftest", C.c_int, [_U64P, C.c_uint64, _U64P, _U64P, C.c_uint64, _U64P, _U64P, _U64P, _U64P, _U64P,
                                   C.c_uint64, _U64P, C.c_uint64]),
    ("kc_spec_tuple_words", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("kc_spec_state_words", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("kc_spec_init", C.c_int, [C.POINTER(KcModelConfig), _U64P, C.c_int]),
    ("kc_spec_successors", C.c_int, [C.POINTER(KcModelConfig), _U64P, _IP, _U64P, C.c_int, _IP]),
    ("kc_spec_check", C.c_int, [C.POINTER(KcModelConfig), _U64P]),
    ("kc_spec_cover", C.c_int, [C.POINTER(KcModelConfig), _U64P, C.c_uint64, _U64P]),
    ("kc_pred_eval", C.c_int, [C.POINTER(KcModelConfig), _U64P, C.c_int, _U64P]),
    ("kc_pred_selftest", C.c_int, [C.c_int, _U64P, C.c_int, _U64P, C.c_uint64, C.c_uint64, _U64P, C.c_uint64]),
    ("kc_cover_count", C.c_int, []),
    ("kc_cover_name", C.c_char_p, [C.c_int]),
    ("kc_spec_fingerprint", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P]),
    ("kc_spec_fingerprint_own", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P]),
    ("kc_spec_fp_selfcheck", C.c_int, [C.POINTER(KcModelConfig), _U64P]),
    ("kc_spec_permute", C.c_int, [C.POINTER(KcModelConfig), _U64P, _IP, _U64P]),
    ("kc_spec_fingerprint_sym", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P]),
    ("kc_sym_selftest_fps", C.c_int, [C.POINTER(KcModelConfig), _U64P, C.c_uint64, _U64P]),
    ("kc_spec_in_model", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P, C.c_int]),
    ("kc_con_selftest", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P, _IP, C.c_uint64, _IP]),
    ("kc_engine_instantiation", C.c_int, [_P]),
    ("kc_spec_step_violations", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P, C.c_int]),
    ("kc_act_selftest", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P, _IP, C.c_uint64, _IP]),
    ("kc_spec_pack", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P]),
    ("kc_spec_unpack", C.c_int, [C.POINTER(KcModelConfig), _U64P, _U64P]),
]

_lib = None


class KubecheckError(RuntimeError):
    def __init__(self, func: str, code: int, msg: str):
        super().__init__(f"{func} failed ({code}): {msg}")
        self.code = code


def load() -> C.CDLL:
    """Load libkubecheck.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 and
    # cannot initialise on top of /opt/rocm's if that one is loaded first, so
    # when torch is installed it is loaded before libkubecheck (whose
    # libamdhip64.so.7 dependency then resolves to the already-loaded copy).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libkubecheck.so not found at {LIB_PATH}; build it with "
            "`make -C tla-kubernetes_amd/csrc` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def build_id() -> str:
    """A digest of the HIP sources libkubecheck.so is built from (csrc/*.hip,
    *.h and the C-ABI header).  Profiles record it (tools/pmc_summary.py), so
    a bench line uses a committed PMC figure as a measurement only when it
    was taken on the kernels of this build."""
    import hashlib
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
    hdr = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include", "kubecheck.h")
    h = hashlib.sha1()
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))) if os.path.isdir(csrc) else []
    for f in [os.path.join(csrc, f) for f in files] + [hdr]:
        try:
            with open(f, "rb") as fh:
                h.update(os.path.basename(f).encode() + b"\0" + fh.read())
        except OSError:
            pass
    return h.hexdigest()[:16]


def check(func: str, rc: int) -> int:
    if rc < 0:
        msg = load().kc_last_error()
        raise KubecheckError(func, rc, msg.decode() if msg else "")
    return rc
