/*
 * kubecheck.h — C ABI of libkubecheck.so, the MI355X-native BFS model
 * checker for KubeAPI.tla (JohnStrunk/tla-kubernetes).
 *
 * Plain C, plain pointers and sizes; no torch, no C++ types.  Every entry
 * point returns 0 on success or a negative errno-style code (-EINVAL bad
 * argument, -ENOMEM device memory / table full, -EIO HIP failure, -ENODEV
 * no GPU) and leaves a thread-local message for kc_last_error().  Nothing
 * aborts and nothing throws across this boundary.
 *
 * What each group replaces in the reference's hot path.  The reference's
 * checker is TLC 2.16 (tla2tools.jar, rev cdddf55; KubeAPI.toolbox/Model_1/
 * MC.out:2), a third-party Java jar not vendored in the reference; its
 * plugin seams are named in the recorded run's banner (MC.out:5:
 * "OffHeapDiskFPSet, DiskStateQueue") and selected by TLC system properties
 * [ext-TLC].  INTEGRATION.md shows the Java (Panama FFM) binding a TLC
 * maintainer would add over these symbols.
 *
 *   kc_fpset_*   tlc2.tool.fp.FPSet (abstract class; impl chosen by
 *                -Dtlc2.tool.fp.FPSet.impl=<class>):
 *                  put(long fp)      -> boolean "was already present"
 *                  contains(long fp) -> boolean
 *                  size()            -> long
 *                  checkFPs()        -> double (collision estimate, MC.out:42)
 *                  init/close        -> create/destroy
 *                Batched: TLC's put() is per-state; the shim batches puts
 *                from all -workers threads (flat combining).  Within one
 *                batch, equal fps resolve exactly as sequential puts would:
 *                the lowest index gets seen=0, every later one seen=1.
 *                Fingerprints are normalised like TLC's disk FPSets: the
 *                MSB is ignored and 0 is mapped to 1 (documented merge).
 *   kc_squeue_*  tlc2.tool.queue.StateQueue (MC.out:5 "DiskStateQueue"):
 *                FIFO of packed states in HBM (enqueue/dequeue batches).
 *   kc_engine_*  tlc2.TLC's BFS ModelChecker run over Model_1-style inputs
 *                (MC.cfg:1-16, MC.tla:1-16, KubeAPI___Model_1.launch):
 *                counts, depth, per-action coverage and counterexamples.
 *   kc_sim_*     tlc2.TLC -simulate: bounded random behaviours checked
 *                against the same invariants, Asserts and deadlock (the
 *                reference holds no simulation run; semantics below).
 *   kc_live_*    tlc2.TLC's liveness check of the spec's temporal properties
 *                under WF_vars(Next) or per-process weak fairness (the
 *                reference holds no liveness output; semantics below).
 *   kc_spec_*    host-side access to the lowered spec (canonical tuples) —
 *                used for trace replay and by the parity tests.
 */
#ifndef KUBECHECK_H
#define KUBECHECK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KC_ABI_VERSION 1
#define KC_NACTIONS 22
#define KC_MAX_LEVELS 4096

/* ------------------------------------------------------------------ misc */
/* Thread-local description of the last failure on this thread. */
const char *kc_last_error(void);
/* ABI version (KC_ABI_VERSION) and build string. */
int kc_abi_version(void);
const char *kc_build_info(void);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int kc_device_count(void);

/* ---------------------------------------------------------------- FPSet */
typedef struct kc_fpset kc_fpset;

/* Create a set able to hold `capacity_fps` fingerprints at <= 75% load
 * (rounded up to whole 64-B buckets); it grows (rehash) when a batch would
 * push it past 75%.  `device` is a HIP device ordinal. */
int kc_fpset_create(uint64_t capacity_fps, int device, kc_fpset **out);
void kc_fpset_destroy(kc_fpset *s);
/* put: seen_out[i] = 1 iff fps[i] was already present (TLC FPSet.put). */
int kc_fpset_put_batch(kc_fpset *s, const uint64_t *fps, size_t n, uint8_t *seen_out);
/* contains: seen_out[i] = 1 iff present (TLC FPSet.contains). */
int kc_fpset_contains_batch(kc_fpset *s, const uint64_t *fps, size_t n, uint8_t *seen_out);
/* Device-pointer variants (HBM in and out, asynchronous on `hip_stream`,
 * which may be NULL for the handle's own stream; that stream is a blocking
 * one, ordered with the legacy default stream).  fps_dev may be rewritten
 * (normalised in place). */
int kc_fpset_put_batch_dev(kc_fpset *s, uint64_t *fps_dev, size_t n, uint8_t *seen_dev,
                           void *hip_stream);
int kc_fpset_contains_batch_dev(kc_fpset *s, uint64_t *fps_dev, size_t n, uint8_t *seen_dev,
                                void *hip_stream);
/* Distinct fingerprints stored. */
uint64_t kc_fpset_size(const kc_fpset *s);
/* Slot capacity (u64 fingerprint slots, linear probing). */
uint64_t kc_fpset_capacity(const kc_fpset *s);
/* TLC checkFPs(): the minimum gap between any two stored fingerprints
 * (sorted), from which TLC derives "based on the actual fingerprints"
 * (MC.out:42).  *prob_out = 1/min_gap (TLC's estimate). */
int kc_fpset_check_fps(kc_fpset *s, uint64_t *min_gap_out, double *prob_out);
/* Single-fingerprint put/contains, safe from many host threads at once
 * (TLC's -workers threads each call FPSet.put(long); MC.out:5 "4 workers").
 * Concurrent calls are flat-combined: one caller launches every pending
 * request as one batch (arrival order = sequential put order) while the
 * others wait for their result.  *seen_out = 1 iff already present. */
int kc_fpset_put(kc_fpset *s, uint64_t fp, int *seen_out);
int kc_fpset_contains(kc_fpset *s, uint64_t fp, int *seen_out);
/* Number of combined batches launched by kc_fpset_put/contains so far. */
uint64_t kc_fpset_combine_rounds(const kc_fpset *s);
/* Bulk insert / lookup of device-resident fingerprints without per-fp
 * results (a sharded or streaming caller that only needs the totals):
 * *n_new_out = fps newly inserted, *found_out = fps present.  Synchronous. */
int kc_fpset_insert_count_dev(kc_fpset *s, const uint64_t *fps_dev, size_t n, uint64_t *n_new_out,
                              void *hip_stream);
int kc_fpset_contains_count_dev(kc_fpset *s, const uint64_t *fps_dev, size_t n, uint64_t *found_out,
                                void *hip_stream);
/* Fingerprint-owner routing of a batch (multi-GPU FPSet): stable counting
 * sort of fps_dev by owner rank floor(fp * world / 2^63) (after the MSB/0
 * normalisation) into out_dev; counts_out[r] = fps for rank r (host array of
 * `world` entries, 1 <= world <= 16).  Synchronous. */
int kc_fpset_partition_dev(kc_fpset *s, const uint64_t *fps_dev, uint64_t n, int world,
                           uint64_t *out_dev, uint64_t *counts_out, void *hip_stream);
/* Synthetic stress, fingerprints generated on device:
 * insert stream i -> perm63(seed + i) for i in [0, n) (perm63 a bijection of
 * [0, 2^63), so the n fps are distinct and normalised), in batches of
 * `batch`; then n_lookup lookups, entry j present for even j and absent for
 * odd j.  So size() grows by exactly n and *found_out = ceil(n_lookup / 2).
 * Needs 1 <= seed and seed + n + n_lookup < 2^63.  Device times in seconds. */
int kc_fpset_stress(kc_fpset *s, uint64_t seed, uint64_t n, uint64_t batch,
                    uint64_t n_lookup, double *insert_seconds, double *lookup_seconds,
                    uint64_t *found_out);
/* The same streams written to device memory: kind 0 = insert stream entries
 * [start, start + n); kind 1 = lookup stream entries (n_ins = the insert
 * stream's length).  Asynchronous on hip_stream. */
int kc_stress_fps_dev(uint64_t seed, int kind, uint64_t n_ins, uint64_t start, uint64_t n,
                      uint64_t *out_dev, void *hip_stream);
/* Host copy of one stream entry (tests). */
uint64_t kc_stress_fp(uint64_t seed, int kind, uint64_t n_ins, uint64_t i);

/* ----------------------------------------------------------- StateQueue */
typedef struct kc_squeue kc_squeue;
/* FIFO of fixed-width packed states (words per state = `state_words`) in
 * segments over three tiers: HBM, pinned host RAM beyond `hbm_bytes`, and
 * spill files in `spill_dir` beyond `host_bytes` (DiskStateQueue's role).
 * The tail segment is always in HBM; a spilled segment comes back to HBM
 * when a reader reaches it.  The segments being read (front runs handed
 * out since the last pop) and written stay resident whatever the budget.
 * Every call takes a HIP stream (NULL = the queue's own blocking stream);
 * drive one queue from one stream: copies and kernels are then ordered
 * without events. */
typedef struct {
  int state_words;
  int device;
  uint64_t segment_states;  /* states per segment (0 = 2^20) */
  uint64_t hbm_bytes;       /* HBM budget of the segments (0 = unlimited) */
  uint64_t host_bytes;      /* pinned host RAM budget (0 = unlimited) */
  const char *spill_dir;    /* disk tier (NULL = none: past both budgets -ENOMEM) */
} kc_squeue_config;
typedef struct {
  uint64_t size, segments, seg_hbm, seg_host, seg_disk;
  uint64_t hbm_bytes, host_bytes, disk_bytes;      /* now */
  uint64_t spilled_host_bytes, spilled_disk_bytes, reloaded_bytes, peak_hbm_bytes;  /* cumulative */
} kc_squeue_stats;
int kc_squeue_create2(const kc_squeue_config *cfg, kc_squeue **out);
/* one HBM tier of `capacity_states`-state segments, no budget (round-1 API);
 * capacity_states is also a hard bound on the queue's size: enqueue,
 * enqueue_dev and reserve_dev past it fail with -ENOMEM ("StateQueue full") */
int kc_squeue_create(int state_words, uint64_t capacity_states, int device, kc_squeue **out);
void kc_squeue_destroy(kc_squeue *q);
/* host buffers (synchronous) */
int kc_squeue_enqueue(kc_squeue *q, const uint64_t *states, size_t n);
/* dequeue up to `max_n` states into `out`; *n_out = number dequeued */
int kc_squeue_dequeue(kc_squeue *q, uint64_t *out, size_t max_n, size_t *n_out);
/* device buffers, stream-ordered (TLC's sEnqueue / sDequeue(n) batches) */
int kc_squeue_enqueue_dev(kc_squeue *q, const uint64_t *dev_states, size_t n, void *hip_stream);
int kc_squeue_dequeue_dev(kc_squeue *q, uint64_t *dev_out, size_t max_n, size_t *n_out, void *hip_stream);
/* In place: a device run of n states at the tail for a kernel to write,
 * valid until the next call; commit(k <= n) appends its first k states. */
int kc_squeue_reserve_dev(kc_squeue *q, size_t n, uint64_t **dev_ptr, void *hip_stream);
int kc_squeue_commit(kc_squeue *q, size_t n, void *hip_stream);
/* In place: a contiguous device run of up to max_n states starting `offset`
 * states after the head (*n_out may be smaller, at a segment end), valid
 * until it is popped; pop(n) drops n states from the head. */
int kc_squeue_front_dev(kc_squeue *q, size_t offset, size_t max_n, const uint64_t **dev_ptr,
                        size_t *n_out, void *hip_stream);
int kc_squeue_pop(kc_squeue *q, size_t n, void *hip_stream);
/* host copy of states [offset, offset + n) after the head, from any tier */
int kc_squeue_peek(kc_squeue *q, size_t offset, size_t n, uint64_t *host_out, void *hip_stream);
int kc_squeue_get_stats(kc_squeue *q, kc_squeue_stats *out);
uint64_t kc_squeue_size(const kc_squeue *q);

/* -------------------------------------------------------------- Engine */
typedef struct {
  int nc, np, ns;          /* clients, PVC controllers, API servers (Model_1: 1,1,1) */
  int can_fail;            /* REQUESTS_CAN_FAIL  (MC.tla:5-7) */
  int can_timeout;         /* REQUESTS_CAN_TIMEOUT (MC.tla:10-12) */
  int check_deadlock;      /* launch:16 */
  int variant;             /* 0 = KubeAPI.tla as written; seeded bugs: 1 = Update w/o
                              HasRead, 2 = Force w/o replace, 3 = C1 ignores the
                              reply status, 4 = list ignores kind, 5 = Init store
                              with two Secret versions (kubeapi_spec.h Flags) */
  int device;              /* HIP device ordinal */
  int keep_trace;          /* parent pointers (TLC's trace file); default 1 */
  int max_levels;          /* 0 = to completion */
  uint64_t fpset_slots;    /* initial FPSet slots; 0 = default */
  uint64_t chunk_states;   /* parents per expansion chunk; 0 = default */
  int verbose;             /* progress lines to stderr */
  int timing;              /* 1 = time every kernel launch with HIP events,
                              2 = only k_claim (the roofline kernel) */
  int invariants;          /* MC.cfg INVARIANT list: bit 0 TypeOK, bit 1
                              OnlyOneVersion (default 3; 0 = check none), bit 2
                              the build-defined NoLostUpdate (with its lostUpdate
                              history variable; models of <= 3 actors) */
  /* Frontier spill (single-GPU engine).  frontier_hbm_bytes > 0 keeps the
   * frontiers in a kc_squeue with that HBM budget: levels run in chunks of
   * <= frontier_segment_states parents, read from the queue's head and
   * written into its tail; segments past the budget go to pinned host RAM
   * (up to frontier_host_bytes, 0 = unlimited), then to files in spill_dir.
   * trace_host = 1 keeps the trace file (parent index + ordinal, 9 B per
   * state) in pinned host RAM instead of HBM. */
  uint64_t frontier_hbm_bytes;
  uint64_t frontier_host_bytes;
  uint64_t frontier_segment_states;   /* 0 = 2^22 */
  const char *spill_dir;
  int trace_host;
  /* Seen-set spill (single-GPU engine, and every rank of the sharded loop
   * for its own share of the fingerprints; TLC's OffHeapDiskFPSet role,
   * MC.out:5).  seen_hbm_bytes > 0 caps the HBM the seen-set uses: a fixed
   * hot ClaimSet (<= half of it), scratch, and the HBM directories and
   * filters of the cold tier.  When the hot table fills, its fingerprints are
   * flushed into sorted runs in pinned host RAM (up to seen_host_bytes,
   * 0 = unlimited), then in files in spill_dir; every level's new states are
   * checked against the runs on the GPU.  Results are identical to the
   * unbounded seen-set's. */
  uint64_t seen_hbm_bytes;
  uint64_t seen_host_bytes;
  /* Sharded loop at world > 1 (kc_group_*, kc_shard_*): 1 = claims ordered
   * by each parent's position in sequential-BFS order instead of (rank, local
   * index), so the first discoverer of every state, the error reported and
   * its trace are TLC -workers 1's (KubeAPI___Model_1.launch:4-7); costs a
   * per-level all-reduce of per-parent masks and a sort of each rank's new
   * frontier.  Counted levels only, with the deferred frontier; not with the
   * seen-set spill.  Ignored at world 1, where the order is TLC's anyway. */
  int tlc_order;
  /* 1 = the first inserter of a fingerprint owns it, as in a TLC -workers N
   * run (KubeAPI___Model_1.launch:33): no settle passes.  Counts, widths,
   * per-action generated counts, error kinds and levels and trace lengths are
   * unchanged; which same-level copy wins (its parent, the per-action
   * distinct split, which of several equal-level errors is reported) is not
   * deterministic.  Single-GPU engine: in-HBM wide levels only (ignored with
   * the seen-set spill or a frontier HBM budget; KC_FIRST_CLAIM=1 sets it
   * too).  Sharded loop (kc_shard_*, kc_group_*): every counted level, at any
   * world; kc_shard_create fails with -EINVAL together with tlc_order or the
   * seen-set spill.  kc_result.claim_mode reports what ran.  The seen-set
   * then holds 8-B fingerprint words (16-B {fp, claim} slots otherwise): the
   * same slot count and load in half the HBM, half the per-run clear. */
  int first_claim;
  /* Symmetry reduction (TLC's SYMMETRY): bit 0 = the
   * clients are interchangeable, bit 1 = the PVC controllers are; 0 = off.
   * The seen-set then holds one fingerprint per permutation orbit (the minimum
   * of the fingerprints of the state's permutations), so distinct, level_width
   * and act_dist count orbits; generated counts the successors of the states
   * expanded, one per orbit.  Frontier states, traces and counterexamples stay
   * real (unpermuted) states.  A bit whose process set has fewer than two
   * members is ignored; with no bit left the plain engine runs.  Single-GPU
   * engine only (frontier_hbm_bytes and seen_hbm_bytes included):
   * kc_engine_create fails with -EINVAL together with variant 5 when the group
   * moves actor 0 (that Init store names actor 0); kc_shard_create and kc_live_create fail
   * with -EINVAL (the owner projection is not orbit-invariant; liveness under
   * symmetry is unsound), and so does kc_sim_create. */
  int symmetry;
  /* Constraints (TLC's CONSTRAINT and ACTION_CONSTRAINT; DESIGN.md section
   * 4.11).  A successor x of an expanded state s is in the model iff every
   * state constraint holds in x and every action constraint holds on the step
   * s -> x (state constraints first).  A successor outside the model still
   * counts as generated; it is discarded without a seen-set lookup (not
   * distinct, not queued, no trace link), after its invariants were checked.
   * Deadlock is a property of Next alone; Init states outside a state
   * constraint are discarded.  The vocabulary is build-defined:
   *   constraint_stored   = k >= 0: StoredAtMost<k>, Cardinality(apiState) <= k
   *   constraint_inflight = k >= 0: InFlightAtMost<k>, Cardinality(PendingClients)
   *                         + Cardinality(PendingListClients) <= k
   *   action_constraints  bit 0: ServeClientsFirst, an APIStart step that takes
   *                         a PVC controller's request or list request out of
   *                         "Pending" only while no client's is pending
   * Negative bounds (kc_model_config_default sets -1) and mask 0 = off: then
   * nothing changes and the plain engine runs.  Single-GPU in-HBM BFS only:
   * kc_engine_create fails with -EINVAL together with symmetry,
   * seen_hbm_bytes, frontier_hbm_bytes or trace_host, with mask bits outside
   * bit 0, and for a model not built with constraints (built: (1,1,1),
   * (2,1,1), (1,2,1), (1,3,1)); kc_engine_set_coverage, kc_engine_checkpoint,
   * kc_engine_set_checkpoint and kc_engine_recover fail with -EINVAL on such
   * an engine; kc_shard_create (so every kc_group_*), kc_live_create and
   * kc_sim_create fail with -EINVAL. */
  int constraint_stored;
  int constraint_inflight;
  int action_constraints;
  /* Action properties (TLC's PROPERTY with a formula [][A]_vars, a step
   * invariant).  A is evaluated on every step
   * s -> x the BFS generates, x new or seen, before the seen-set lookup; a
   * step with x = s passes.  Init states are not steps.  The first level with
   * a violating step ends the run: err_kind 4, err_invariant = the property's
   * bit index, err_action / err_self = the step's, and the trace is the path
   * to s followed by x (trace_len = depth(s) + 1).  Of the errors of one
   * (parent, successor position) an invariant violation wins.  The level runs
   * to its end, so step_checked and step_violations[] count whole levels.
   * The vocabulary is build-defined:
   *   bit 0 NoBlindUpdate: every requests[c] that is an Update, "Pending" in
   *         s and "Ok" in x has a stored version of its object (unprimed
   *         apiState) that c has read (HasRead)
   *   bit 1 OneReplyPerStep: at most one requests[a] / listRequests[a] leaves
   *         "Pending" in the step
   *   bit 2 StoreNeverShrinks: Cardinality(apiState') >= Cardinality(apiState)
   * Mask 0 = off: then nothing changes and the plain engine runs.
   * Single-GPU in-HBM BFS only: kc_engine_create fails with -EINVAL together
   * with constraints, symmetry, seen_hbm_bytes, frontier_hbm_bytes or
   * trace_host, with mask bits outside 0..2, and for a model not built with
   * action properties (built: (1,1,1), (2,1,1), (1,2,1), (1,3,1));
   * kc_engine_set_coverage, kc_engine_checkpoint, kc_engine_set_checkpoint
   * and kc_engine_recover fail with -EINVAL on such an engine; kc_shard_create
   * (so every kc_group_*) and kc_sim_create fail with -EINVAL. */
  int action_properties;
} kc_model_config;

typedef struct {
  uint64_t init, generated, distinct, queue_left;
  int depth;               /* BFS levels, init = level 1 (TLC msg 2194) */
  int complete;
  uint64_t act_gen[KC_NACTIONS];
  uint64_t act_dist[KC_NACTIONS];
  int nlevels;
  uint64_t level_width[KC_MAX_LEVELS];
  int err_kind;            /* 0 none, 1 assertion, 2 invariant, 3 deadlock, 4 action property */
  int err_action;          /* action id (assertion; the violating step of an action property) */
  int err_self;            /* process index of the failing action */
  int err_invariant;       /* 0 TypeOK, 1 OnlyOneVersion, 2 NoLostUpdate; err_kind 4: the action
                            * property's bit index (0 NoBlindUpdate, 1 OneReplyPerStep, 2 StoreNeverShrinks) */
  int err_level;           /* BFS level of the last trace state */
  int trace_len;           /* states in the counterexample */
  double seconds;          /* wall time of the BFS (device work + host loop) */
  double collision_optimistic; /* TLC's calculated estimate d*(g-d)/2^64 */
  uint64_t fpset_slots;
  uint64_t peak_frontier;
  uint64_t fpset_probes;   /* FPSet insert probes (level-unique successors) */
  uint64_t batch_inserts;  /* batch-table inserts (= generated successors) */
  uint64_t levels_chunks;  /* expansion chunks over the whole run */
  uint64_t outdeg_hist[16]; /* TLC outdegree (msg 2268): expanded states by the number of
                              new states first reached from them; [15] = 15 or more
                              (single-GPU engine; zero in the sharded path) */
  uint64_t frontier_spilled_bytes;   /* frontier bytes written to host RAM or disk */
  uint64_t frontier_reloaded_bytes;  /* ... and read back into HBM */
  uint64_t frontier_peak_hbm_bytes;  /* peak HBM held by the frontier queue */
  /* seen-set spill (cfg.seen_hbm_bytes > 0) */
  uint64_t seen_flushes;        /* hot-table flushes into the cold tier */
  uint64_t seen_cold_fps;       /* fingerprints in cold runs at the end */
  uint64_t seen_cold_runs;      /* cold runs at the end (host + disk) */
  uint64_t seen_cold_queries;   /* new-to-the-hot-table fingerprints checked against the cold tier */
  uint64_t seen_cold_hits;      /* ... found there (states already seen) */
  uint64_t seen_merges;         /* run merges */
  uint64_t seen_filter_tests;   /* (query, run) pairs tested by a run's Bloom filter */
  uint64_t seen_filter_passed;  /* ... that the filter let through to the run */
  uint64_t seen_disk_bytes;     /* cold-run bytes written to spill files */
  uint64_t seen_peak_hbm_bytes; /* peak HBM of the seen-set (hot table + scratch + cold metadata) */
  double seen_seconds;          /* host wall time in chunk planning, flushes and cold checks */
  double seen_flush_seconds;    /* ... of it in flushes (sort, copy out, merges, files) */
  double seen_merge_seconds;    /* ... of that in the host merges of runs */
  double seen_check_seconds;    /* ... in the per-chunk cold checks (queries, sort, probe) */
  uint64_t cand_overflow_records;  /* settle candidates beyond their tile's segment (overflow list) */
  uint64_t cand_buffer_peak_bytes; /* HBM of the candidate-record buffers (tile segments + overflow list) */
  /* deferred frontier (the default wide path): states rebuilt from their
   * links inside k_claim (which then also writes them), and whether this run
   * was redone on the materialising path (an error or a capacity estimate
   * exceeded; the reported result is the redone run's) */
  uint64_t deferred_states;
  uint64_t defer_fallback;
  /* the level an exact redo of a deferred-frontier anomaly started from (the
   * anomaly's level; 1 = from Init), 0 if there was none */
  uint64_t defer_redo_level;
  /* levels run by a device-driven narrow path (single-GPU engine: k_nfinish;
   * sharded loop: the fixed-slot exchange levels, shard_narrow.h) */
  uint64_t narrow_levels;
  /* the claim protocol the wide (counted) levels ran with: 0 = the
   * sequential-BFS minimum key (TLC -workers 1's first discoverer on one GPU;
   * (rank, parent) order on shards), 1 = first inserter (cfg.first_claim),
   * 2 = TLC order on shards (cfg.tlc_order at world > 1) */
  int claim_mode;
  /* constraints: successors (and Init states) discarded by a state
   * constraint, and successors that passed those and were discarded by an
   * action constraint; both 0 without constraints */
  uint64_t cut_state;
  uint64_t cut_action;
  /* action properties: the steps evaluated (every generated successor:
   * generated - init) and the steps violating property k, summed over every
   * level up to and including the one whose parents made the first
   * violation; all 0 without action properties */
  uint64_t step_checked;
  uint64_t step_violations[3];
} kc_result;

typedef struct kc_engine kc_engine;
/* Fill a config with Model_1 defaults (1,1,1, both constants TRUE, deadlock on). */
void kc_model_config_default(kc_model_config *cfg);
int kc_engine_create(const kc_model_config *cfg, kc_engine **out);
void kc_engine_destroy(kc_engine *e);
/* Run BFS to completion (or error / max_levels). */
int kc_engine_run(kc_engine *e, kc_result *res);
/* Counterexample as TLC-style text ("State 1: ..."); returns bytes needed. */
size_t kc_engine_trace_text(kc_engine *e, char *buf, size_t cap);
/* Canonical tuple of trace state i (see kc_spec_tuple_words). */
int kc_engine_trace_tuple(kc_engine *e, int i, uint64_t *out);
/* Canonical tuples of the states of BFS level `level` (1-based) from the
 * last run's frontier buffers, if still resident (only the final level and
 * levels captured with kc_engine_capture_level).  Returns count or <0. */
int64_t kc_engine_level_tuples(kc_engine *e, int level, uint64_t *out, uint64_t cap_states);
/* Ask run() to keep a host copy of level `level`'s packed states. */
int kc_engine_capture_level(kc_engine *e, int level);
/* Expression-level coverage (TLC's -coverage).  With
 * coverage on, run() also sums kc_cover_count() base counters over every
 * state it expands (levels 1..max_levels-1 of a bounded run): one counting
 * kernel per level next to the engine's own, and one host sync per narrow
 * level.  Off (the default) the engine allocates and launches what it always
 * did.  -EINVAL for an engine under symmetry reduction (its states stand for
 * orbits) and with seen_hbm_bytes, frontier_hbm_bytes or trace_host. */
int kc_engine_set_coverage(kc_engine *e, int on);
/* The summed counters of the last run, in kc_cover_name order; returns the
 * number written (cap >= kc_cover_count()).  -EINVAL when coverage was off,
 * and after a run that ended in an error (TLC prints no coverage then). */
int kc_engine_coverage(kc_engine *e, uint64_t *out, int cap);
/* User-defined invariants.  `program` is n_instr 16-byte
 * instructions (two uint64_t each; the encoding is csrc/pred.h's, compiled by
 * kubecheck/pred.py): at most 128 instructions, 8 invariants, nesting depth
 * 32.  It takes effect from the next run; n_instr = 0 turns it off, and then
 * the engine allocates and launches what it always did.
 *
 * With a program set, run() evaluates every invariant on every state it
 * expands, Init states included (levels 1..max_levels-1 of a bounded run):
 * one kernel per chunk next to the engine's own, and one host sync per narrow
 * level.  The first level that holds a violating state ends the run once that
 * level's expansion is closed: err_kind = 2, err_invariant = 3 + k (k in the
 * order given), err_level = that level, and the trace is the parent chain of
 * the violating state with the smallest index in that level (of the
 * invariants that state violates, the smallest k is reported).  generated,
 * distinct and the level widths are whole-level numbers that include that
 * level's expansion.  A violation at level L comes before anything the
 * expansion of level L itself found (an Assert, a deadlock, a built-in
 * invariant violated by a level-L+1 state): TLC would have checked the
 * level-L state when it was generated.  In the deterministic claim mode a
 * level's index order is TLC's -workers 1 order, so the state and the trace
 * are TLC's; in first-claim mode the length is the same and the trace is a
 * real behaviour.
 *
 * -EINVAL, with the reason in kc_last_error: a bad program; an engine under
 * symmetry reduction; with constraints (TLC checks invariants on the
 * successors a constraint discards; they are never expanded, so evaluation on
 * expansion would miss them); with action properties; with coverage on; with
 * checkpoint or recover; with seen_hbm_bytes, frontier_hbm_bytes or
 * trace_host. */
int kc_engine_set_invariants(kc_engine *e, const uint64_t *program, int n_instr);
/* The last run's states evaluated, then the states violating each invariant
 * (all zero but for the level that ended the run); returns the number of
 * words written (1 + invariants).  -EINVAL with no program set or no run
 * since. */
int kc_engine_invariant_stats(kc_engine *e, uint64_t *out, int cap);
/* Per-kernel device timings of the last run (ms; needs cfg.timing=1, or 2
 * for expand alone):
 * expand, resolve, scan, emit; and the number of launches of each. */
int kc_engine_kernel_times(kc_engine *e, double *ms4, uint64_t *launches4);
/* The narrow-level kernel of the last run (frontiers <= 8192 states run as
 * whole levels inside one single-workgroup launch): its device time in ms
 * (with cfg.timing), launches, and the BFS levels it expanded. */
int kc_engine_narrow_times(kc_engine *e, double *ms, uint64_t *launches, uint64_t *levels);
/* TLC's checkFPs on the last run's seen-set ("based on the actual
 * fingerprints", MC.out:42): the minimum gap between sorted fingerprints;
 * *prob_out = 1/min_gap. */
int kc_engine_check_fps(kc_engine *e, uint64_t *min_gap_out, double *prob_out);

/* ---------------------------------------------------------- Checkpoint */
/* Checkpoint and recover (TLC's -checkpoint / -recover; DESIGN.md section
 * 4.10) for the single-GPU in-HBM engine: both claim modes, narrow and wide
 * levels, the deferred and the materialising frontier, with or without
 * keep_trace and symmetry.  Not with seen_hbm_bytes, frontier_hbm_bytes or
 * trace_host, not with coverage on (-EINVAL and a kc_last_error text), and
 * not for the sharded loop, simulation or liveness, which have no such calls.
 *
 * A checkpoint is the state at the top of a BFS level: that level's frontier,
 * the seen-set as bare fingerprints (old claim words are never read again, so
 * it restores into a table of any size and either slot layout), the
 * cumulative counters and, with keep_trace, the trace file.  A recovered run
 * reports cumulative results, as if it had never stopped.
 *
 * The file is DIR/checkpoint.kc, written as checkpoint.kc.tmp, fsynced and
 * renamed, so a writer that dies leaves the previous checkpoint intact.  It
 * holds little-endian u64 words: a header of 64 words, then the sections.
 *
 *   word  0      magic 0x54504B434542554B ("KUBECKPT" as bytes)
 *   word  1      format version (1)
 *   word  2      header length in words (64)
 *   word  3      file length in bytes
 *   words 4-13   nc, np, ns, can_fail, can_timeout, check_deadlock, variant,
 *                invariants, effective symmetry mask (bits whose process set
 *                has fewer than two members cleared), state_words
 *   word  14     keep_trace (0 / 1)
 *   word  15     claim mode that wrote it (kc_result.claim_mode; informational)
 *   words 16-20  level, level_gidx (states before this level), n (frontier
 *                width), cand (successors of the frontier, exact), cand_total
 *   words 21-24  init, distinct, nlevels, peak_frontier
 *   word  25     number of sections (5)
 *   words 26-45  per section {offset in bytes, length in bytes, sum, xor};
 *                all four 0 for a section the checkpoint does not carry
 *   words 46-61  0
 *   words 62-63  (sum, xor) of words 0-61
 *
 * A checksum is the pair (sum mod 2^64, xor) of the u64 words it covers.
 * Sections (offsets are multiples of 8, at or after byte 512, none overlapping):
 *   0 COUNTERS      level_width[nlevels], act_gen[22], act_dist[22],
 *                   outdeg_hist[16], fpset probes of the wide levels, settles,
 *                   candidate overflow records, fpset probes of the narrow levels
 *   1 FRONTIER      n x state_words packed states, in the engine's FIFO order
 *   2 FPS           `distinct` fingerprint words, in any order
 *   3 TRACE_PARENT  (level_gidx + n) x u64 parent index (~0 for an Init state);
 *                   with keep_trace only
 *   4 TRACE_ORD     (level_gidx + n) x u8 successor ordinal, zero-padded to a
 *                   multiple of 8 bytes; with keep_trace only
 * distinct = level_gidx + n, nlevels = level, and the level widths add up to
 * distinct with n the last. */
#define KC_CKPT_SECTIONS 5
/* (a struct tag, not a typedef: the function below has the same name) */
struct kc_checkpoint_info {
  uint64_t version, file_bytes;
  int nc, np, ns, can_fail, can_timeout, check_deadlock, variant, invariants;
  int symmetry;            /* the effective mask */
  int state_words, keep_trace, claim_mode;
  int level, nlevels;
  uint64_t level_gidx, n, cand, cand_total;
  uint64_t init, distinct, peak_frontier;
  uint64_t section_offset[KC_CKPT_SECTIONS], section_bytes[KC_CKPT_SECTIONS];
  uint64_t section_sum[KC_CKPT_SECTIONS], section_xor[KC_CKPT_SECTIONS];
};
typedef struct {
  const char *dir;
  int every_levels;        /* > 0: checkpoint at the top of level L when L - L0 is a positive
                              multiple of it (L0 = 1, or the recovered level) */
  double every_seconds;    /* > 0: ... or when this much wall time has passed since the last one */
  uint64_t stage_bytes;    /* pinned staging per buffer, two buffers; 0 = 64 MiB; >= 4096 */
} kc_checkpoint_options;
/* Read and fully validate DIR/checkpoint.kc on the host (no GPU): the header,
 * the section table and every section's checksum, streamed.  -ENOENT: no
 * file; -EINVAL: not a checkpoint (magic) or an unknown version; -EIO:
 * truncated, inconsistent, or failing a checksum. */
int kc_checkpoint_info(const char *dir, struct kc_checkpoint_info *out);
/* Write the state the last kc_engine_run left, when that run stopped at
 * max_levels with err_kind == 0 and queue_left > 0 (-EINVAL otherwise). */
int kc_engine_checkpoint(kc_engine *e, const char *dir);
/* Make kc_engine_run itself checkpoint at level tops (see the options); each
 * checkpoint replaces the one before.  A deferred frontier is materialised
 * first, which changes no result.  NULL = off: the engine then allocates and
 * launches exactly what it does without this call.  Also takes stage_bytes
 * for kc_engine_checkpoint and kc_engine_recover (dir may then be NULL with
 * both periods 0). */
int kc_engine_set_checkpoint(kc_engine *e, const kc_checkpoint_options *opt);
/* Validate DIR/checkpoint.kc against the engine's model and arm the next
 * kc_engine_run only: it starts at the checkpoint's level instead of Init
 * (max_levels keeps its absolute meaning); a later run starts from Init
 * again.  -EINVAL names the first model field that differs (an engine with
 * keep_trace = 1 cannot take a checkpoint without trace sections; the reverse
 * is fine); -EIO on a bad file.  The table is sized as the larger of
 * fpset_slots and what the engine's growth rule keeps for `distinct` entries.
 * The armed run fails with -EIO if a restored fingerprint is not new to the
 * table or a section uploaded to the device fails its checksum there. */
int kc_engine_recover(kc_engine *e, const char *dir);

/* --------------------------------------------------- Sharded (multi-GPU) */
/* Fingerprint-owner-sharded BFS, one process per GPU (replaces TLC's
 * single-host worker pool; TLC's own distributed mode is off in Model_1,
 * KubeAPI___Model_1.launch:4-7).  The caller drives the levels and does the
 * exchange between pack() and insert() (kubecheck/distributed.py: RCCL
 * all-to-all through torch.distributed).  owner(fp) = floor(fp*R/2^63).
 * Per level:  expand -> pack(send) -> [all-to-all] -> insert(recv) ->
 * [all-reduce of new counts / error keys] -> advance.
 * Keys (records and errors): rank<<60 | parent index<<16 | successor<<8 |
 * low byte (action id in records; 1 assertion, 2 invariant, 3 deadlock,
 * 0x12 invariant violated by an Init state in error keys). */
typedef struct kc_shard kc_shard;
int kc_shard_create(const kc_model_config *cfg, int rank, int world, kc_shard **out);
void kc_shard_destroy(kc_shard *s);
/* Adopt (insert + enqueue) the Init states this rank owns. */
int kc_shard_init(kc_shard *s, uint64_t *n_local);
/* After kc_shard_init: the error key (low byte 0x12) of this rank's first
 * Init state that violates an invariant, ~0 if none.  It is level 1's error
 * and takes precedence over anything level 1's expansion reports. */
int kc_shard_init_error(kc_shard *s, uint64_t *key_out);
/* Run every stage on the caller's HIP stream (e.g. the one its RCCL
 * collectives use) instead of the shard's own: pack() then returns without a
 * host sync and insert() may read a recv buffer written earlier on that
 * stream (NULL = the default stream).  Call before kc_shard_init. */
int kc_shard_set_stream(kc_shard *s, void *hip_stream);
/* Expand the frontier: claim the successors this rank owns in place;
 * counts_out[r] = records destined to rank r (world entries, 0 for this
 * rank); *err_key_out = this rank's min Assert/deadlock key or ~0. */
int kc_shard_expand(kc_shard *s, uint64_t *counts_out, uint64_t *err_key_out);
/* Bytes per record: the state's canonical words and the key, padded to 16 B
 * (the receiver recomputes the fingerprint). */
uint64_t kc_shard_record_bytes(kc_shard *s);
/* Write sum(counts) records, grouped by owner rank, into device memory
 * (complete on return unless a caller stream was set). */
int kc_shard_pack(kc_shard *s, void *send_dev);
/* Dedup + insert `n_records` received records (device memory, grouped by
 * source rank) together with this rank's own claims of the level;
 * *n_new = states added to this rank's next frontier.  Without a caller
 * stream the library reads recv_dev on its own HIP stream: the caller must
 * have completed every write to it (e.g. synchronised its all-to-all). */
int kc_shard_insert(kc_shard *s, const void *recv_dev, uint64_t n_records, uint64_t *n_new,
                    uint64_t *err_key_out);
/* The new states become the frontier (after the caller's agreement step). */
int kc_shard_advance(kc_shard *s);
/* Parent key of local state `idx` of BFS level `level` (trace walk-back). */
int kc_shard_parent_key(kc_shard *s, int level, uint64_t idx, uint64_t *key_out);
/* Canonical tuple of current-frontier state `idx`. */
int kc_shard_frontier_tuple(kc_shard *s, uint64_t idx, uint64_t *out);
/* This rank's counters: act_gen (its parents), act_dist (its new states),
 * generated, distinct (owned), fpset_slots. */
int kc_shard_result(kc_shard *s, kc_result *res);
/* k_claim device time in ms (HIP events; needs cfg.timing != 0), launches
 * and parents expanded since the previous call (counters reset on read). */
int kc_shard_claim_times(kc_shard *s, double *ms, uint64_t *launches, uint64_t *parents);
/* owner rank of a fingerprint */
int kc_shard_owner(uint64_t fp, int world);

/* ------------------------------------------- Native sharded level loop */
/* The whole level-synchronous sharded BFS in C++ (the protocol above, with
 * one all-gather and one all-to-all per level and no caller in the loop).
 * A group is the set of shards one process drives plus their collectives:
 *   - kc_group_create_rccl: one shard per process (one process per GPU) and
 *     an RCCL communicator; every rank passes the same 128-byte id, made by
 *     kc_rccl_unique_id on one rank and sent to the others by the caller
 *     (e.g. a torch.distributed broadcast).  RCCL is loaded at run time.
 *   - kc_group_create_local: ranks 0..n-1 of one process on one GPU, the
 *     collectives done by device copies (multi-rank emulation, tests).
 * kc_group_run fills the GLOBAL result (the same on every rank): totals,
 * per-action counts, level widths, depth, and any error with its trace. */
#define KC_RCCL_ID_BYTES 128
typedef struct kc_group kc_group;
int kc_rccl_unique_id(uint8_t *id_out /* KC_RCCL_ID_BYTES */);
int kc_group_create_rccl(kc_shard *s, const uint8_t *id, kc_group **out);
int kc_group_create_local(kc_shard **shards, int nshards, kc_group **out);
/* One shard per process with the caller's own transport (MPI, gloo,
 * sockets) instead of RCCL: the loop calls these on host buffers, from the
 * thread that called kc_group_run; each returns 0 or < 0 (the run then fails
 * with -EIO on every rank that sees it; like RCCL's, a transport failure on
 * one rank only is the transport's to surface).  Every rank makes the same
 * sequence of calls.
 *   all_gather:     out[r * n + k] = rank r's in[k]  (n words)
 *   exchange:       this rank's all-to-all as kc_exchange_plan lists it, in
 *                   BYTES: xfers[4k..4k+3] = peer, 1 send / 0 receive, byte
 *                   offset into sendbuf / recvbuf, bytes; post all of them,
 *                   then wait (the k-th send from s to d pairs with the k-th
 *                   receive at d from s)
 *   broadcast:      *v from rank `root` to every rank
 *   all_reduce_sum: v[0..n) summed over ranks, in place
 * kubecheck.distributed.GlooHostComm implements it over torch.distributed. */
typedef struct kc_host_comm {
  void *ctx;
  int (*all_gather)(void *ctx, const uint64_t *in, uint64_t n, uint64_t *out);
  int (*exchange)(void *ctx, const uint64_t *xfers, int nxfers, const void *sendbuf, void *recvbuf);
  int (*broadcast)(void *ctx, int root, uint64_t *v);
  int (*all_reduce_sum)(void *ctx, uint64_t *v, uint64_t n);
} kc_host_comm;
int kc_group_create_host(kc_shard *s, const kc_host_comm *comm, kc_group **out);
void kc_group_destroy(kc_group *g);
int kc_group_run(kc_group *g, kc_result *res);
/* Canonical tuple of trace state i of the last run's error; returns words. */
int kc_group_trace_tuple(kc_group *g, int i, uint64_t *out);
/* Records this group's ranks sent to other ranks in the last run (global). */
uint64_t kc_group_records_sent(const kc_group *g);
/* The all-to-all of rank `me` as issued to RCCL (and replayed by the
 * one-process emulation): for each peer in rank order, its sends then its
 * receives, each cut into pieces of <= piece_records records (the native loop
 * uses 256 MiB / record bytes, or KC_PIECE_BYTES).  Mx = world x world
 * record counts (row = source rank).  out[4k..4k+3] = peer, 1 send / 0 receive,
 * offset and count in records (offsets into the destination-grouped send /
 * source-grouped receive buffer); fills at most `cap` transfers and returns
 * how many there are.  Host only (no GPU): the CPU tests check every rank's
 * plan pairs with its peers' for world 1..9. */
int kc_exchange_plan(int world, int me, const uint64_t *Mx, uint64_t piece_records, uint64_t *out, int cap);

/* ---------------------------------------------------------- Simulation */
/* Simulation mode (TLC's -simulate): num_walks bounded random behaviours on
 * one GPU, one lane per walk, each state checked against the invariants, the
 * Asserts and deadlock.  For models whose state space no BFS can finish.
 *
 * RNG (counter-based; csrc/simulate.h, the same code on device and host):
 *   mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x>>30) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ x>>27) * 0x94D049BB133111EB; return x ^ x>>31  (mod 2^64)
 *   K(w)    = mix(mix(seed) ^ w)
 *   r(w, k) = mix(K(w) ^ k)
 *   pick(r, n) = floor(r * n / 2^64)
 *
 * Walk w, 0 <= w < num_walks, has states s_0, s_1, ...; s_0 is Init state
 * pick(r(w, 0), num_init) in kc_spec_init order.  At s_k (k + 1 states so
 * far), in this order:
 *   1. the invariants of cfg.invariants in MC.cfg order: a violation ends the
 *      walk with kind invariant, trace_len = k + 1 (an Init state included,
 *      as in the BFS);
 *   2. if k + 1 == depth the walk ends at the depth limit, not expanded
 *      (depth = the most states in a behaviour, TLC's -depth);
 *   3. an Assert raised while evaluating Next ends it with kind assertion
 *      (whichever successor would have been chosen), trace_len = k + 1;
 *   4. no successor: kind deadlock with cfg.check_deadlock, else the walk has
 *      terminated (no error);
 *   5. else s_{k+1} = successor pick(r(w, k + 1), total) in
 *      kc_spec_successors order; one step is counted for its action.
 * The result is a function of (model, seed, num_walks, depth) alone, whatever
 * steps_per_launch.  The error reported is the error walk with the smallest
 * (trace_len, walk).  The device keeps no trace: kc_sim_replay recomputes a
 * walk on the host, and kc_sim_trace checks that replay against the kind,
 * length and final state the device recorded.
 * stop_on_error = 1: no launch is made after the first one in which a walk
 * erred; the walks advance in lock-step, so the error reported is the same and
 * the totals cover the steps run.
 * count_distinct = 1: distinct_visited = distinct states visited over all
 * walks (Init states included), by 63-bit fingerprint in an HBM FPSet that is
 * grown before each launch to hold live walks x steps more (-ENOMEM if it
 * cannot be). */
#define KC_SIM_MAX_DEPTH 65535
#define KC_SIM_MAX_WALKS (1ull << 30)
/* kc_sim_walks / kc_sim_replay kinds: kc_result.err_kind's 1-3, then */
#define KC_SIM_RUNNING 0      /* stopped early by stop_on_error */
#define KC_SIM_DEPTH 4        /* ended at the depth limit */
#define KC_SIM_TERMINATED 5   /* no successor, check_deadlock off */
typedef struct {
  uint64_t seed;
  uint64_t num_walks;        /* 1 .. 2^30 */
  int depth;                 /* 1 .. KC_SIM_MAX_DEPTH */
  int steps_per_launch;      /* 0 = default */
  int count_distinct;
  int stop_on_error;
} kc_sim_config;
typedef struct {
  uint64_t steps;                     /* successor choices made */
  uint64_t act_steps[KC_NACTIONS];    /* ... per action */
  uint64_t walks_error, walks_depth, walks_terminated;
  uint64_t distinct_visited;          /* with count_distinct */
  int err_kind;                       /* as in kc_result; 0 none */
  int err_action, err_self, err_invariant;
  int trace_len;                      /* states of the reported error walk */
  uint64_t err_walk;
  double seconds;                     /* host wall time of the run */
  double kernel_ms;                   /* HIP events around the walk launches */
  uint64_t launches;                  /* walk launches */
  uint64_t fpset_slots;               /* visited-state table at the end (count_distinct) */
} kc_sim_result;
typedef struct kc_sim kc_sim;
/* Model validation and errors as kc_engine_create (-EINVAL, -ENODEV without a
 * GPU, -ENOMEM); the BFS-only fields of the model config are ignored. */
int kc_sim_create(const kc_model_config *cfg, const kc_sim_config *sim, kc_sim **out);
void kc_sim_destroy(kc_sim *s);
int kc_sim_run(kc_sim *s, kc_sim_result *res);
/* Every walk of the last run: how it ended, its number of states and its final
 * state as a canonical tuple (final_tuples_out may be NULL). */
int kc_sim_walks(kc_sim *s, uint32_t *kind_out, uint32_t *len_out, uint64_t *final_tuples_out);
/* The behaviour of `walk`, replayed on the host and checked against the
 * device's record (-EIO on a mismatch): up to `cap` states as canonical tuples
 * and the action that led to each (-1 for the Init state); returns the number
 * of states. */
int kc_sim_trace(kc_sim *s, uint64_t walk, uint64_t *tuples_out, int *actions_out, int cap);
/* The same as TLC-style text ("State 1: ..."); returns bytes needed or < 0. */
int64_t kc_sim_trace_text(kc_sim *s, uint64_t walk, char *buf, size_t cap);
/* Host copies of the RNG: r(walk, k) and pick(r, n). */
uint64_t kc_sim_rand(uint64_t seed, uint64_t walk, uint64_t k);
uint64_t kc_sim_pick(uint64_t r, uint64_t n);
/* One walk on the host (no GPU needed, no state kept): the steps above run
 * through the host build of the spec code the kernel uses.  Writes up to `cap`
 * states and actions (either may be NULL), *kind_out = how the walk ended;
 * returns the number of states. */
int kc_sim_replay(const kc_model_config *cfg, uint64_t seed, int depth, uint64_t walk,
                  uint64_t *tuples_out, int *actions_out, int cap, int *kind_out);

/* ------------------------------------------------------------ Liveness */
/* KubeAPI.tla's temporal properties (ReconcileCompletes :798,
 * CleansUpProperly :806) on one GPU, under
 *   Spec == Init /\ [][Next]_vars /\ WF_vars(Next)                 (:765).
 *
 * Each property reduces to one question about a state predicate `stay`: is
 * there a behaviour of Spec that reaches a stay state and remains in stay
 * states for ever?
 *   0 ReconcileCompletes  sR ~> ~sR          stay = shouldReconcile[Client]
 *   1 CleansUpProperly    []~sR ~> no Secret/foo in apiState
 *                                            stay = ~sR /\ apiState holds a
 *                                                   version of Secret/foo
 *   2 ClientRestarts      []<>(pc[Client] = "CStart")   (build-defined)
 *                                            stay = pc[Client] # "CStart"
 *   3 SomeActorRestarts   []<>(some client is at CStart or some controller at
 *                         PVCStart)                     (build-defined)
 *                                            stay = no actor is at its start
 * 2 and 3 are not in KubeAPI.tla (as NoLostUpdate is not among its
 * invariants): on this spec 0 and 1 never make the elimination remove a state,
 * and these two do.  0-2 speak of the one client: nc must be 1 (-EINVAL).
 *
 * fairness = 0, WF_vars(Next), the default.  Weak fairness of Next as a whole
 * only forbids stuttering for ever while a step that changes vars is enabled.  On the finite reachable graph, with the
 * edges s -> s dropped (they are not <Next>_vars steps): s is terminal if it
 * has no successor other than itself, and L is the largest set of reachable
 * stay states in which every state is terminal or has a successor in L.  The
 * property is violated iff L is not empty.  L is computed by elimination:
 * alive = stay, then rounds in which an alive, non-terminal state with no alive
 * successor other than itself dies, until a round removes nothing (one-pass
 * OWCTY without the SCC step; exact for this single fairness condition, not
 * for per-process fairness).
 *
 * The counterexample is a shortest behaviour from an Init state to the L state
 * with the smallest (BFS level, discovery index), then from that state the
 * first alive successor other than itself, in kc_spec_successors order, until
 * the walk meets a state it has visited (kind 1, TLC's "Back to state") or a
 * terminal state (kind 2, TLC's "Stuttering").
 *
 * fairness = 1, per-process weak fairness, PlusCal's `fair process`:
 *   Spec /\ (\A p \in ProcSet : WF_vars(step of p)).
 * A model has P = NC + NP + NS <= 5 processes: actor a (clients, then PVC
 * controllers) is process a, server k is process A + k, A = NC + NP.  In
 * kc_spec_successors' slot order, slots a and A + a (the actor's API / ListAPI
 * procedure steps and its own labels, which `fair process` makes fair as
 * WF(P(self)) /\ WF(API(self)) /\ WF(ListAPI(self)); pc makes the three
 * mutually exclusive, so one condition per process is equivalent) are steps
 * of process a, slot 2A + k of process A + k.  Edges s -> s are dropped as
 * above; enabled(s) is the mask of the processes with a successor other than s,
 * and s is terminal iff enabled(s) = 0.  Within the reachable stay states S
 * take the SCCs of the subgraph S induces.  An SCC C of more than one state is
 * fair iff for every process p some state of C has p disabled or some edge
 * with both ends in C is a p step.  F = the union of the fair SCCs and the
 * terminal states of S; L = the states of S from which F is reachable inside
 * S; the property is violated iff F is not empty.  (For weak fairness the
 * maximal SCCs suffice: the witnesses of a fair cycle all lie in its SCC, and
 * an SCC has a cycle through all its states.)  live_states = |L|,
 * live_terminal = the terminal states in L, kc_live_alive gives L.  The
 * counterexample is the same shortest prefix to the L state with the smallest
 * discovery index, a shortest path inside S into F, and then a terminal state
 * (kind 2) or a cycle inside one fair SCC (kind 1) that for every process p
 * contains a p step or visits a state with p disabled.
 *
 * The graph is built by a BFS of the checker's own (the engine is not
 * involved); the invariants are not evaluated.  A state whose Next raises an
 * Assert ends the build: err_kind = 1 and no verdict (kc_engine_* is the tool
 * for safety).  max_states sizes every buffer at create (the edge buffer holds
 * 8 per state); a larger graph ends kc_live_run with -ENOMEM.
 *
 * User formulas (property = KC_LIVE_USER and kc_live_create_formula): two state
 * predicates P and Q as one predicate program (kc_engine_set_invariants'
 * format; END 0 = P, END 1 = Q) and a form.  Every form reduces to the stay
 * question above plus a trigger set T:
 *   form 0   P ~> Q, [](P => <>Q)   stay = ~Q   T = the states where P holds
 *            []<>Q                  the same with P = TRUE
 *   form 1   <>Q                    stay = ~Q   T = the Init states
 * L is computed from alive = stay exactly as above, under either fairness; the
 * property is violated iff L and T share a state, and the counterexample is
 * the shortest prefix to the state of L /\ T with the smallest discovery index,
 * then the same lasso from it (L is closed under "can stay in L for ever").
 * The built-in properties are the case T = every state.  A user formula places
 * no nc = 1 requirement.  <>[]Q is not of this shape (it needs an acceptance
 * condition on the SCCs of the whole graph) and []P is an invariant. */
#define KC_LIVE_USER (-1)
typedef struct {
  int property;              /* 0 .. 3, above; KC_LIVE_USER: with kc_live_create_formula only */
  uint64_t max_states;       /* 0 = 2^24; 16 .. 2^27 */
  int fairness;              /* 0 WF_vars(Next), 1 per process; else -EINVAL */
} kc_live_config;
typedef struct {
  uint64_t states, edges, init; /* the graph: the BFS's distinct, generated - init */
  int depth;                    /* ... and depth */
  uint64_t stay_states, live_states, live_terminal; /* |S|, |L|, terminal states in L */
  uint64_t rounds;              /* trim launches, the last (empty) one included */
  int err_kind, err_action, err_self; /* an Assert met while building the graph */
  int violated;                 /* 1 iff |L| > 0; a user formula: iff |L /\ T| > 0 */
  int kind;                     /* 0 none, 1 back-to-state, 2 stuttering */
  int prefix_len;               /* states up to and including the first L state */
  int trace_len, loop_start;    /* states in the counterexample; 0-based index the last
                                   state steps back to, -1 if stuttering */
  double seconds, build_ms, trim_ms; /* host wall time: the run, the graph build, mark and trim */
  /* fairness = 1 only (0 otherwise): */
  uint64_t sccs, fair_sccs;     /* SCCs of more than one state in S; the fair ones */
  uint64_t fair_states;         /* |F| */
  uint64_t scc_rounds;          /* launches of the SCC, accumulate and closure phases that
                                   end in a counter read */
  double scc_ms;                /* host wall time from the end of the trim to L */
} kc_live_result;
typedef struct kc_live kc_live;
/* Model validation and errors as kc_sim_create (-EINVAL, -ENODEV without a
 * GPU, -ENOMEM); the BFS-only fields of the model config are ignored. */
int kc_live_create(const kc_model_config *cfg, const kc_live_config *live, kc_live **out);
void kc_live_destroy(kc_live *l);
int kc_live_run(kc_live *l, kc_live_result *res);
/* kc_live_create for a user formula: live->property must be KC_LIVE_USER
 * (kc_live_create itself keeps refusing that value: a handle never lacks its
 * formula).  form 0 = leads-to, 1 = eventually (above); program = n_instr
 * instructions of two words each, valid for the model's packed state, with
 * exactly two ENDs.  -EINVAL, the reason in kc_last_error, for a bad program,
 * a bad form or another property, checked before the device is touched. */
int kc_live_create_formula(const kc_model_config *cfg, const kc_live_config *live, int form, const uint64_t *program,
                           int n_instr, kc_live **out);
/* Another formula for the runs that follow, on a handle of
 * kc_live_create_formula; -EINVAL as above, and for a handle created with a
 * built-in property.  The handle keeps the formula it had. */
int kc_live_set_formula(kc_live *l, int form, const uint64_t *program, int n_instr);
/* |S /\ T| and |L /\ T| of the last run of a user formula (violated iff the
 * second is not 0); 0 and 0 for the built-in properties.  (kc_live_result keeps
 * its layout: these two counts are read here.) */
int kc_live_trigger_counts(kc_live *l, uint64_t *trigger_stay_out, uint64_t *trigger_live_out);
/* The counterexample of the last run: up to `cap` states as canonical tuples
 * and the action that led to each (-1 for the Init state); returns the number
 * of states (0 if the property holds). */
int kc_live_trace(kc_live *l, uint64_t *tuples_out, int *actions_out, int cap);
/* The same as TLC-style text ("State 1: ..."); returns bytes needed or < 0. */
int64_t kc_live_trace_text(kc_live *l, char *buf, size_t cap);
/* Every state of the last run's graph, in discovery order, with its final
 * alive bit (1 = in L); for the tests.  Returns the number of states; nothing
 * is written if cap is smaller. */
int kc_live_alive(kc_live *l, uint64_t *tuples_out, uint8_t *alive_out, uint64_t cap);
/* Every edge of the last run's graph (a fairness = 1 run; -EINVAL otherwise),
 * in CSR order: source and target as discovery indices and the process that
 * takes the step; for the tests.  Returns the number of edges; nothing is
 * written if cap is smaller. */
int64_t kc_live_edge_procs(kc_live *l, uint32_t *src_out, uint32_t *dst_out, uint8_t *proc_out, uint64_t cap);
/* stay(tuple) of a property on the host (no GPU), through the code the kernels
 * run: 1 / 0, < 0 on error. */
int kc_live_stay(const kc_model_config *cfg, int property, const uint64_t *tuple);
/* The process (0 .. P-1, above) that takes the step to successor `ordinal` of
 * the state, in kc_spec_successors order, on the host through the code
 * k_live_expand runs; -EINVAL if the state has no such successor or its Next
 * raises an Assert. */
int kc_live_step_process(const kc_model_config *cfg, const uint64_t *tuple, int ordinal);

/* ----------------------------------------------- Seen-set spill (tests) */
/* Host self-check of the cold tier's run search (coldset.hip run_find, the
 * search every GPU lookup of a spilled fingerprint runs): n sorted random
 * keys and their directory; every key must be found and absent keys not,
 * whole-run and through staging windows.  Returns the number of wrong
 * answers (0 expected).  No GPU needed. */
int64_t kc_cold_find_selftest(uint64_t n, uint64_t seed);
/* The same host search on the caller's n strictly ascending keys and m
 * queries (each 1 to 2^21): views[i] = the number of views of the run in
 * which q[i] is found, the views being the whole run (window 0) or its
 * staging windows of `window` keys (a multiple of 8): 1 for a present key, 0
 * for an absent one.  No GPU needed. */
int kc_cold_find_keys_selftest(const uint64_t *keys, uint64_t n, const uint64_t *q, uint64_t m, uint64_t window,
                               uint8_t *views);
/* cold_key (unkey 0) or cold_unkey (1) of n words, on the host (on_device 0)
 * or in a kernel (1). */
int kc_cold_key_selftest(const uint64_t *in, uint64_t *out, uint64_t n, int unkey, int on_device);

/* ------------------------------------------------ Cold tier driven directly (tests) */
/* A kc::ColdSet (csrc/coldset.h) of its own, on a stream of its own
 * (csrc/coldset_selftest.hip).  The arguments are ColdSet::Config's:
 * meta_hbm_bytes / host_bytes 0 = unlimited, dir NULL or "" = no spill
 * directory, window_keys a multiple of 8 in [64, 2^23].  The harness keeps the
 * kernels inside their buffers: -EINVAL, before any launch, for keys not
 * strictly ascending, queries not ascending, n or m of 0 or above 2^21; and
 * after a failed add (which leaves a run without a directory in the set)
 * probe, all_keys and add_run answer -EINVAL until clear. */
int kc_coldset_create(uint64_t meta_hbm_bytes, uint64_t host_bytes, const char *dir, uint64_t window_keys,
                      int bloom_bits, int cache_keys, int merge_div, int merge_threads, void **out);
/* Uploads the n host keys and adds them as a run (ColdSet::add_run). */
int kc_coldset_add_run(void *h, const uint64_t *keys, uint64_t n);
/* Uploads the m queries, the caller's found bytes and hit counter, probes
 * (ColdSet::probe), synchronises and copies both back. */
int kc_coldset_probe(void *h, const uint64_t *q, uint64_t m, uint8_t *found, uint64_t *hits);
/* The integer fields of ColdStats, in this order: runs, runs_disk, keys,
 * host_bytes, disk_bytes, meta_bytes, peak_meta_bytes, merges, merged_keys,
 * disk_written, disk_read, windows_skipped, cached_runs, cached_keys,
 * cache_bytes, cache_uploaded, filter_tests, filter_passed, merge_probes. */
#define KC_COLDSET_NSTATS 19
int kc_coldset_stats(void *h, uint64_t *out);
/* ColdSet::all_keys: the first `cap` of the merged keys into out; returns how
 * many there are (reading a file run counts in disk_read). */
int64_t kc_coldset_all_keys(void *h, uint64_t *out, uint64_t cap);
int kc_coldset_clear(void *h);
void kc_coldset_destroy(void *h);

/* --------------------------------- Kernels joining the seen-set's tiers (tests) */
/* One launch of a kernel of csrc/engine_spill.h, as the engine launches it
 * (csrc/spill_selftest.hip), for Model<1,np,1>, np 1 or 2, with the default
 * constants.  Every index a kernel derives from its input is checked on the
 * host first (-EINVAL).  By kind:
 * 0 k_claimset_keys: a = table image ({fp, ~claim} per slot), na = slots;
 *   out = nout >= cap words, uploaded as given and copied back; res[0] = count.
 * 1 k_spill_queries: a = na packed parents; b[i] = newmask of parent i (nb =
 *   na; bits below its successor count only); c = nc exclusive winner sums per
 *   256-parent tile; out = qkey and res = qloc, nout words each, uploaded as
 *   given and copied back.
 * 2 k_spill_apply: a = table image, na = slots; b = nb x {qkey, qloc, found};
 *   c = newmask of the nc = cap parents (a found query's bit is set, once);
 *   tile_total starts at each tile's popcount.  out = table image (nout = 2 na);
 *   res = [Counters::overflow, newmask x nc, tile_total per 256 parents].
 * 3 k_tile_succ: a = na packed parents; res[t] = successors of tile t. */
int kc_spill_selftest(int kind, int np, const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb,
                      const uint64_t *c, uint64_t nc, uint64_t cap, uint64_t *out, uint64_t nout, uint64_t *res);

/* ------------------------------ Scan, emit and rebuild of a wide level (tests) */
/* One launch of a kernel that turns a wide level's newmask words into the
 * next frontier (csrc/engine_kernels.h), with the engine's grid and block
 * sizes (csrc/emit_selftest.hip).  par = the kind's npar scalars; a, b =
 * inputs; out = the output sections, res = counters.  Everything travels as
 * u64 words, one per element.  Each output section is uploaded as given and
 * copied back whole: KC_EMIT_FORE guard elements, the kernel's array, the
 * caller's aft guards.  Every index a kernel derives from its input is checked
 * on the host first, and every section must hold the worst case the input
 * allows (-EINVAL, with or without a GPU).  cfg is read by kinds 3 and 4 only
 * (nc = ns = 1, np 1 or 2; variant, invariants and the constants apply).
 * 0 k_tile_scan / k_chunk_scan: par = [T, reg_ok, chunk]; a = the
 *   4 * ceil(T / 4) cells the scan loads (pad cells: anything; the first T sum
 *   below 2^32); out = off, max(4 * ceil(T / 4), T + 1) cells at least;
 *   res = the na input cells after the launch.
 * 1 tile_scan_body with ScanMarks: par = [T, reg_ok, stride, nmark <= 16,
 *   extra (0xffffffff: none)]; a, out as kind 0; res = sh_mark[0 .. 16], each
 *   0xA5A5A5A5 before the scan.
 * 2 k_emit_links: par = [n, base, level_gidx, next_gidx, cap, chunk_base, mode,
 *   want_link, want_trace, seclen]; a = newmask[n]; b = tile_off[T + 1] (mode 0;
 *   T = ceil(n / 256)) or coff[ceil(T / 64) + 1] then ttot[T] (mode 1), which
 *   must be the masks' exclusive sums and counts; out = link, parent, ord:
 *   seclen elements each, KC_EMIT_FORE + next_gidx + chunk_base + total + 1 at
 *   least; res = [defer_flags, outdeg[16]].
 * 3 k_emit<M>: par = [n, base, next_base, chunk_base, level_gidx, next_gidx,
 *   keep_trace, mode, seclen_next, seclen_trace]; a = n packed parents raising
 *   no Assert; b = newmask[n], bits below each parent's successor count; mode 0
 *   tile offsets, 1 per-parent offsets (the harness's own sums); out = next
 *   (seclen_next states >= KC_EMIT_FORE + chunk_base - next_base + total), then
 *   parent and ord (seclen_trace >= KC_EMIT_FORE + next_gidx + chunk_base +
 *   total each); res = [err_key, next_cand, act_dist[22], outdeg[16]].
 * 4 k_materialize<M>: par = [n, nprev, mode, gidx0, prev_gidx0, prev_counts];
 *   a = nprev packed states; b = link[n] (mode 0: parent << 8 | position) or
 *   parent[n] then ord[n] (mode 1: global indices, read at gidx0 + i); parents
 *   inside the previous frontier, positions below the parent's successor
 *   count; out = KC_EMIT_FORE + n states at least; res = [defer_flags,
 *   defer_inv_n, next_cand, act_dist[22]].
 * 5 k_parent_chain: par = [g, cap]; a = parent[na] (below na, or ~0), b =
 *   ord[na]; out (pinned host memory) = guards, the length, cap chain words.
 * 6 spread_tile: par = [G, S]; out[b] = spread_tile(b, G, S), b < G. */
#define KC_EMIT_FORE 8
int kc_emit_selftest(int kind, const kc_model_config *cfg, const uint64_t *par, uint64_t npar, const uint64_t *a,
                     uint64_t na, const uint64_t *b, uint64_t nb, uint64_t *out, uint64_t nout, uint64_t *res,
                     uint64_t nres);

/* ------------------------------------------ k_claim and the settle passes (tests) */
/* One launch set of k_claim (csrc/engine_kernels.h) over n parents and a
 * seen-set image of exactly nslots slots, with the product's launch spelling
 * (csrc/claim_selftest.hip).  The data rules are kc_emit_selftest's: u64 words,
 * sections uploaded as given and copied back whole behind KC_EMIT_FORE guard
 * elements, every index checked on the host first (-EINVAL with or without a
 * GPU, -ENODEV only for good input).  cfg: nc = ns = 1, np 1 to 3 (kind 0 also
 * nc = np = 1, ns = 0); variant, invariants and the constants apply.
 * kind 0: k_claim<M>, then the engine's three settle launches; 1: first-claim
 * on 16-B slots; 2: first-claim on the compact table (nslots even); 3: the
 * sharded k_claim<M, 0, true, 1> with record staging, then the settle launches
 * under the rank's claim keys.
 * par = [n, base, level (the successors'), check_deadlock, spread, nslots,
 *   world, rank, flags, nprev, stage_cap, aft]; flags: 1 = the deferred
 *   frontier (kinds 0-2), 2 = with prev_counts, 4 = with csum (kinds 1, 2).
 *   Kinds 0-2: world 1, rank 0, stage_cap 0; kind 3: world 2 to 8, base 0.
 * a = n packed parents (na = n * state words; an Assert parent is legal), b
 *   unused; deferred: na = 0 and b = nprev packed states of the previous
 *   frontier (raising no Assert), then link[n] (parent << 8 | position, inside
 *   the previous frontier and below the parent's successor count).
 * table = the image, in and out: {fp, ~claim} per slot, or the compact table's
 *   fp words; all zero = empty.  nslots >= stored + the frontier's successors
 *   + 1.
 * out = 12 sections, each KC_EMIT_FORE guards + its elements + aft guards:
 *   newmask[n], rcount[tiles], tile_total / ttot[tiles], csum[ceil(tiles / 64)]
 *   (flag 4, else empty), df.out[(base + n) states] and counts_out[base + n]
 *   (deferred, else empty), and for kind 3 (else empty) repmask[n],
 *   cnt[world][n], tcnt[world][tiles], stoff[tiles], the staging buffer
 *   (stage_cap records, raw words), the same records unpacked (state words,
 *   then the key; the harness writes these on the host).  tiles = ceil(n / 256).
 * res = [err_key, overflow, probes, settles, cand_ovf, next_cand, defer_flags,
 *   defer_inv_n, the overflow list's count, stage_cur, act_gen[22],
 *   act_dist[22]].  Test-only. */
int kc_claim_selftest(int kind, const kc_model_config *cfg, const uint64_t *par, uint64_t npar, const uint64_t *a,
                      uint64_t na, const uint64_t *b, uint64_t nb, uint64_t *table, uint64_t ntable, uint64_t *out,
                      uint64_t nout, uint64_t *res, uint64_t nres);

/* --------------------------- The sharded level's exchange kernels (tests) */
/* The kernels of a sharded level (csrc/shard_kernels.h): the owner scans, the
 * send buffer's gather and pack, the TLC-order renumbering, the deferred
 * frontier's rebuild, the undo of a level's generated counts, and the insert
 * of the received records with both emits, each on inputs of the caller's
 * making, with the grids and block sizes ShardT launches them with
 * (csrc/shard_selftest.hip).  The data rules are kc_emit_selftest's: u64 words,
 * sections uploaded as given and copied back whole behind KC_EMIT_FORE guard
 * elements and the caller's aft guards, every index checked on the host first
 * (-EINVAL with or without a GPU, -ENODEV only for good input).  cfg is read by
 * every kind but 0 and 2 (nc = ns = 1, np 1 or 2; variant, invariants and the
 * constants apply).
 * 0 the owner scans: par = [mode, world (1 to 15), T, status_new, status_err,
 *   level1, init_err, want_row, aft]; mode 0 k_owner_tscan on tcnt[world][T],
 *   1 k_owner_cscan on ocsum[world][T] (u32 cells, T >= 1, the scan's pad cells
 *   hold 0xA5A5A5A5), 2 k_owner_scan_small and 3 hipcub's exclusive sum through
 *   Widen8 + k_owner_totals on cnt[world][T] (u8 cells, T parents from 0; mode
 *   2: world * T <= 16384).  a = the world * T cells, owner-major, summing below
 *   2^32; b = the first ten words of Counters (err_key, chunk_base, overflow,
 *   batch_used, cand_total, level_new, emit_done, defer_flags, defer_inv_n,
 *   defer_err).  out = 5 sections: off (modes 0, 1: max(4 * ceil(cells / 4),
 *   cells + 1) cells; 2, 3: cells), tot[16], host_tot[16] and host_head[10]
 *   (pinned host memory), row[world + 3] (want_row 0: the kernel gets no row).
 *   res = the world * T cells after the launch.
 * 1 k_shard_gather<M>: par = [world, T (1 to 2^16 tiles), chunked, nstage,
 *   aft]; a = the staging buffer, nstage records of raw words (4 at np 1, 6 at
 *   np 2); b = stoff[T] (~0: nothing staged; else the tile's segment lies
 *   inside the staging buffer), tcnt[world][T], then toff[world][T] (chunked 0)
 *   or coff[world][ceil(T / 64)] (chunked 1): the owner-major exclusive sums of
 *   tcnt, or of its 64-tile chunk sums.  out = one section: the send buffer,
 *   exactly sum(tcnt) records.
 * 2 TLC order: par = [nn, W (1 to 2^20), aft]; a = pkeys[nn] (parent G << 16 |
 *   position << 8 | action), then link[nn]; b = other[W], the other ranks'
 *   position words, OR-ed in after k_tlc_mask (the all-reduce's stand-in).
 *   Then ShardT::tlc_order's sequence: the NewCount scan, k_tlc_pos, the bitmap
 *   scan, k_tlc_perm.  out = 8 sections: wmask[W], wbase[W], gnew[nn],
 *   bits[W + 1], brank[W + 1], link_out[nn], pk_out[nn], gpos_out[nn].  res =
 *   [Counters::overflow].  With a key of G >= W or position >= 32 (counted as
 *   overflow) only k_tlc_mask runs.
 * 3 k_shard_pack<M>: par = [n, world, rank, with_gpos, aft]; a = n packed
 *   parents raising no Assert; b = repmask[n] (bits below each parent's
 *   successor count), then gpos[n] when with_gpos.  The harness gives the
 *   kernel the owner-major exclusive sums of the marked successors per owner
 *   and parent.  out = 2 sections: the send buffer (exactly the marked
 *   successors' records), then the same records unpacked on the host (state
 *   words, then the key).  res = the records per owner [world].
 * 4 k_shard_materialize<M, tlc>: par = [n, nprev, nrec, rank, tlc, prev_counts,
 *   aft]; a = nprev packed states raising no Assert, then (tlc 1)
 *   prev_gpos[nprev]; b = link[n] (parent << 8 | position inside the previous
 *   frontier and below the parent's successor count, or bit 63 | a record
 *   index below nrec), then nrec records as state words + key (the harness
 *   packs them).  out = n states.  res = [defer_err, next_cand, act_dist[22]].
 * 5 k_undo_gen<M>: par = [n]; a = n packed states (an Assert parent is legal);
 *   b = act_gen[22] before; the plans are Plan::counts of each state, what
 *   k_claim keeps.  No out.  res = act_gen[22] after, mod 2^64.
 * 6, 7 one rank's half of a level after the exchange, as ShardT::expand_dev,
 *   insert and insert_emit launch it; 6 deterministic (k_head_reset, the
 *   sharded k_claim, k_rec_claim, k_settle_both<M, 0>, k_settle_both<M, 1>, the
 *   winners' scan, an emit), 7 first-claim (k_claim FIRST, k_rec_claim_first,
 *   k_win_scan, an emit).
 *   par = [n_local, nrec, level (the successors'), nslots, world (2 to 15),
 *     rank, path, tlc, emit, cap, tail, unfused, next_gidx, aft, cap2, W].
 *     path, kind 6: 0 = tile counts (pass B with wtot, then k_ovf_win_scan, or
 *     with unfused 1 k_settle_ovf<1> + k_win_scan), 1 = pass B without wtot +
 *     k_shard_scan_small, 2 = the same with hipcub's scans + k_shard_base; kind
 *     7: 0 = 16-B slots, 1 = the compact table (nslots even).  tlc 1 (kind 6,
 *     path 0, emit 1): TLC-order claim keys; a ends with gpos[n_local],
 *     strictly increasing and below W, the level's width.  emit 0 =
 *     k_shard_emit, 1 = k_shard_emit_links with cap (path 0 only); cap2 != 0:
 *     after DF_CAPACITY the flags are cleared and the launch repeated with
 *     cap2.  tail 1 = the emit runs the level tail, 0 = k_shard_cand.
 *   a = n_local packed parents (0 is legal); b = nrec records as state words +
 *     key, senders below world and not this rank (TLC: parent G below W).
 *   table = the image, in and out, as kc_claim_selftest's; nslots >= stored +
 *     the parents' successors + nrec + 1.
 *   out = 11 sections: newmask[n_local], rfp[nrec], flag[nrec], isnew[nrec],
 *     wtot and woff [own tiles + record blocks + 8] (path 0 and kind 7, else
 *     empty), offsets[n_local] and ioff[nrec] (kind 6 path 1, 2, else empty),
 *     next[bound states] (emit 0), link[bound] (emit 1), pkeys[next_gidx +
 *     bound + 1]; bound = the parents' successors + nrec.
 *   res = [err_key, overflow, probes, chunk_base, level_new, cand_total,
 *     defer_flags, defer_flags after the first emit launch, act_dist[22], the
 *     pinned host head's 10 words (0xA5.. before)].
 * table is NULL for kinds 0 to 5.  Test-only. */
int kc_shard_selftest(int kind, const kc_model_config *cfg, const uint64_t *par, uint64_t npar, const uint64_t *a,
                      uint64_t na, const uint64_t *b, uint64_t nb, uint64_t *table, uint64_t ntable, uint64_t *out,
                      uint64_t nout, uint64_t *res, uint64_t nres);

/* ------------------------------------------ Liveness graph kernels (tests) */
/* The graph part of the liveness checker (csrc/live_graph.h: the trim, the SCC
 * decomposition, F and the closure to L, the lassos, and the host loops that
 * drive them) on a graph of the caller's making (csrc/live_selftest.hip).  The
 * harness builds the CSR rows, marks alive = stay and terminal with the code
 * k_live_mark runs, and then makes the call kc_live_run makes after its build.
 * The data rules are kc_emit_selftest's: u64 words, sections uploaded as given
 * and copied back whole behind KC_EMIT_FORE guard elements and the caller's aft
 * guards, every input checked on the host first (-EINVAL with or without a
 * GPU, -ENODEV only for good input).
 * par = [n (1 .. 2^22), P (1 .. 8), fairness (0 / 1), path_cap (0 = what
 *   kc_live_create allocates: n * (P + 3) under fairness 1, n under fairness 0,
 *   where a given one must be at least n), aft].
 * deg[n] = out-degrees, summing to ne < 2^31; edges[ne] = targets (< n) in CSR
 *   order, eproc[ne] = the process of each (< P); stay[n] = 0 / 1; parent[n],
 *   level[n] = the discovery order: level[0] = 1, levels never fall along the
 *   index, a level-1 state has parent ~0, any other state has parent[i] < i on
 *   level[i] - 1 with an edge parent[i] -> i.
 * out = alive (= L), terminal, enabled, comp, fair: KC_EMIT_FORE + n + aft
 *   words each; then path: KC_EMIT_FORE + path_cap + aft words.  enabled, comp
 *   and fair come back as given under fairness 0.
 * res = [stay, stay_terminal, removed, trim rounds, sccs, fair_sccs,
 *   fair_states, live, live_terminal, SCC-phase launches, violated, lasso kind,
 *   prefix, loop, len, lasso_err << 32 | -(the driver's return code: 0, or EIO
 *   when it found no counterexample; the sections are still copied back)].
 * Test-only. */
int kc_live_selftest(const uint64_t *par, uint64_t npar, const uint64_t *deg, const uint64_t *edges, uint64_t ne,
                     const uint64_t *eproc, const uint64_t *stay, const uint64_t *parent, const uint64_t *level,
                     uint64_t *out, uint64_t nout, uint64_t *res, uint64_t nres);

/* The two kernels of a user formula alone (csrc/live_prog.h k_live_mark_prog,
 * csrc/live_graph.h k_live_first_trig) on made data (csrc/live_mark_selftest.hip);
 * the data rules are kc_live_selftest's.
 * par = [W (4, 6 or 10), form (0 / 1), n (1 .. 2^22), aft].
 * program = n_instr instructions with exactly two ENDs, valid for W words;
 * packed_states = n * W words; deg[n], edges[ne] = the CSR graph (targets < n,
 * ne < 2^31); level[n] = any levels >= 1; alive_in[n] = 0 / 1, the alive bytes
 * the first-trigger step runs on (it runs after the mark step, on trig as the
 * mark step wrote it).
 * out = alive, terminal, trig as the mark step wrote them: KC_EMIT_FORE + n +
 *   aft words each.
 * res = [stay, stay_terminal, trig_stay, first (0xffffffff = none), trig_live].
 * Test-only. */
int kc_live_mark_selftest(const uint64_t *par, uint64_t npar, const uint64_t *program, int n_instr,
                          const uint64_t *packed_states, const uint64_t *deg, const uint64_t *edges, uint64_t ne,
                          const uint64_t *level, const uint64_t *alive_in, uint64_t *out, uint64_t nout,
                          uint64_t *res, uint64_t nres);

/* ------------------------------------------------ Checkpoint streams (tests) */
/* Device harness for the checkpoint streams (csrc/ckpt_selftest.hip) on a
 * table of exactly nslots slots; layout 0 = 16-B {fp, ~claim} slots, 1 = the
 * compact table's u64 words (nslots even).  stage_bytes as in
 * kc_checkpoint_options.  stats_out has 4 words.
 * kind 0: in = a table image of n words (2 per slot, or 1); k_ckpt_pack over
 *   it in windows of `window` slots (0 = what a staging buffer takes);
 *   out[0 .. count) = the dense fingerprint stream (room for nslots words),
 *   stats_out = [count, sum, xor, words the sink received].
 * kind 1: in = n fingerprints; they go into an empty table through the
 *   recovery's list inserts, at most `window` per launch (0 = a staging
 *   buffer's worth); out = the table image, stats_out = [inserts that were not
 *   new, sum, xor of the list as uploaded, n].  Test-only. */
int kc_ckpt_selftest(int kind, int layout, uint64_t nslots, const uint64_t *in, uint64_t n, uint64_t window,
                     uint64_t stage_bytes, uint64_t *out, uint64_t *stats_out);

/* ------------------------------------------------- Probe primitives (tests) */
/* Device harness for the seen-set probe loops (csrc/probe_selftest.hip): runs
 * n operations of one kind through the product's device functions on a table
 * of exactly nslots slots (any size >= 2; even for the compact table, whole
 * 8-slot buckets for the FPSet, a power of two at most half full for the batch
 * table, the LDS table's own size for the LDS kinds), zeroed or pre-loaded
 * from table_in, and copies back one result word per operation and the final
 * table image (u64 words: 1 per slot for the FPSet and the compact table,
 * {fp, ~claim} / {fp, key} for the others).  mode 0: one lane runs the
 * operations in order; 1: one lane per operation in one launch.  Kinds:
 * 0 fpset_insert, 1 fpset_contains, 2 claimset_claim, 3 the STORE-claim
 * protocol (three launches; res_out[n + i] = operation i holds the slot's
 * claim), 4 claimset_get, 5 claimset_insert_from, 6 fpslots_insert_pair,
 * 7 the same in k_claim's pipelined order, 8 the same from a given pair
 * (keys[2i], keys[2i + 1]), 9 batch_insert + batch_is_rep, 10 / 11 lds_claim
 * of the engine / the sharded tile, 12-14 the ClaimSet / compact / FPSet
 * rehash kernel (table_in: the old table of n slots; res_out[0] = failures).
 * keys: the claim keys (claim = level << 44 | key).  Test-only. */
int kc_probe_selftest(int kind, uint64_t nslots, const uint64_t *fps, const uint64_t *keys, uint64_t n,
                      uint32_t level, int mode, const uint64_t *table_in, uint64_t *res_out,
                      uint64_t *table_out);

/* ---------------------------------------------------------- Spec (host) */
/* Words of the canonical tuple for a model: 1 + 19 * (nc + np + ns). */
int kc_spec_tuple_words(int nc, int np, int ns);
/* Words of the packed state (GPU layout) for a model. */
int kc_spec_state_words(int nc, int np, int ns);
/* Init states as canonical tuples; returns count. */
int kc_spec_init(const kc_model_config *cfg, uint64_t *tuples_out, int cap);
/* Successors of a canonical tuple in TLC order; returns count, or -2 when
 * the state raises an Assert failure (*fail_action set), <0 on error. */
int kc_spec_successors(const kc_model_config *cfg, const uint64_t *tuple, int *actions_out,
                       uint64_t *succ_tuples_out, int cap, int *fail_action);
/* TypeOK/OnlyOneVersion: -1 = both hold, 0 = TypeOK fails, 1 = OOV fails. */
int kc_spec_check(const kc_model_config *cfg, const uint64_t *tuple);
/* Coverage base counters (csrc/cover.h) summed over n canonical tuples, each
 * taken as a state the BFS expands: the host definition of what
 * kc_engine_coverage counts.  sums_out holds kc_cover_count() words. */
int kc_spec_cover(const kc_model_config *cfg, const uint64_t *tuples, uint64_t n, uint64_t *sums_out);
/* A predicate program (kc_engine_set_invariants) on one canonical tuple, on
 * the host through the code k_pred runs: bit k of the result is set when
 * invariant k is FALSE there.  -EINVAL for a bad program or tuple. */
int kc_pred_eval(const kc_model_config *cfg, const uint64_t *program, int n_instr, const uint64_t *tuple);
/* Test-only: k_pred alone on made packed states of W words (4, 6 or 10),
 * launched as the engine launches it on a chunk that starts at index `base`.
 * out = KC_EMIT_FORE guard words, the result block (min over the violating
 * states of (base + i) << 8 | k, or ~0; states evaluated; 8 violation
 * counts), then the caller's aft guards: uploaded as given and copied back
 * whole.  The arguments are validated on the host first (-EINVAL needs no
 * GPU); -ENODEV without one. */
int kc_pred_selftest(int W, const uint64_t *program, int n_instr, const uint64_t *packed_states, uint64_t n_states,
                     uint64_t base, uint64_t *out, uint64_t nout);
int kc_cover_count(void);
/* Name of counter i, or NULL. */
const char *kc_cover_name(int i);
/* Fingerprint of the packed form of a canonical tuple. */
int kc_spec_fingerprint(const kc_model_config *cfg, const uint64_t *tuple, uint64_t *fp_out);
/* The same with the owner projection of the sharded path in its top bits
 * (M::fingerprint<1>): what kc_shard_owner takes. */
int kc_spec_fingerprint_own(const kc_model_config *cfg, const uint64_t *tuple, uint64_t *fp_out);
/* Self-check of the kernels' incremental fingerprint: the number of
 * successors of `tuple` whose fingerprint_succ differs from a full
 * fingerprint (0 expected), <0 on error. */
int kc_spec_fp_selfcheck(const kc_model_config *cfg, const uint64_t *tuple);
/* Packed <-> canonical conversion. */
/* The action of an actor permutation on a state: perm has nc + np entries,
 * perm[a] = the new index of actor a.  -EINVAL if perm is not a permutation or
 * maps a client onto a PVC controller. */
int kc_spec_permute(const kc_model_config *cfg, const uint64_t *tuple, const int *perm, uint64_t *tuple_out);
/* The fingerprint the engine stores under cfg->symmetry: the minimum of
 * kc_spec_fingerprint over the orbit (kc_spec_fingerprint itself at 0). */
int kc_spec_fingerprint_sym(const kc_model_config *cfg, const uint64_t *tuple, uint64_t *fp_out);
/* Device harness (csrc/sym_selftest.hip): the device code of
 * kc_spec_fingerprint_sym over n tuples, one lane per state.  -ENODEV without
 * a GPU. */
int kc_sym_selftest_fps(const kc_model_config *cfg, const uint64_t *tuples, uint64_t n, uint64_t *fps_out);
int kc_spec_pack(const kc_model_config *cfg, const uint64_t *tuple, uint64_t *packed_out);
int kc_spec_unpack(const kc_model_config *cfg, const uint64_t *packed, uint64_t *tuple_out);
/* Constraints (cfg->constraint_stored, constraint_inflight,
 * action_constraints), the host definition on canonical tuples: is successor
 * tuple_x of tuple_s, made by action id `action`, in the model?  0 = in,
 * 1 = cut by a state constraint, 2 = passed those and cut by an action
 * constraint.  tuple_s may be NULL when no action constraint is set (an Init
 * state); -EINVAL (< 0) when it is NULL while one is set, for a bad tuple,
 * an action id outside the action table or a model not built with
 * constraints. */
int kc_spec_in_model(const kc_model_config *cfg, const uint64_t *tuple_s, const uint64_t *tuple_x, int action);
/* Device harness (csrc/con_selftest.hip): the device code of the same hook
 * over n (parent, successor, action) triples, one lane per pair; out[i] as
 * kc_spec_in_model returns it.  -ENODEV without a GPU. */
int kc_con_selftest(const kc_model_config *cfg, const uint64_t *tuples_s, const uint64_t *tuples_x,
                    const int *actions, uint64_t n, int *out);
/* Diagnostic (tests use it to see that a config with the constraint fields
 * off runs the plain engine): which model type a kc_engine was built from,
 * 0 = the plain model, 1 = under symmetry reduction, 2 = under constraints,
 * 3 = under action properties.
 * Not something to branch on: what an engine computes is defined by its
 * config alone. */
int kc_engine_instantiation(kc_engine *e);
/* Action properties (cfg->action_properties), the host definition on
 * canonical tuples: the mask (>= 0) of the properties that the step
 * tuple_s -> tuple_x, made by action id `action`, violates; 0 when the
 * tuples are equal.  -EINVAL (< 0) for a bad tuple, an action id outside the
 * action table, mask bits outside 0..2 or a model not built with action
 * properties. */
int kc_spec_step_violations(const kc_model_config *cfg, const uint64_t *tuple_s, const uint64_t *tuple_x, int action);
/* Device harness (csrc/act_selftest.hip): the device code of the same hook
 * over n (parent, successor, action) triples, one lane per pair; out[i] as
 * kc_spec_step_violations returns it.  -ENODEV without a GPU. */
int kc_act_selftest(const kc_model_config *cfg, const uint64_t *tuples_s, const uint64_t *tuples_x,
                    const int *actions, uint64_t n, int *out);

#ifdef __cplusplus
}
#endif
#endif
