// engine.hip — single-GPU level-synchronous BFS model checker for KubeAPI.tla
// (replaces TLC's BFS ModelChecker + workers, FPSet and StateQueue for this
// spec; MC.out:5).  Host loop + C-ABI kc_engine_*.
//
// Per level (all on one HIP stream, one host sync per level):
//   for each chunk of <= chunk_states parents:
//     k_claim (LDS tile dedup + ClaimSet claims); k_settle_rec<0>, <1> (winners);
//     hipcub exclusive scan; k_emit; k_advance
//   read {next width, next candidates, error key} back.
// The frontier buffers are the StateQueue: double-buffered packed states
// in HBM, FIFO order = (parent order, TLC successor order), identical to a
// sequential TLC -workers 1 BFS.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <array>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kubecheck.h"
#include "ckpt.h"
#include "claim_launch.h"
#include "coldset.h"
#include "cover.h"
#include "pred.h"
#include "engine.h"
#include "engine_kernels.h"
#include "engine_narrow.h"
#include "engine_spill.h"
#include "engine_util.h"
#include "fpset_host.h"
#include "kc_common.h"
#include "squeue.h"

// The symmetric instantiations (EngineT<SymModel<..>>, kc_model_config.symmetry)
// are compiled from this same text as a second translation unit
// (engine_sym.hip defines KC_ENGINE_SYM_TU and includes this file): there the
// launch helpers below are that unit's own copies, and it defines
// make_engine_sym instead of make_engine and the C-ABI.  The constrained
// instantiations (EngineT<ConModel<..>>, kc_model_config.constraint_*) are a
// third unit in the same way (engine_con.hip, KC_ENGINE_CON_TU,
// make_engine_con), and the instantiations under action properties
// (EngineT<ActModel<..>>, kc_model_config.action_properties) a fourth
// (engine_act.hip, KC_ENGINE_ACT_TU, make_engine_act).
#if defined(KC_ENGINE_SYM_TU) || defined(KC_ENGINE_CON_TU) || defined(KC_ENGINE_ACT_TU)
#define KC_ENGINE_DERIVED_TU 1
#endif
namespace kc {

#ifndef KC_ENGINE_DERIVED_TU
namespace {

const char* kActionNames[A_COUNT] = {
    "DoRequest", "DoReply", "DoListRequest", "DoListReply", "CStart", "C1", "C10", "C11",
    "c12", "C13", "C2", "C3", "C8", "C6", "C7", "C4", "C5", "PVCStart", "PVCListedPVCs",
    "PVCHavePVCs", "PVCDone", "APIStart"};

}  // namespace
#else
namespace {
#endif

// chunk_base += the chunk's new states (last exclusive offset + last count,
// or the tile scan's total tile_off[tiles]); cand_total = sum of the
// next_cand stripes (one 64-lane wave, one stripe per lane).  host != nullptr
// (the level's last chunk): the level's head goes straight into pinned host
// memory and the device head is reset for the next level (no copy launch,
// no separate reset launch).
// (K_ADVANCE_THREADS lanes: the 64-KiB snapshot copy is 16 loads per lane,
// all in flight at once; round 5's 64 lanes ran it as 8 dependent batches)
constexpr int K_ADVANCE_THREADS = 256;
__global__ void __launch_bounds__(K_ADVANCE_THREADS)
k_advance(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ newmask, uint64_t n,
          Counters* __restrict__ C, const uint32_t* __restrict__ tile_off, uint64_t tiles,
          unsigned long long* __restrict__ host, unsigned long long* __restrict__ ovf_count = nullptr,
          CtrStripe* __restrict__ snap = nullptr) {
  static_assert(CTR_STRIPES == 64, "one lane per stripe");
  constexpr int UNITS = (int)(CTR_STRIPES * sizeof(CtrStripe) / 16), PER = UNITS / K_ADVANCE_THREADS;
  static_assert(UNITS % K_ADVANCE_THREADS == 0, "whole 16-B units per lane");
  if (ovf_count && threadIdx.x == 0) *ovf_count = 0;   // the next chunk's candidate overflow list starts empty
  // the level's last chunk: the counters as the level leaves them, kept for
  // a deferred-frontier redo from the next level
  if (snap) {
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(C->s);
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(snap);
    ulonglong2 v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = src[k * K_ADVANCE_THREADS + threadIdx.x];
#pragma unroll
    for (int k = 0; k < PER; ++k) dst[k * K_ADVANCE_THREADS + threadIdx.x] = v[k];
  }
  if (threadIdx.x >= 64) return;
  unsigned long long v = C->s[threadIdx.x].next_cand;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (threadIdx.x == 0) {
    C->cand_total = v;
    if (tile_off)
      C->chunk_base += tile_off[tiles];
    else if (n > 0)
      C->chunk_base += (unsigned long long)offsets[n - 1] + NewCount()(newmask[n - 1]);
    if (host) {
      host[0] = C->err_key;
      host[1] = C->chunk_base;
      host[2] = C->overflow;
      host[3] = C->batch_used;
      host[4] = C->cand_total;
      host[5] = C->level_new;
      host[7] = C->defer_flags;
      host[8] = C->defer_inv_n;        // (Counters::defer_inv_n of the pinned copy)
      C->err_key = ~0ull;
      C->chunk_base = 0;
      C->overflow = 0;
      C->batch_used = 0;
      C->defer_flags = 0;
      C->defer_inv_n = 0;
    }
  }
}

// Per-level counter head reset (err_key = ~0; chunk_base, overflow,
// batch_used = 0), enqueued behind the previous level's head read-back so
// it runs while the host waits, not after it.
__global__ void k_level_reset(Counters* __restrict__ C) {
  if (threadIdx.x == 0) {
    C->err_key = ~0ull;
    C->chunk_base = 0;
    C->overflow = 0;
    C->batch_used = 0;
    C->defer_flags = 0;
    C->defer_inv_n = 0;
  }
}

#ifndef KC_ENGINE_DERIVED_TU
const char* action_name(int a) { return (a >= 0 && a < A_COUNT) ? kActionNames[a] : "?"; }
#endif

// Deferred-frontier redo from level X: every fingerprint claimed at a
// successor level above X (inserted by level X or later) leaves the
// ClaimSet.  Linear probing never moves an entry, so with no rehash since
// level X began the table is then exactly what level X found.
__global__ void k_claimset_drop(ClaimEntry* __restrict__ t, uint64_t nslots, uint32_t level) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(t + i);
    if (e.x && ((~e.y) >> CLAIM_KEY_BITS) >= level)
      *reinterpret_cast<ulonglong2*>(t + i) = make_ulonglong2(0ull, 0ull);
  }
}

// The counters as a redo from level X needs them: every stripe as level
// X - 1 left it (prev), except the per-action distinct counts, taken from
// level X's snapshot (cur): on the deferred frontier a level's own states
// are counted when its k_claim rebuilds them, which the exact path (it
// counts them in the previous level's emit) will not do again.
__global__ void __launch_bounds__(64)
k_counters_restore(Counters* __restrict__ C, const CtrStripe* __restrict__ prev, const CtrStripe* __restrict__ cur) {
  CtrStripe& d = C->s[threadIdx.x];
  d = prev[threadIdx.x];
#pragma unroll
  for (int a = 0; a < A_COUNT; ++a) d.act_dist[a] = cur[threadIdx.x].act_dist[a];
}

// fingerprints of a ClaimSet into a dense array (order irrelevant: sorted next)
// (csh: slot i's fp word is word i << csh, DevClaimSet::word_shift)
__global__ void k_claimset_fps(const unsigned long long* __restrict__ w, uint64_t nslots, uint32_t csh,
                               unsigned long long* __restrict__ out, uint64_t cap,
                               unsigned long long* __restrict__ n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long fp = w[i << csh];
    if (fp) {
      const unsigned long long k = atomicAdd(n, 1ull);
      if (k < cap) out[k] = fp;
    }
  }
}
__global__ void k_adjacent_min_gap(const unsigned long long* __restrict__ s, uint64_t n,
                                   unsigned long long* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 < n) atomicMin(out, s[i + 1] - s[i]);
}

#ifdef KC_ENGINE_DERIVED_TU
}  // namespace
#endif

constexpr uint64_t kMaxChunk = (1ull << 27) - 256;

template <class M>
class EngineT final : public EngineBase {
  using State = typename M::State;
  OwnedStream st_;   // (first: destroyed after every buffer below)

 public:
  explicit EngineT(const kc_model_config& cfg) : EngineBase(cfg) {
    flags_ = flags_of(cfg);
    timing_ = cfg.timing == 2 ? 2 : (cfg.timing != 0 ? 1 : 0);
    ablate_ = env_flag("KC_ABLATE", false);
    if (ablate_) timing_ = 1;
    // the narrow-level kernel: on by default; off when the caller asks for
    // explicit chunks (the chunked wide path is what they exercise) or with
    // KC_NARROW=0
    narrow_on_ = cfg.chunk_states == 0 && env_flag("KC_NARROW", true) && !ablate_;
    // frontiers in the StateQueue (spill mode): the chunked wide path only
    queued_ = cfg.frontier_hbm_bytes > 0;
    if (queued_) narrow_on_ = false;
    // seen-set spill: a fixed-size hot ClaimSet + the cold tier (coldset.h);
    // the chunked wide path with tile offsets only
    spill_ = cfg.seen_hbm_bytes > 0;
    if (spill_) narrow_on_ = false;
    tscan_ = spill_ || env_flag("KC_TSCAN", true);
    // KC_NARROW_BATCH: narrow levels enqueued per host sync (A/B)
    if (const uint64_t nb = env_u64("KC_NARROW_BATCH")) narrow_batch_ = (int)nb;
    tscan_reg_ = env_flag("KC_TSCAN_REG", true);
    headcopy_ = env_flag("KC_HEADCOPY", false);
    // deferred frontier (engine_kernels.h DeferArgs): the default wide path
    // (KC_DEFER=0: every level's k_emit builds and stores its new states)
    defer_ = env_flag("KC_DEFER", true) && !spill_ && !queued_ && !ablate_;
    redo_on_ = env_flag("KC_DEFER_REDO", true);        // KC_DEFER_REDO=0: an anomaly redoes the run from Init
    defer_direct_ = env_flag("KC_DEFER_DIRECT", true); // KC_DEFER_DIRECT=0: invariant anomalies are redone too (A/B)
    // KC_DEFER_SLACK: the capacity estimate's factor over the measured
    // successors per state (tests shrink it to force the exact-path redo)
    const char* ds = getenv("KC_DEFER_SLACK");
    if (ds && atof(ds) > 0) defer_slack_ = atof(ds);
    if (defer_) tscan_ = true;    // the link emit takes the tile offsets
    // KC_FIRST_CLAIM=1: first-claim mode (k_claim FIRST) on the in-HBM wide
    // path: the first inserter of a fingerprint wins, no settle passes (decided
    // after the tile scan is, which it needs; kc_result.claim_mode reports it)
    first_claim_ = (cfg.first_claim || env_flag("KC_FIRST_CLAIM", false)) && tscan_ && !spill_ && !queued_;
    // (first-claim mode writes no claim words, so no level's inserts can be
    // dropped: a deferred-frontier capacity anomaly redoes the run from Init;
    // an Assert or deadlock key is reported directly, as on the exact path)
    if (first_claim_) redo_on_ = false;
    // its ClaimSet holds fp words only (8-B slots: half the table to clear);
    // KC_CLAIM_COMPACT=0 keeps 16-B slots (A/B)
    cs_.compact = first_claim_ && env_flag("KC_CLAIM_COMPACT", true);
    chunk_scan_ = env_flag("KC_CHUNK_SCAN", true);
  }
  ~EngineT() override { (void)hipSetDevice(cfg_.device); }   // (the members free themselves on it)

  int state_words() const override { return M::W; }
  // which model type this engine was built from: 0 plain, 1 SymModel, 2 ConModel, 3 ActModel
  int instantiation() const override {
    return M::STEP_CHECKED ? 3 : M::CONSTRAINED ? 2 : std::is_same<Model<M::NC, M::NP, M::NS>, M>::value ? 0 : 1;
  }
  int tuple_words() const override { return M::TUPLE_WORDS; }

  int setup() override {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      set_error("kubecheck: no HIP device visible (the engine has no CPU fallback)");
      return -ENODEV;
    }
    if (cfg_.device < 0 || cfg_.device >= ndev) {
      set_error("kubecheck: bad device %d", cfg_.device);
      return -EINVAL;
    }
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    KC_TRY(st_.create(hipStreamNonBlocking));
    KC_TRY(d_ctr_.alloc(1));
    KC_TRY(h_ctr_.alloc(1));
    KC_TRY(d_ns_.alloc(1));
    KC_TRY(h_ns_.alloc(1));
    if (narrow_on_) KC_TRY(d_nsc_.alloc(1));
    return 0;
  }

  // A deferred level that meets anything but a clean level (an error of any
  // kind, a capacity estimate too small) is redone on the exact,
  // materialising path from the level the anomaly belongs to (redo_from:
  // the ClaimSet, the counters and the host state are put back as that
  // level found them), so error reports and every count come from the path
  // that checks each new state where it is emitted.  When that cannot be
  // done exactly (a rehash since, KC_DEFER_REDO=0) the whole run is redone
  // from Init on the exact path.  (A run recovered from a checkpoint: from
  // the checkpoint, which run_once restores again.)
  int run(kc_result* res) override {
    defer_now_ = defer_;
    int rc = run_once(res);
    if (rc == kDeferRetry) {
      ++defer_fallbacks_;
      defer_now_ = false;
      rc = run_once(res);
      res->defer_fallback = 1;
      res->defer_redo_level = rec_armed_ ? (uint64_t)rec_info_.level : 1;
    }
    rec_armed_ = false;              // (recover() arms one run)
    cover_valid_ = cover_on_ && rc == 0 && res->err_kind == 0;
    pred_valid_ = pred_on_ && rc == 0;
    return rc;
  }

  // ---- expression-level coverage (cover.h).  k_cover runs
  // over each expanded level's parents where they are resident in cur_; a
  // level's sums go to the host at the level's own sync and count once the
  // level is closed (a level the deferred frontier redoes is dropped first).
  int set_coverage(bool on) override {
    if (on && M::CONSTRAINED) {
      set_error("kc_engine_set_coverage: not with constraints (coverage counts every successor's expressions)");
      return -EINVAL;
    }
    if (on && M::STEP_CHECKED) {
      set_error("kc_engine_set_coverage: not with action properties (the coverage counters name none)");
      return -EINVAL;
    }
    if (on && !std::is_same<Model<M::NC, M::NP, M::NS>, M>::value) {   // (a SymModel)
      set_error("kc_engine_set_coverage: not under symmetry reduction (the states explored stand for orbits)");
      return -EINVAL;
    }
    if (on && (spill_ || queued_ || cfg_.trace_host || ablate_)) {
      set_error("kc_engine_set_coverage: not with seen_hbm_bytes, frontier_hbm_bytes or trace_host");
      return -EINVAL;
    }
    if (on && (ck_on_ || rec_armed_)) {
      set_error("kc_engine_set_coverage: not with checkpointing (a checkpoint holds no coverage sums)");
      return -EINVAL;
    }
    if (on && pred_on_) {
      set_error("kc_engine_set_coverage: not with user invariants (kc_engine_set_invariants; a run that ends at a "
                "violation has no coverage to report)");
      return -EINVAL;
    }
    cover_on_ = on;
    cover_valid_ = false;
    return 0;
  }
  int coverage(uint64_t* out, int cap) const override {
    if (!out || cap < KC_COVER_N) {
      set_error("kc_engine_coverage: NULL or fewer than %d words", KC_COVER_N);
      return -EINVAL;
    }
    if (!cover_valid_) {
      set_error(cover_on_ ? "kc_engine_coverage: the last run ended in an error (or there was none)"
                          : "kc_engine_coverage: coverage is off (kc_engine_set_coverage)");
      return -EINVAL;
    }
    for (int k = 0; k < KC_COVER_N; ++k) out[k] = 0;
    for (const auto& lv : cover_levels_)
      for (int k = 0; k < KC_COVER_N; ++k) out[k] += lv.second[k];
    return KC_COVER_N;
  }
  int cover_begin() {
    cover_levels_.clear();
    if (!cover_on_) return 0;
    KC_TRY(d_cover_.alloc(KC_COVER_N));
    KC_TRY(h_cover_.alloc(KC_COVER_N));
    KC_HIP_TRY(hipMemsetAsync(d_cover_, 0, KC_COVER_N * 8, st_));
    return 0;
  }
  // parents [start, start + cn) of the level in cur_
  int cover_count(uint64_t start, uint64_t cn) {
    return cover_launch(cfg_, cur_.p + start, cn, d_cover_.p, st_);
  }
  // the level's sums to the host and the device vector clear again (enqueued; valid after the next sync)
  int cover_fetch() {
    KC_HIP_TRY(hipMemcpyAsync(h_cover_, d_cover_, KC_COVER_N * 8, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipMemsetAsync(d_cover_, 0, KC_COVER_N * 8, st_));
    return 0;
  }
  void cover_commit(int level) {
    std::array<uint64_t, KC_COVER_N> v;
    for (int k = 0; k < KC_COVER_N; ++k) v[k] = h_cover_[k];
    cover_levels_.emplace_back(level, v);
  }
  void cover_drop_from(int level) {
    while (!cover_levels_.empty() && cover_levels_.back().first >= level) cover_levels_.pop_back();
  }

  // ---- user-defined invariants (pred.h).  k_pred runs where
  // k_cover runs: over each expanded level's parents while they are resident
  // in cur_.  A level's result block goes to the host at the level's own sync
  // and counts once the level is closed (a level the deferred frontier redoes
  // is dropped first); the first level with a violating state ends the run.
  int set_invariants(const uint64_t* program, int n_instr) override {
    if (n_instr == 0) {
      pred_on_ = false;
      pred_valid_ = false;
      pred_prog_.clear();
      return 0;
    }
    const char* why = nullptr;
    if (!program) why = "NULL program";
    else if (M::CONSTRAINED)
      why = "not with constraints (TLC checks invariants on the successors a constraint discards; they are never "
            "expanded, so this evaluation on expansion would miss them)";
    else if (M::STEP_CHECKED) why = "not with action properties";
    else if (!std::is_same<Model<M::NC, M::NP, M::NS>, M>::value)
      why = "not under symmetry reduction (a predicate that names a process is not orbit-invariant)";
    else if (spill_ || queued_ || cfg_.trace_host)
      why = "not with seen_hbm_bytes, frontier_hbm_bytes or trace_host";
    else if (ablate_) why = "not with KC_ABLATE";
    else if (cover_on_) why = "not with coverage on (kc_engine_set_coverage)";
    else if (ck_on_ || rec_armed_) why = "not with checkpoint or recover (a checkpoint holds no invariant counts)";
    if (why) {
      set_error("kc_engine_set_invariants: %s", why);
      return -EINVAL;
    }
    const PredInstr* code = reinterpret_cast<const PredInstr*>(program);
    const int ninv = pred_validate(code, n_instr, M::W, &why);
    if (ninv < 0) {
      set_error("kc_engine_set_invariants: bad program (at most %d instructions, %d invariants, nesting depth %d): %s",
                KC_PRED_MAX_INSTR, KC_PRED_MAX_INV, KC_PRED_MAX_DEPTH, why);
      return -EINVAL;
    }
    pred_prog_.assign(code, code + n_instr);
    pred_ninv_ = ninv;
    pred_on_ = true;
    pred_valid_ = false;
    return 0;
  }
  int invariant_stats(uint64_t* out, int cap) const override {
    if (!pred_on_) {
      set_error("kc_engine_invariant_stats: no user invariants are set (kc_engine_set_invariants)");
      return -EINVAL;
    }
    if (!out || cap < 1 + pred_ninv_) {
      set_error("kc_engine_invariant_stats: NULL or fewer than %d words", 1 + pred_ninv_);
      return -EINVAL;
    }
    if (!pred_valid_) {
      set_error("kc_engine_invariant_stats: no run since kc_engine_set_invariants (or the last one failed)");
      return -EINVAL;
    }
    for (int k = 0; k < 1 + pred_ninv_; ++k) out[k] = 0;
    for (const auto& lv : pred_levels_)
      for (int k = 0; k < 1 + pred_ninv_; ++k) out[k] += lv.second[1 + k];
    return 1 + pred_ninv_;
  }
  int pred_begin() {
    pred_levels_.clear();
    if (!pred_on_) return 0;
    KC_TRY(d_pred_prog_.alloc(KC_PRED_MAX_INSTR));
    KC_TRY(d_pred_.alloc(PRED_OUT_WORDS));
    KC_TRY(h_pred_.alloc(PRED_OUT_WORDS));
    KC_HIP_TRY(hipMemcpyAsync(d_pred_prog_, pred_prog_.data(), pred_prog_.size() * sizeof(PredInstr),
                              hipMemcpyHostToDevice, st_));
    return pred_reset(d_pred_.p, st_);
  }
  // parents [start, start + cn) of the level in cur_
  int pred_count(uint64_t start, uint64_t cn) {
    return pred_launch(M::W, cur_.p + start, cn, start, d_pred_prog_.p, (int)pred_prog_.size(), d_pred_.p, st_);
  }
  // the level's block to the host and the device block reset (enqueued; valid after the next sync)
  int pred_fetch() {
    KC_HIP_TRY(hipMemcpyAsync(h_pred_, d_pred_, PRED_OUT_WORDS * 8, hipMemcpyDeviceToHost, st_));
    return pred_reset(d_pred_.p, st_);
  }
  void pred_commit(int level) {
    std::array<uint64_t, PRED_OUT_WORDS> v;
    for (int k = 0; k < PRED_OUT_WORDS; ++k) v[k] = h_pred_[k];
    pred_levels_.emplace_back(level, v);
  }
  void pred_drop_from(int level) {
    while (!pred_levels_.empty() && pred_levels_.back().first >= level) pred_levels_.pop_back();
  }
  // the level just committed holds a violating state: the report (the parent
  // chain of the smallest index, the smallest k it violates)
  bool pred_violated() const { return !pred_levels_.empty() && pred_levels_.back().second[0] != ~0ull; }
  int pred_report(kc_result* res, int level, uint64_t level_gidx, uint64_t n) {
    const uint64_t key = pred_levels_.back().second[0];
    const uint64_t idx = key >> 8;
    if (idx >= n || (int)(key & 0xff) >= pred_ninv_) {
      set_error("kubecheck: bad user-invariant key");
      return -EIO;
    }
    res->err_kind = E_INVARIANT;
    res->err_invariant = 3 + (int)(key & 0xff);
    res->err_level = level;
    res->err_action = res->err_self = -1;
    if (cfg_.keep_trace) {
      std::vector<State> path;
      KC_TRY(path_to(level_gidx + idx, path));
      trace_ = path;
      res->trace_len = (int)path.size();
    }
    return 0;
  }

  // Where the BFS stands at the top of a level.
  // Deferred frontier (defer_now_): `mat` = cur_ holds this level's states.
  // Otherwise the level's k_claim rebuilds them from the previous frontier
  // (next_, which starts at global index prev_gidx) and the links the
  // previous level's emit wrote; `cand` is then unknown and the level's
  // buffers are sized from `ratio`, the last measured successors per state.
  struct LevelCursor {
    uint64_t n = 0, level_gidx = 0, cand = 0, cand_total = 0, prev_gidx = 0;
    int level = 1;
    bool mat = true;
    double ratio = 1.0;
  };

  // ---- checkpoint / recover (ckpt.h).  A checkpoint is the
  // top of a level with its states materialised in cur_: the cursor, the
  // run's totals, the cumulative counters, the ClaimSet's fingerprints and
  // the trace file.  Nothing here runs, and nothing is allocated, unless one
  // of the three calls below was made.
  const char* ckpt_refusal() const {
    if (M::CONSTRAINED) return "not with constraints (a checkpoint header names none)";
    if (M::STEP_CHECKED) return "not with action properties (a checkpoint header names none)";
    if (spill_ || queued_ || cfg_.trace_host) return "not with seen_hbm_bytes, frontier_hbm_bytes or trace_host";
    if (cover_on_) return "not with coverage on (a checkpoint holds no coverage sums)";
    if (pred_on_) return "not with user invariants (a checkpoint holds no invariant counts)";
    if (ablate_) return "not with KC_ABLATE";
    return nullptr;
  }
  int set_checkpoint(const kc_checkpoint_options* opt) override {
    if (!opt) {
      ck_on_ = false;
      ck_every_ = 0;
      ck_seconds_ = 0;
      ck_stage_bytes_ = 0;
      return 0;
    }
    const bool periodic = opt->every_levels > 0 || opt->every_seconds > 0;
    if (const char* why = ckpt_refusal()) {
      set_error("kc_engine_set_checkpoint: %s", why);
      return -EINVAL;
    }
    if (periodic && (!opt->dir || !opt->dir[0])) {
      set_error("kc_engine_set_checkpoint: no directory");
      return -EINVAL;
    }
    if (opt->stage_bytes && opt->stage_bytes < CKPT_STAGE_MIN) {
      set_error("kc_engine_set_checkpoint: stage_bytes %llu below %llu", (unsigned long long)opt->stage_bytes,
                (unsigned long long)CKPT_STAGE_MIN);
      return -EINVAL;
    }
    ck_on_ = periodic;
    ck_every_ = std::max(opt->every_levels, 0);
    ck_seconds_ = opt->every_seconds > 0 ? opt->every_seconds : 0;
    ck_stage_bytes_ = opt->stage_bytes;
    ck_dir_ = opt->dir ? opt->dir : "";
    return 0;
  }
  int checkpoint(const char* dir) override {
    if (!dir || !dir[0]) {
      set_error("kc_engine_checkpoint: no directory");
      return -EINVAL;
    }
    if (const char* why = ckpt_refusal()) {
      set_error("kc_engine_checkpoint: %s", why);
      return -EINVAL;
    }
    if (!stop_valid_) {
      set_error("kc_engine_checkpoint: the last run did not stop at max_levels with states left and no error");
      return -EINVAL;
    }
    return write_checkpoint(dir, stop_cur_, stop_totals_);
  }
  int recover(const char* dir) override {
    if (!dir || !dir[0]) {
      set_error("kc_engine_recover: no directory");
      return -EINVAL;
    }
    if (const char* why = ckpt_refusal()) {
      set_error("kc_engine_recover: %s", why);
      return -EINVAL;
    }
    CkptFileSource src;
    const std::string path = ckpt_path(dir);
    int rc = src.open(path);
    if (rc) {
      set_error("kc_engine_recover: %s: %s", path.c_str(), rc == -ENOENT ? "no such file" : "cannot open");
      return rc;
    }
    std::string err;
    struct kc_checkpoint_info h;
    rc = ckpt_validate(src, &h, &err);
    if (rc) {
      set_error("kc_engine_recover: %s: %s", path.c_str(), err.c_str());
      return rc;
    }
    const int mine[] = {cfg_.nc, cfg_.np, cfg_.ns, cfg_.can_fail != 0, cfg_.can_timeout != 0, cfg_.check_deadlock != 0,
                        cfg_.variant, cfg_.invariants & 7, sym_effective(cfg_.nc, cfg_.np, cfg_.symmetry), M::W};
    const int theirs[] = {h.nc, h.np, h.ns, h.can_fail, h.can_timeout, h.check_deadlock, h.variant, h.invariants,
                          h.symmetry, h.state_words};
    static const char* names[] = {"nc", "np", "ns", "can_fail", "can_timeout", "check_deadlock", "variant",
                                  "invariants", "symmetry", "state_words"};
    for (int k = 0; k < 10; ++k)
      if (mine[k] != theirs[k]) {
        set_error("kc_engine_recover: the checkpoint has %s = %d, the engine %d", names[k], theirs[k], mine[k]);
        return -EINVAL;
      }
    if (cfg_.keep_trace && !h.keep_trace) {
      set_error("kc_engine_recover: the checkpoint has keep_trace = 0 (no trace sections), the engine 1");
      return -EINVAL;
    }
    rec_dir_ = dir;
    rec_info_ = h;
    rec_armed_ = true;
    return 0;
  }

  // the totals of a run so far that a checkpoint carries besides the counters
  struct RunTotals {
    uint64_t init = 0, distinct = 0, peak = 0;
    int nlevels = 0;
    std::vector<uint64_t> widths;
  };
  static RunTotals totals_of(const kc_result* res) {
    RunTotals t;
    t.init = res->init;
    t.distinct = res->distinct;
    t.peak = res->peak_frontier;
    t.nlevels = res->nlevels;
    t.widths.assign(res->level_width, res->level_width + res->nlevels);
    return t;
  }
  bool ckpt_due(int level) const {
    if (ck_every_ > 0 && level > ck_l0_ && (level - ck_l0_) % ck_every_ == 0) return true;
    return ck_seconds_ > 0 &&
           std::chrono::duration<double>(std::chrono::steady_clock::now() - ck_last_).count() >= ck_seconds_;
  }
  // run()'s own checkpoint at the top of level c.level: a deferred frontier
  // is materialised first, as the narrow path and the level capture do
  int ckpt_now(const kc_result* res, LevelCursor& c) {
    if (!c.mat) {
      KC_TRY(materialize(c));
      c.mat = true;
      KC_TRY(counter_snap(c.level - 1));     // (k_materialize counted the states' actions)
      pc_valid_ = false;
    }
    KC_TRY(write_checkpoint(ck_dir_.c_str(), c, totals_of(res)));
    ck_last_ = std::chrono::steady_clock::now();
    return 0;
  }

  int write_checkpoint(const char* dir, const LevelCursor& c, const RunTotals& t) {
    static_assert(sizeof(State) == (size_t)M::W * 8, "a packed state is W words");
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    const auto tw0 = std::chrono::steady_clock::now();
    KC_TRY(ck_stage_.setup(ck_stage_bytes_));
    std::string err;
    CkptWriter wr;
    const int orc = wr.open(dir, &err);
    if (orc) {
      set_error("checkpoint: %s", err.c_str());
      return orc;
    }
    const CkptSink sink = [&wr](const uint64_t* w, uint64_t n) -> int {
      const int r = wr.append(w, n);
      if (r) set_error("checkpoint: write failed: %s", strerror(errno));
      return r;
    };
    // COUNTERS: the widths, then the striped totals summed
    KC_HIP_TRY(hipStreamSynchronize(st_));
    if (!ck_ctr_) ck_ctr_.reset(new Counters);
    KC_HIP_TRY(hipMemcpy(ck_ctr_.get(), d_ctr_, sizeof(Counters), hipMemcpyDeviceToHost));
    std::vector<uint64_t> cw(t.widths);
    for (int a = 0; a < A_COUNT; ++a) cw.push_back(ck_ctr_->act_gen(a));
    for (int a = 0; a < A_COUNT; ++a) cw.push_back(ck_ctr_->act_dist(a));
    for (int b = 0; b < OUTDEG_BINS; ++b) cw.push_back(ck_ctr_->outdeg(b));
    cw.push_back(ck_ctr_->probes());
    cw.push_back(ck_ctr_->settles());
    cw.push_back(ck_ctr_->cand_ovf());
    cw.push_back(narrow_probes_);
    static_assert(2 * A_COUNT + OUTDEG_BINS + 4 == CKPT_COUNTER_TAIL, "the COUNTERS section's fixed part");
    wr.begin(CS_COUNTERS);
    KC_TRY(sink(cw.data(), cw.size()));
    wr.begin(CS_FRONTIER);
    KC_TRY(ckpt_download(cur_.p, c.n * sizeof(State), ck_stage_, st_, sink));
    // FPS: the device's count and checksum of the stream against the run's
    // count and what reached the file
    wr.begin(CS_FPS);
    uint64_t nfp = 0;
    CkptSum dsum;
    double pack_ms = 0;
    const auto tp0 = std::chrono::steady_clock::now();
    KC_TRY(ckpt_pack_fps(cs_, 0, ck_stage_, st_, sink, &nfp, &dsum, cfg_.verbose ? &pack_ms : nullptr));
    const double fps_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count();
    if (nfp != t.distinct || nfp != cs_.count) {
      set_error("checkpoint: the seen-set holds %llu fingerprints, the run counted %llu", (unsigned long long)nfp,
                (unsigned long long)t.distinct);
      return -EIO;
    }
    if (!(dsum == wr.sum(CS_FPS))) {
      set_error("checkpoint: the fingerprint stream's checksum changed between the device and the file");
      return -EIO;
    }
    const uint64_t states = c.level_gidx + c.n;
    if (cfg_.keep_trace) {
      wr.begin(CS_TRACE_PARENT);
      KC_TRY(ckpt_download(tf_.parent(), states * 8, ck_stage_, st_, sink));
      wr.begin(CS_TRACE_ORD);
      KC_TRY(ckpt_download(tf_.ord(), states, ck_stage_, st_, sink));
    }
    uint64_t w[CKPT_HEADER_WORDS] = {};
    w[CW_NC] = (uint64_t)cfg_.nc, w[CW_NP] = (uint64_t)cfg_.np, w[CW_NS] = (uint64_t)cfg_.ns;
    w[CW_CAN_FAIL] = cfg_.can_fail != 0, w[CW_CAN_TIMEOUT] = cfg_.can_timeout != 0;
    w[CW_CHECK_DEADLOCK] = cfg_.check_deadlock != 0;
    w[CW_VARIANT] = (uint64_t)cfg_.variant;
    w[CW_INVARIANTS] = (uint64_t)(cfg_.invariants & 7);
    w[CW_SYMMETRY] = (uint64_t)sym_effective(cfg_.nc, cfg_.np, cfg_.symmetry);
    w[CW_STATE_WORDS] = (uint64_t)M::W;
    w[CW_KEEP_TRACE] = cfg_.keep_trace != 0;
    w[CW_CLAIM_MODE] = first_claim_ ? 1 : 0;
    w[CW_LEVEL] = (uint64_t)c.level, w[CW_LEVEL_GIDX] = c.level_gidx, w[CW_N] = c.n;
    w[CW_CAND] = c.cand, w[CW_CAND_TOTAL] = c.cand_total;
    w[CW_INIT] = t.init, w[CW_DISTINCT] = t.distinct, w[CW_NLEVELS] = (uint64_t)t.nlevels;
    w[CW_PEAK_FRONTIER] = t.peak;
    const int frc = wr.finish(w, &err);
    if (frc) set_error("checkpoint: %s", err.c_str());
    if (cfg_.verbose && !frc)
      fprintf(stderr, "kubecheck: checkpoint at level %d: %llu bytes, %llu states; k_ckpt_pack %.3f ms over %llu table "
                      "bytes; FPS section %.3f s; whole write %.3f s\n",
              c.level, (unsigned long long)wr.file_bytes(), (unsigned long long)t.distinct, pack_ms,
              (unsigned long long)(cs_.nslots * cs_.slot_bytes()), fps_s,
              std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count());
    return frc;
  }

  // The armed run's start, in place of seed_init: c and res as the
  // checkpointed run had them at the top of its level.
  int restore_run(kc_result* res, LevelCursor& c) {
    const struct kc_checkpoint_info& h = rec_info_;
    CkptFileSource src;
    const std::string path = ckpt_path(rec_dir_.c_str());
    std::string err;
    struct kc_checkpoint_info now;
    if (src.open(path) || ckpt_parse_header(src, &now, &err) || now.file_bytes != h.file_bytes ||
        now.level != h.level || now.distinct != h.distinct ||
        memcmp(now.section_sum, h.section_sum, sizeof h.section_sum) != 0) {
      set_error("kubecheck: %s is gone or changed since kc_engine_recover", path.c_str());
      return -EIO;
    }
    KC_TRY(ck_stage_.setup(ck_stage_bytes_));
    // one section's words, and the device's checksum of it against the header's
    auto feed_of = [&](int s) {
      return CkptFeed([&src, &h, s](uint64_t* dst, uint64_t at, uint64_t n) -> int {
        if (src.read(h.section_offset[s] + at * 8, dst, n * 8)) return 0;
        set_error("kubecheck: checkpoint read failed");
        return -EIO;
      });
    };
    auto same = [&](int s, const CkptSum& got) -> int {
      if (got.sum == h.section_sum[s] && got.x == h.section_xor[s]) return 0;
      set_error("kubecheck: checkpoint section %d fails its checksum on the device", s);
      return -EIO;
    };
    // the Init states: path_to starts from them
    std::vector<State> init;
    std::vector<uint64_t> fps;
    (void)init_list(init, fps);
    init_states_ = init;
    // the seen-set: the table seed_init would make, grown for the checkpoint's
    // fingerprints by the engine's own rule, filled by the list inserts
    const uint64_t fp_slots = cfg_.fpset_slots ? cfg_.fpset_slots : (1ull << 20);
    if (cs_.t && cs_.capacity() >= fp_slots) {
      KC_TRY(cs_.clear(st_));
    } else {
      KC_TRY(cs_.init(fp_slots, st_));
    }
    KC_TRY(cs_.reserve(h.distinct, st_));
    uint64_t bad = 0;
    CkptSum got;
    KC_TRY(ckpt_restore_fps(cs_, h.distinct, 0, ck_stage_, st_, feed_of(CS_FPS), &bad, &got));
    if (bad) {
      set_error("kubecheck: %llu of the checkpoint's fingerprints were not new to the table", (unsigned long long)bad);
      return -EIO;
    }
    KC_TRY(same(CS_FPS, got));
    cs_.count = h.distinct;
    hot_count_ = h.distinct;
    // the frontier and the trace file
    KC_TRY(cur_.grow(h.n, st_));
    KC_TRY(ckpt_upload(cur_.p, h.n * M::W, ck_stage_, st_, feed_of(CS_FRONTIER), &got));
    KC_TRY(same(CS_FRONTIER, got));
    const uint64_t states = h.level_gidx + h.n;
    KC_TRY(tf_.grow(false, cfg_.keep_trace ? states + h.cand + 16 : h.init + h.cand, st_, false));
    if (cfg_.keep_trace) {
      KC_TRY(ckpt_upload(tf_.parent(), states, ck_stage_, st_, feed_of(CS_TRACE_PARENT), &got));
      KC_TRY(same(CS_TRACE_PARENT, got));
      // (the padding of the last word is part of the section: cap >= states + 16)
      KC_TRY(ckpt_upload(tf_.ord(), h.section_bytes[CS_TRACE_ORD] / 8, ck_stage_, st_, feed_of(CS_TRACE_ORD), &got));
      KC_TRY(same(CS_TRACE_ORD, got));
    }
    // the counters: the saved totals in stripe 0, zero in the rest
    std::vector<uint64_t> cw(h.section_bytes[CS_COUNTERS] / 8);
    KC_TRY(feed_of(CS_COUNTERS)(cw.data(), 0, cw.size()));
    const uint64_t* q = cw.data() + h.nlevels;
    if (!ck_ctr_) ck_ctr_.reset(new Counters);
    memset(ck_ctr_.get(), 0, sizeof(Counters));
    CtrStripe& s0 = ck_ctr_->s[0];
    for (int a = 0; a < A_COUNT; ++a) s0.act_gen[a] = q[a];
    for (int a = 0; a < A_COUNT; ++a) s0.act_dist[a] = q[A_COUNT + a];
    for (int b = 0; b < OUTDEG_BINS; ++b) s0.outdeg[b] = q[2 * A_COUNT + b];
    q += 2 * A_COUNT + OUTDEG_BINS;
    s0.probes = q[0];
    s0.settles = q[1];
    s0.cand_ovf = q[2];
    narrow_probes_ = q[3];
    s0.next_cand = h.cand_total;
    KC_HIP_TRY(hipMemcpyAsync(d_ctr_, ck_ctr_.get(), sizeof(Counters), hipMemcpyHostToDevice, st_));
    if (d_ovf_cnt_) KC_HIP_TRY(hipMemsetAsync(d_ovf_cnt_, 0, 8, st_));
    if (csum_) KC_HIP_TRY(hipMemsetAsync(csum_, 0, csum_.cap * sizeof(uint32_t), st_));
    // (a deferred-frontier redo from this level needs the previous level's counters)
    if (defer_now_) KC_TRY(counter_snap(h.level - 1));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    res->init = h.init;
    res->distinct = h.distinct;
    res->peak_frontier = h.peak_frontier;
    res->nlevels = h.nlevels;
    for (int L = 0; L < h.nlevels; ++L) res->level_width[L] = cw[L];
    c = LevelCursor{};
    c.n = h.n;
    c.level_gidx = h.level_gidx;
    c.cand = h.cand;
    c.cand_total = h.cand_total;
    c.level = h.level;
    return 0;
  }

  // What a level's launches share, fixed when its buffers are sized.
  struct LevelPlan {
    bool dfr = false;            // this level runs deferred (emits links, not states)
    bool use_link = false;       // links in HBM (the trace may be host memory)
    uint64_t bound = 0, next_gidx = 0, link_cap = ~0ull;
    uint32_t succ_level = 0;     // BFS level of the successors
    DeferArgs df;
  };
  // a step's answer beyond "go on" (0) and an error (< 0)
  static constexpr int kRunDone = 1;     // the result is complete (an error of the model was reported)
  static constexpr int kGoWide = 2;      // the narrow kernel took no level: this one runs wide

  int run_once(kc_result* res) {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    reset_run(res);
    KC_TRY(cover_begin());
    KC_TRY(pred_begin());
    LevelCursor c;
    std::vector<State> init;
    int rc = rec_armed_ ? restore_run(res, c) : seed_init(res, c, init);
    if (rc) return rc < 0 ? rc : 0;
    ck_l0_ = c.level;
    ck_last_ = t0_;

    if (queued_) return run_queued(res, c.n, c.cand, init);

    // default: one chunk per level; chunk_states bounds the per-chunk
    // buffers.  Claims are level-global (keys grow with the parent index),
    // so a chunk's winners are final once its own claim pass is done.
    // per-level counter fields: err_key = ~0, the rest 0 (act_* are cumulative)
    hipLaunchKernelGGL(k_level_reset, dim3(1), dim3(64), 0, st_, d_ctr_.p);
    // <= 2^27 parents per chunk: the chunk's scan runs on int counts and its
    // offsets are u32 (at most 32 new states per parent: < 2^32 per chunk)
    const uint64_t chunk =
        (std::min<uint64_t>(cfg_.chunk_states ? cfg_.chunk_states : kMaxChunk, kMaxChunk) + 255) / 256 * 256;
    c.ratio = c.n ? (double)c.cand / (double)c.n : 1.0;
    pc_valid_ = false;                 // pc_prev_ holds the previous frontier's plans
    while (c.n > 0) {
      if (cfg_.max_levels && c.level >= cfg_.max_levels) break;
      if (ck_on_ && ckpt_due(c.level)) KC_TRY(ckpt_now(res, c));
      if (narrow_on_ && c.n <= (uint64_t)NARROW_MAX &&
          (c.mat || (double)c.n * c.ratio <= 1.25 * (double)NARROW_CAND_MAX)) {
        rc = narrow_levels(res, c);
        if (rc < 0) return rc;
        if (rc == kRunDone) return 0;
        if (rc != kGoWide) continue;
        // not even one level fitted (buffer room): this level goes wide
      }
      LevelPlan lp;
      KC_TRY(size_level(res, c, chunk, lp));
      for (uint64_t start = 0, cn = 0; start < c.n; start += cn) {
        cn = std::min(chunk, c.n - start);
        // seen-set spill: a chunk whose insertions fit the hot table (may flush it)
        if (spill_) KC_TRY(spill_cut(cur_ + start, cn, &cn));
        ++res->levels_chunks;
        KC_TRY(launch_chunk(c, lp, start, cn));
      }
      rc = close_level(res, c, lp);
      if (rc < 0) return rc;
      if (rc == kRunDone) return 0;
    }
    // the last, unexpanded level (max_levels): its states' invariants
    if (!c.mat && c.n) KC_TRY(materialize(c));
    last_level_ = res->nlevels;
    last_n_ = c.n;
    finish(res, c.n);
    // what kc_engine_checkpoint writes: the level's top as this run left it
    if (c.n && !spill_) {
      stop_cur_ = c;
      stop_cur_.mat = true;
      stop_totals_ = totals_of(res);
      stop_valid_ = true;
    }
    if (ablate_) KC_TRY(ablate_report());
    return 0;
  }

  // ---- the steps of run_once

  void reset_run(kc_result* res) {
    memset(res, 0, sizeof *res);
    res->err_action = res->err_self = res->err_invariant = -1;
    res->claim_mode = first_claim_ ? 1 : 0;
    trace_.clear();
    stop_valid_ = false;
    narrow_probes_ = 0;
    for (auto& t : ktime_ms_) t = 0;
    ev_kind_.clear();
    ev_used_ = 0;
    for (auto& c : klaunch_) c = 0;
    narrow_levels_ = 0;
    exact_until_ = 0;
    for (auto& v : snap_lv_) v = -1;
    for (auto& h : hs_) h.c.level = -1;
    for (auto& v : succ_lv_) v = -1;
    t0_ = std::chrono::steady_clock::now();
  }

  // ---- Init (KubeAPI.tla:455-469), on the host: 2^NC states into cur_, the
  // seen-set and the trace; their invariants.  c: level 1.  kRunDone: an
  // Init state violates an invariant (reported).
  // (under symmetry the fingerprint is the orbit's: of the Init states of
  // one orbit the first is kept, the others count as generated only)
  // the Init states kept (one per fingerprint), their fingerprints and successor count
  // (an Init state outside a state constraint is discarded: generated, not
  // distinct, counted in cut_state)
  uint64_t init_list(std::vector<State>& init, std::vector<uint64_t>& fps, uint64_t* cut = nullptr) const {
    uint64_t cand = 0;
    for (int k = 0; k < M::num_init(); ++k) {
      State s0;
      M::init_state(k, s0, cfg_.variant);
      if (M::init_in_model(s0, flags_) != CUT_NONE) {
        if (cut) ++*cut;
        continue;
      }
      const uint64_t fp0 = M::fingerprint(s0);
      if (std::find(fps.begin(), fps.end(), fp0) != fps.end()) continue;
      init.push_back(s0);
      fps.push_back(fp0);
      cand += (uint64_t)M::plan(s0, flags_).total;
    }
    return cand;
  }
  int seed_init(kc_result* res, LevelCursor& c, std::vector<State>& init) {
    const int ni_all = M::num_init();
    std::vector<uint64_t> fps;
    init_cut_ = 0;
    const uint64_t cand = init_list(init, fps, &init_cut_);
    const int ni = (int)init.size();
    // under constraints: the invariants of every Init state, the discarded
    // ones included (TLC checks a state it did not find in the seen-set, and
    // one outside the model is never looked up); and a run all of whose Init
    // states are outside the constraint has nothing to explore.  Only a
    // violating DISCARDED Init state (the first violator in Init order) is
    // reported here, with the kept Init states counted as the path below
    // counts them; a violating Init state inside the model is that path's.
    if constexpr (M::CONSTRAINED) {
      int bad = -1, inv = -1;
      State s0;
      for (int k = 0; k < ni_all && bad < 0; ++k) {
        M::init_state(k, s0, cfg_.variant);
        inv = M::check(s0, flags_.inv_mask);
        if (inv >= 0) bad = k;
      }
      if (bad >= 0 && M::init_in_model(s0, flags_) == CUT_NONE) bad = -1;   // (in the model: reported below)
      if (bad >= 0 || ni == 0) {
        KC_HIP_TRY(hipMemsetAsync(d_ctr_, 0, sizeof(Counters), st_));
        KC_HIP_TRY(hipStreamSynchronize(st_));
        res->init = res->generated = ni_all;
        res->distinct = ni;
        if (ni) {
          res->level_width[0] = ni;
          res->nlevels = 1;
        }
        init_states_ = init;
        c = LevelCursor{};
        c.n = 0;
        if (bad >= 0) {
          res->err_kind = E_INVARIANT;
          res->err_invariant = inv;
          res->err_level = 1;
          trace_.push_back(s0);
          res->trace_len = 1;
        }
        finish(res, 0);
        return kRunDone;
      }
    }
    // the seen-set allocation is kept across runs (cleared each run), like a
    // TLC FPSet pre-sized with -fpmem; it grows by rehash when needed
    const uint64_t fp_slots = cfg_.fpset_slots ? cfg_.fpset_slots : (1ull << 20);
    if (spill_) {
      KC_TRY(spill_setup());
    } else if (cs_.t && cs_.capacity() >= fp_slots) {
      KC_TRY(cs_.clear(st_));
    } else {
      KC_TRY(cs_.init(fp_slots, st_));
    }
    KC_TRY(cur_.grow((uint64_t)ni, st_));
    KC_TRY(tf_.grow(cfg_.trace_host, (uint64_t)ni + cand, st_, false));
    KC_HIP_TRY(hipMemcpyAsync(cur_, init.data(), ni * sizeof(State), hipMemcpyHostToDevice, st_));
    // (the Init fingerprints' device buffers are kept across runs: a
    // hipMalloc / hipFree pair per run cost a device-wide sync)
    KC_TRY(init_fps_.grow((uint64_t)ni, st_));
    KC_TRY(init_res_.grow((uint64_t)ni, st_));
    KC_HIP_TRY(hipMemcpyAsync(init_fps_, fps.data(), ni * 8, hipMemcpyHostToDevice, st_));
    launch_claimset_insert_list(init_fps_.p, (uint64_t)ni, cs_, 1u, init_res_.p, st_);
    std::vector<int> ires(ni);
    KC_HIP_TRY(hipMemcpyAsync(ires.data(), init_res_, ni * sizeof(int), hipMemcpyDeviceToHost, st_));
    std::vector<unsigned long long> ipar(ni, ~0ull);
    std::vector<uint8_t> iord(ni);
    for (int k = 0; k < ni; ++k) iord[k] = (uint8_t)k;
    if (cfg_.trace_host) {
      KC_HIP_TRY(hipStreamSynchronize(st_));
      memcpy(tf_.parent(), ipar.data(), ni * 8);
      memcpy(tf_.ord(), iord.data(), ni);
    } else {
      KC_HIP_TRY(hipMemcpyAsync(tf_.parent(), ipar.data(), ni * 8, hipMemcpyHostToDevice, st_));
      KC_HIP_TRY(hipMemcpyAsync(tf_.ord(), iord.data(), ni, hipMemcpyHostToDevice, st_));
    }
    KC_HIP_TRY(hipStreamSynchronize(st_));
    for (int k = 0; k < ni; ++k) {
      if (ires[k] != CL_NEW) {
        set_error("kubecheck: init states not distinct");
        return -EIO;
      }
    }
    cs_.count = ni;
    hot_count_ = ni;
    KC_HIP_TRY(hipMemsetAsync(d_ctr_, 0, sizeof(Counters), st_));
    if (d_ovf_cnt_) KC_HIP_TRY(hipMemsetAsync(d_ovf_cnt_, 0, 8, st_));
    // k_chunk_scan's chunk sums: zero when a level starts (a run that
    // stopped between k_claim and the scan left them dirty)
    if (csum_) KC_HIP_TRY(hipMemsetAsync(csum_, 0, csum_.cap * sizeof(uint32_t), st_));
    if (defer_now_) KC_TRY(counter_snap(0));
    res->init = ni_all;
    res->generated = ni_all;
    res->distinct = ni;
    init_states_ = init;

    c = LevelCursor{};
    c.n = ni;
    c.cand = cand;
    res->level_width[0] = c.n;
    res->nlevels = 1;
    // invariants of the initial states
    for (int k = 0; k < ni; ++k) {
      const int inv = M::check(init[k], flags_.inv_mask);
      if (inv >= 0) {
        res->err_kind = E_INVARIANT;
        res->err_invariant = inv;
        res->err_level = 1;
        trace_.push_back(init[k]);
        res->trace_len = 1;
        finish(res, c.n);
        return kRunDone;
      }
    }
    return 0;
  }

  // ---- narrow levels: one single-workgroup launch runs as many levels as
  // fit (engine_narrow.h); the host takes over at the first level it cannot
  // run.  It needs the states and their exact successor count: a deferred
  // frontier is materialised first.  kGoWide: no level ran and there are
  // states left.
  int narrow_levels(kc_result* res, LevelCursor& c) {
    if (!c.mat) {
      KC_TRY(materialize(c));
      c.mat = true;
      KC_TRY(counter_snap(c.level - 1));     // (k_materialize counted the states' actions)
    }
    pc_valid_ = false;
    int stop = cfg_.max_levels;
    if (capture_level_ >= c.level + 1 && (stop == 0 || capture_level_ - 1 < stop)) stop = capture_level_ - 1;
    // coverage: one level per run, counted from cur_ before the run expands it
    if ((cover_on_ || pred_on_) && (stop == 0 || c.level + 1 < stop)) stop = c.level + 1;
    // a checkpoint by levels: the run stops at the top of the next level due
    if (ck_on_ && ck_every_ > 0) {
      const int due = c.level + ck_every_ - (c.level - ck_l0_) % ck_every_;
      if (stop == 0 || due < stop) stop = due;
    }
    const int level0 = c.level;
    const uint64_t n0 = c.n, gidx0 = c.level_gidx;
    NarrowRun nr;
    KC_TRY(run_narrow(c, stop, nr));
    bool pred_bad = false;
    if (pred_on_ && nr.counted) {
      // (as coverage below: a run that took no level leaves it to the wide path, which evaluates it again)
      KC_TRY(pred_fetch());
      KC_HIP_TRY(hipStreamSynchronize(st_));
      if (nr.levels > 1) {
        set_error("kubecheck: user invariants: the narrow kernel ran %d levels in one run", nr.levels);
        return -EIO;
      }
      if (nr.levels == 1) {
        pred_commit(level0);
        pred_bad = pred_violated();
      }
    }
    if (cover_on_ && nr.counted) {
      // (a run that took no level leaves it to the wide path, which counts it again)
      KC_TRY(cover_fetch());
      KC_HIP_TRY(hipStreamSynchronize(st_));
      if (nr.levels > 1) {
        set_error("kubecheck: coverage: the narrow kernel ran %d levels in one run", nr.levels);
        return -EIO;
      }
      if (nr.levels == 1) cover_commit(level0);
    }
    res->distinct += nr.new_total;
    for (int L = level0; L < c.level; ++L) {
      if (L >= KC_MAX_LEVELS) {
        set_error("kubecheck: more than %d levels", KC_MAX_LEVELS);
        return -ENOMEM;
      }
      res->level_width[L] = h_ns_->widths[L];
    }
    if (nr.levels) res->peak_frontier = std::max<uint64_t>(res->peak_frontier, std::max(n0, nr.peak));
    if (nr.levels) res->nlevels = c.n ? c.level : c.level - 1;
    if (pred_bad) {
      // the level's own violation comes before anything its expansion found
      // (an NX_ERROR included, which leaves the next level's width unrecorded);
      // the counts are the whole level's, the width of what it found included
      res->nlevels = level0;
      if (nr.new_total && level0 < KC_MAX_LEVELS) {
        res->level_width[level0] = nr.new_total;
        res->nlevels = level0 + 1;
      }
      KC_TRY(pred_report(res, level0, gidx0, n0));
      finish(res, 0);
      return kRunDone;
    }
    if (defer_now_ && nr.levels && nr.reason != NX_ERROR) KC_TRY(counter_snap(c.level - 1));
    if (nr.reason == NX_ERROR) {
      KC_TRY(report_error(res, h_ns_->err_key, c.level, c.level_gidx, c.n));
      finish(res, 0);
      return kRunDone;
    }
    return (nr.levels > 0 || c.n == 0) ? 0 : kGoWide;
  }

  // The per-chunk buffers of a level whose chunks have <= cmax parents and
  // whose successors number <= bound (run_once and run_queued).
  int size_chunk_buffers(uint64_t cmax, uint64_t bound, int level, uint64_t n) {
    const uint64_t tiles = (cmax + CLAIM_TILE - 1) / CLAIM_TILE;
    KC_TRY(rcount_.grow(tiles, st_));
    if (tscan_) {
      KC_TRY(ttot_.grow(tiles + 4, st_));
      KC_TRY(toff_.grow(tiles + 4, st_));
      if (first_claim_ && chunk_scan_) {
        const uint64_t old = csum_.cap;
        KC_TRY(csum_.grow(tiles / CSUM_TILES + 4, st_));
        if (csum_.cap != old) KC_HIP_TRY(hipMemsetAsync(csum_, 0, csum_.cap * sizeof(uint32_t), st_));
      }
    }
    KC_TRY(rec_fp_.grow(tiles * CLAIM_RCAP, st_));
    KC_TRY(rec_lk_.grow(tiles * CLAIM_RCAP, st_));
    KC_TRY(cand_overflow(bound, level, n));
    KC_TRY(newmask_.grow(cmax, st_));
    return offsets_.grow(cmax, st_);
  }

  // Capacity for this level's output, and what its launches share (lp).
  int size_level(kc_result* res, LevelCursor& c, uint64_t chunk, LevelPlan& lp) {
    if (c.n >= (1ull << 32)) {
      set_error("kubecheck: level wider than 2^32 states");
      return -ENOMEM;
    }
    // cand is exact (next_cand of the previous level) when the states are
    // materialised; a deferred level's is estimated, and a level past the
    // estimate (DF_CAPACITY, a full candidate list or table) is redone on
    // the exact path
    lp.dfr = defer_now_ && c.level > exact_until_;
    if (c.mat && c.n) c.ratio = std::max(1.0, (double)c.cand / (double)c.n);
    lp.bound = c.mat ? c.cand
                     : std::min<uint64_t>((uint64_t)((double)c.n * c.ratio * defer_slack_) + 4096,
                                          (uint64_t)M::MAXSUCC * c.n);
    lp.use_link = !cfg_.keep_trace || cfg_.trace_host;
    if (lp.dfr) {
      if (!c.mat) KC_TRY(cur_.grow(c.n, st_));   // (free: the previous frontier is in next_)
      KC_TRY(pc_cur_.grow(c.n, st_));
      if (lp.use_link) KC_TRY(link_next_.grow(std::max<uint64_t>(lp.bound, 1), st_));
    } else {
      KC_TRY(next_.grow(c.cand ? c.cand : 1, st_));
    }
    lp.next_gidx = c.level_gidx + c.n;
    if (cfg_.keep_trace) KC_TRY(tf_.grow(cfg_.trace_host, lp.next_gidx + lp.bound + 1, st_, true));
    // (a deferred level reserves for 16 new states per parent at least:
    // (count + 16 n) * 2 <= capacity keeps even MAXSUCC = 32 per parent
    // from filling the table, whatever the estimate)
    if (!spill_) KC_TRY(cs_.reserve(c.mat ? lp.bound : std::max<uint64_t>(lp.bound, 16 * c.n), st_));
    KC_TRY(size_chunk_buffers(std::min(c.n, chunk), lp.bound, c.level, c.n));
    lp.df = c.mat ? DeferArgs{} : defer_args(c.level_gidx, c.prev_gidx);
    if (lp.dfr) lp.df.counts_out = pc_cur_;   // this level's plans, for the next level's rebuild
    if (!c.mat) res->deferred_states += c.n;
    lp.link_cap = ~0ull;
    if (lp.dfr) {
      if (lp.use_link) lp.link_cap = link_next_.cap;
      if (cfg_.keep_trace) lp.link_cap = std::min<uint64_t>(lp.link_cap, tf_.cap() - lp.next_gidx);
    }
    if (defer_now_)      // (after this level's ClaimSet growth: a rehash later rules out a redo from here)
      hs_[c.level % 3] = HostSnap{c, cs_.count, res->distinct, res->peak_frontier, cs_.nslots, res->nlevels};
    lp.succ_level = (uint32_t)c.level + 1;
    return 0;
  }

  ClaimBufs claim_bufs() const { return ClaimBufs{abl_mask_, rcount_, rec_fp_, rec_lk_, newmask_, d_ctr_}; }
  // k_claim<M, ABL, false, 0, false, FIRST, C8> over cn parents at cur (the
  // chunk that begins at parent `start` of the level)
  template <int ABL = 0, bool FIRST = false, bool C8 = false>
  void claim(const State* cur, uint64_t cn, uint64_t start, unsigned tiles, uint32_t succ_level, const ShardArgs& sh,
             const DeferArgs& df = DeferArgs{}) {
    launch_claim<M, ABL, false, 0, false, FIRST, C8>(st_, tiles, 0, cur, cn, start, flags_, cfg_.check_deadlock, cs_,
                                                     succ_level, claim_bufs(), sh, df);
  }

  // One chunk's launches: parents [start, start + cn) of the level.
  int launch_chunk(const LevelCursor& c, const LevelPlan& lp, uint64_t start, uint64_t cn) {
    const unsigned grid = (unsigned)((cn + 255) / 256);
    const unsigned tiles = (unsigned)((cn + CLAIM_TILE - 1) / CLAIM_TILE);
    const uint32_t succ_level = lp.succ_level;
    // first-claim levels with the link emit: tile counts summed per chunk
    // of CSUM_TILES tiles by k_claim, k_chunk_scan over the chunks
    // (KC_CHUNK_SCAN=0: k_tile_scan over every tile)
    const bool cscan = first_claim_ && chunk_scan_ && tscan_ && lp.dfr;
    const unsigned nchunk = (tiles + CSUM_TILES - 1) / CSUM_TILES;
    timed(KK_EXPAND, [&] {
      if (first_claim_) {
        ShardArgs fa = claim_args_;
        fa.ttot = ttot_;
        if (cscan) fa.csum = csum_;
        if (cs_.compact)
          claim<0, true, true>(cur_ + start, cn, start, tiles, succ_level, fa, lp.df);
        else
          claim<0, true>(cur_ + start, cn, start, tiles, succ_level, fa, lp.df);
      } else {
        claim(cur_ + start, cn, start, tiles, succ_level, claim_args_, lp.df);
      }
    });
    if (ablate_) KC_TRY(ablate_claims(start, cn, tiles, succ_level));
    // coverage: the chunk's parents are in cur_ (a deferred level's k_claim has just rebuilt and stored them)
    if (cover_on_) KC_TRY(cover_count(start, cn));
    if (pred_on_) KC_TRY(pred_count(start, cn));
    // (a small chunk: the overflow list's pass B inside the tile scan's launch)
    const bool fuse = tscan_ && cn <= FUSE_OVF_SCAN_MAX && !first_claim_;
    if (!first_claim_)
      timed(KK_RESOLVE,
            [&] { launch_settle(cn, start, tiles, succ_level, tscan_ ? ttot_.p : (uint32_t*)nullptr, fuse); });
    if (cscan) {
      timed(KK_SCAN, [&] {
        hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, csum_.p, nchunk, toff_.p, tscan_reg_);
      });
    } else if (tscan_) {
      timed(KK_SCAN, [&] {
        if (fuse)
          hipLaunchKernelGGL(k_ovf_tile_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, claim_args_.ovf, cn, start,
                             cs_.t, cs_.nslots, succ_level, newmask_.p, d_ctr_.p, ClaimKeys(0u), ttot_.p, tiles,
                             toff_.p, tscan_reg_);
        else
          hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, ttot_.p, tiles, toff_.p, tscan_reg_);
      });
    } else {
      KC_TRY(scan_newmask(cn));
    }
    if (spill_) KC_TRY(spill_check(cur_ + start, cn, tiles));
    const uint32_t* toff = tscan_ ? toff_.p : nullptr;
    // cut-down k_emit variants on scratch counters, before the real launch
    // (which rewrites whatever they stored)
    if (ablate_) KC_TRY(ablate_emits(c, lp, start, cn, grid, toff));
    timed(KK_EMIT, [&] {
      if (lp.dfr)
        hipLaunchKernelGGL(k_emit_links, dim3((tiles + EMIT_TPB - 1) / EMIT_TPB), dim3(256), 0, st_, cn, start,
                           newmask_.p, toff_.p, c.level_gidx, lp.next_gidx,
                           cfg_.keep_trace ? tf_.parent() : nullptr, cfg_.keep_trace ? tf_.ord() : nullptr,
                           lp.use_link ? link_next_.p : nullptr, lp.link_cap, d_ctr_.p,
                           cscan ? ttot_.p : (const uint32_t*)nullptr);
      else
        hipLaunchKernelGGL(k_emit<M>, dim3(grid), dim3(256), 0, st_, cur_ + start, cn, start, flags_, newmask_.p,
                           offsets_.p, next_.p, 0ull, c.level_gidx, lp.next_gidx, tf_.parent(), tf_.ord(),
                           cfg_.keep_trace, d_ctr_.p, toff);
    });
    const bool last = start + cn >= c.n;
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(K_ADVANCE_THREADS), 0, st_, offsets_.p, newmask_.p, cn, d_ctr_.p,
                       tscan_ ? toff_.p : (const uint32_t*)nullptr, (uint64_t)(cscan ? nchunk : tiles),
                       last && !headcopy_ ? reinterpret_cast<unsigned long long*>(h_ctr_.p) : nullptr,
                       claim_args_.ovf.count,
                       last && defer_now_ && !headcopy_ ? d_snap_[c.level % 3].s : (CtrStripe*)nullptr);
    return 0;
  }

  // KC_TSCAN=0 and the queued path: the per-parent hipcub scan of a chunk's
  // new-state counts into offsets_
  int scan_newmask(uint64_t cn) {
    size_t tmp_bytes = 0;
    const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> newcnt(newmask_.p, NewCount());
    KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, newcnt, offsets_.p, (int)cn, st_));
    KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
    hipError_t scan_err = hipSuccess;
    timed(KK_SCAN, [&] {
      scan_err = hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, newcnt, offsets_.p, (int)cn, st_);
    });
    KC_HIP_TRY(scan_err);
    return 0;
  }

  // After a level's width is known: its place in the result.
  int record_level(kc_result* res, int level, uint64_t n) {
    if (n) {
      if (level > KC_MAX_LEVELS) {
        set_error("kubecheck: more than %d levels", KC_MAX_LEVELS);
        return -ENOMEM;
      }
      res->level_width[level - 1] = n;
      res->nlevels = level;
    }
    return 0;
  }

  // The level's close: head read-back, the redo decision, the error report,
  // the frontier swap and the width bookkeeping.  0: c is the next level to
  // run (after a redo: the level to run again).
  int close_level(kc_result* res, LevelCursor& c, const LevelPlan& lp) {
    const bool dfr = lp.dfr;
    KC_HIP_TRY(hipGetLastError());
    if (headcopy_) {
      KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, kCtrHead, hipMemcpyDeviceToHost, st_));
      hipLaunchKernelGGL(k_level_reset, dim3(1), dim3(64), 0, st_, d_ctr_.p);   // next level's head
    }
    if (cover_on_) KC_TRY(cover_fetch());
    if (pred_on_) KC_TRY(pred_fetch());
    KC_HIP_TRY(hipStreamSynchronize(st_));
    collect_times();
    const Counters& h = *h_ctr_;
    // a deferred level with anything to report: redo exactly, from the level
    // the anomaly belongs to
    // (first-claim mode: an Assert or deadlock key alone is reported below,
    // from the states this k_claim rebuilt into cur_, exactly as the
    // materialising path's k_claim of this level reports it — no redo)
    // (an action-property key is not reported from here: an invariant that a
    // child of the same level violates may have the smaller key, and on the
    // deferred frontier only the next level's rebuild would see it; the redo
    // has both in one err_key)
    const bool key_only = first_claim_ && !h.overflow && !h.batch_used && !h.defer_flags &&
                          (h.err_key & 0xff) != E_ACTION_PROPERTY;
    if (dfr && !key_only && (h.overflow || h.batch_used || h.err_key != ~0ull || h.defer_flags)) {
      // an invariant violation among the states this level rebuilt is
      // the previous level's error (its emit would have found it); the
      // rest (Assert / deadlock keys of this level's parents, a capacity
      // estimate too small) are this level's
      if (h.defer_flags == DF_INVARIANT && !h.overflow && !h.batch_used && defer_direct_) {
        // an invariant violation among this level's rebuilt states and
        // nothing else: reported as the previous level's emit would have
        // (no redo), unless the snapshots it needs are missing
        const int rc = report_deferred_invariant(res, c);
        if (rc < 0) return rc;
        if (rc == 0) {
          finish(res, 0);
          return kRunDone;
        }
      }
      const int X = (h.defer_flags & DF_INVARIANT) ? c.level - 1 : c.level;
      const uint64_t dc_here = h.cand_total - c.cand_total;
      if (!redo_from(X, dc_here, res, c)) return kDeferRetry;
      cover_drop_from(X);            // levels X.. run again and are counted then
      pred_drop_from(X);
      pc_valid_ = false;
      return 0;
    }
    if (h.overflow || h.batch_used) {
      set_error("kubecheck: state with more than %d successors or full table", M::MAXSUCC);
      return -ENOMEM;
    }
    const uint64_t n_new = h.chunk_base;
    cs_.count = spill_ ? hot_count_ : cs_.count + n_new;
    res->peak_frontier = std::max<uint64_t>(res->peak_frontier, c.n);
    if (pred_on_) {
      // this level's own violation comes before anything its expansion found
      pred_commit(c.level);
      if (pred_violated()) {
        KC_TRY(pred_report(res, c.level, c.level_gidx, c.n));
        res->distinct += n_new;
        KC_TRY(record_level(res, c.level + 1, n_new));
        finish(res, 0);
        return kRunDone;
      }
    }
    if (h.err_key != ~0ull) {
      KC_TRY(report_error(res, h.err_key, c.level, c.level_gidx, c.n));
      res->distinct += n_new;
      finish(res, 0);
      return kRunDone;
    }
    res->distinct += n_new;
    if (cover_on_) cover_commit(c.level);
    if (cfg_.verbose)
      fprintf(stderr, "kubecheck: level %d width %llu -> %llu new, %llu distinct\n",
              c.level, (unsigned long long)c.n, (unsigned long long)n_new,
              (unsigned long long)res->distinct);
    if (!dfr && capture_level_ == c.level + 1 && n_new) {
      captured_.resize(n_new);
      KC_HIP_TRY(hipMemcpy(captured_.data(), next_, n_new * sizeof(State), hipMemcpyDeviceToHost));
    }
    // successors counted this level: the new states' (materialising emit),
    // or this level's own (a deferred k_claim)
    const uint64_t dc = h.cand_total - c.cand_total;
    c.cand_total = h.cand_total;
    if (defer_now_) {              // this level's counters (k_advance) and successor count, for a redo
      if (!headcopy_) snap_lv_[c.level % 3] = c.level;
      succ_[c.level % 3] = c.mat ? c.cand : dc;
      succ_lv_[c.level % 3] = c.level;
    }
    if (dfr) {
      if (!c.mat && c.n) c.ratio = std::max(1.0, (double)dc / (double)c.n);
      c.cand = 0;
      c.prev_gidx = c.level_gidx;
      c.mat = false;
      if (lp.use_link) link_cur_.swap(link_next_);
      pc_cur_.swap(pc_prev_);
      pc_valid_ = true;
    } else {
      c.cand = dc;
    }
    c.level_gidx = lp.next_gidx;
    cur_.swap(next_);
    c.n = n_new;
    ++c.level;
    if (dfr && capture_level_ == c.level && c.n) {
      KC_TRY(materialize(c));
      c.mat = true;
      KC_TRY(counter_snap(c.level - 1));
      captured_.resize(c.n);
      KC_HIP_TRY(hipMemcpy(captured_.data(), cur_, c.n * sizeof(State), hipMemcpyDeviceToHost));
    }
    return record_level(res, c.level, c.n);
  }

  // ---- KC_ABLATE=1: cut-down variants of k_claim and k_emit, timed next to
  // the real launches, and their printout
  int ablate_claims(uint64_t start, uint64_t cn, unsigned tiles, uint32_t succ_level) {
    KC_TRY(abl_mask_.grow(cn, st_));
    timed(KA_LDS, [&] { claim<1>(cur_ + start, cn, start, tiles, succ_level, claim_args_); });
    timed(KA_COMPUTE, [&] { claim<2>(cur_ + start, cn, start, tiles, succ_level, claim_args_); });
    timed(KA_PLAN, [&] { claim<3>(cur_ + start, cn, start, tiles, succ_level, claim_args_); });
    timed(KA_FPCHEAP, [&] { claim<4>(cur_ + start, cn, start, tiles, succ_level, claim_args_); });
    timed(KA_NOAPPLY, [&] { claim<5>(cur_ + start, cn, start, tiles, succ_level, claim_args_); });
    return 0;
  }
  template <int ABL>
  void ablate_emit(const LevelCursor& c, const LevelPlan& lp, uint64_t start, uint64_t cn, unsigned grid,
                   const uint32_t* toff) {
    hipLaunchKernelGGL((k_emit<M, ABL>), dim3(grid), dim3(256), 0, st_, cur_ + start, cn, start, flags_, newmask_.p,
                       offsets_.p, next_.p, 0ull, c.level_gidx, lp.next_gidx, tf_.parent(), tf_.ord(), cfg_.keep_trace,
                       d_ctr_abl_.p, toff);
  }
  int ablate_emits(const LevelCursor& c, const LevelPlan& lp, uint64_t start, uint64_t cn, unsigned grid,
                   const uint32_t* toff) {
    KC_TRY(d_ctr_abl_.alloc(1));
    KC_HIP_TRY(hipMemsetAsync(d_ctr_abl_, 0, sizeof(Counters), st_));
    timed(KA_E1, [&] { ablate_emit<1>(c, lp, start, cn, grid, toff); });
    timed(KA_E2, [&] { ablate_emit<2>(c, lp, start, cn, grid, toff); });
    timed(KA_E3, [&] { ablate_emit<3>(c, lp, start, cn, grid, toff); });
    return 0;
  }
  int ablate_report() {
    fprintf(stderr, "kubecheck ablate: claim %.2f ms | successors+LDS %.2f ms | successors only %.2f ms | plan only %.2f ms | settle %.2f | emit %.2f ms"
            " | emit-no-plan %.2f | emit-no-plan-no-check %.2f | emit-parent-only %.2f"
            " | successors, XOR fingerprint %.2f | fingerprints, no apply %.2f\n",
            ktime_ms_[KK_EXPAND], ktime_ms_[KA_LDS], ktime_ms_[KA_COMPUTE], ktime_ms_[KA_PLAN], ktime_ms_[KK_RESOLVE],
            ktime_ms_[KK_EMIT], ktime_ms_[KA_E1], ktime_ms_[KA_E2], ktime_ms_[KA_E3], ktime_ms_[KA_FPCHEAP],
            ktime_ms_[KA_NOAPPLY]);
    KC_HIP_TRY(hipMemcpy(h_ctr_, d_ctr_, sizeof(Counters), hipMemcpyDeviceToHost));
    fprintf(stderr, "kubecheck claim outcomes (KC_DIAG builds): old %llu lost %llu cur %llu new %llu\n",
            h_ctr_->claim_out(0), h_ctr_->claim_out(1), h_ctr_->claim_out(2), h_ctr_->claim_out(3));
    fprintf(stderr, "kubecheck old-state level distance (KC_DIAG): 1:%llu 2:%llu 3:%llu 4:%llu 5-8:%llu 9-16:%llu 17+:%llu\n",
            h_ctr_->old_dist(0), h_ctr_->old_dist(1), h_ctr_->old_dist(2), h_ctr_->old_dist(3), h_ctr_->old_dist(4),
            h_ctr_->old_dist(5), h_ctr_->old_dist(6));
    fprintf(stderr, "kubecheck k_claim successor loop (KC_DIAG): wave trips %llu x 64 lanes, lane trips %llu (%.3f busy);"
            " dealt by successor count: wave trips %llu (%.3f busy)\n",
            h_ctr_->loop_max(), h_ctr_->loop_sum(),
            h_ctr_->loop_max() ? (double)h_ctr_->loop_sum() / (64.0 * h_ctr_->loop_max()) : 0.0,
            h_ctr_->loop_sorted(),
            h_ctr_->loop_sorted() ? (double)h_ctr_->loop_sum() / (64.0 * h_ctr_->loop_sorted()) : 0.0);
    return 0;
  }

  size_t trace_text(char* buf, size_t cap) const override;

  // TLC checkFPs over the ClaimSet's fingerprints: compact, radix-sort,
  // minimum adjacent gap (MC.out:42 "based on the actual fingerprints").
  int check_fps(uint64_t* min_gap, double* prob) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    if (spill_) return check_fps_spill(min_gap, prob);
    const uint64_t cnt = std::max<uint64_t>(cs_.count, 2);
    DeviceArray<unsigned long long> a, b, d_n;
    DeviceArray<uint8_t> tmp;
    int rc = 0;
    unsigned long long n = 0, gap = ~0ull;
    if (a.alloc(cnt) < 0 || b.alloc(cnt) < 0 || d_n.alloc(2) < 0) {
      set_error("kc_engine_check_fps: out of device memory");
      rc = -ENOMEM;
    }
    if (!rc) {
      (void)hipMemsetAsync(d_n, 0, 8, st_);
      (void)hipMemcpyAsync(d_n + 1, &gap, 8, hipMemcpyHostToDevice, st_);
      hipLaunchKernelGGL(k_claimset_fps, dim3(table_grid(cs_.nslots)), dim3(256), 0, st_,
                         cs_.words(), cs_.nslots, cs_.word_shift(), a.p, cnt, d_n.p);
      (void)hipMemcpyAsync(&n, d_n, 8, hipMemcpyDeviceToHost, st_);
      if (hipStreamSynchronize(st_) != hipSuccess || n > cnt) {
        set_error("kc_engine_check_fps: fingerprint count %llu > %llu", n, (unsigned long long)cnt);
        rc = -EIO;
      }
    }
    if (!rc && n > 1) {
      size_t tb = 0;
      if (hipcub::DeviceRadixSort::SortKeys(nullptr, tb, a.p, b.p, (int)n, 0, 64, st_) != hipSuccess ||
          tmp.alloc(tb) < 0) {
        set_error("kc_engine_check_fps: sort setup");
        rc = -EIO;
      } else {
        (void)hipcub::DeviceRadixSort::SortKeys(tmp.p, tb, a.p, b.p, (int)n, 0, 64, st_);
        hipLaunchKernelGGL(k_adjacent_min_gap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st_, b.p, n,
                           d_n + 1);
        (void)hipMemcpyAsync(&gap, d_n + 1, 8, hipMemcpyDeviceToHost, st_);
        if (hipStreamSynchronize(st_) != hipSuccess) {
          set_error("kc_engine_check_fps: HIP failure");
          rc = -EIO;
        }
      }
    }
    if (rc) return rc;
    *min_gap = gap;
    *prob = (n > 1 && gap && gap != ~0ull) ? 1.0 / (double)gap : 0.0;
    return 0;
  }
  // the same over hot + cold tiers, on the host (cold keys are mixed
  // fingerprints: unmixed, merged with the hot table's, sorted)
  int check_fps_spill(uint64_t* min_gap, double* prob) {
    std::vector<uint64_t> keys;
    KC_TRY(sp_.cold.all_keys(keys));
    uint64_t* hk = reinterpret_cast<uint64_t*>(sp_.arena.p);
    KC_HIP_TRY(hipMemsetAsync(sp_.d_spctr + 1, 0, 8, st_));
    hipLaunchKernelGGL(k_claimset_keys, dim3(table_grid(cs_.nslots)), dim3(256), 0, st_, cs_.t,
                       cs_.nslots, hk, sp_.hot_limit, sp_.d_spctr + 1);
    KC_HIP_TRY(hipMemcpyAsync(sp_.h_spctr, sp_.d_spctr, 16, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    const uint64_t c = std::min<uint64_t>(sp_.h_spctr[1], sp_.hot_limit);
    const size_t at = keys.size();
    keys.resize(at + c);
    if (c) KC_HIP_TRY(hipMemcpy(keys.data() + at, hk, c * 8, hipMemcpyDeviceToHost));
    for (auto& k : keys) k = cold_unkey(k);
    std::sort(keys.begin(), keys.end());
    uint64_t gap = ~0ull;
    for (size_t i = 1; i < keys.size(); ++i) gap = std::min<uint64_t>(gap, keys[i] - keys[i - 1]);
    *min_gap = gap;
    *prob = (keys.size() > 1 && gap && gap != ~0ull) ? 1.0 / (double)gap : 0.0;
    return 0;
  }
  int trace_tuple(int i, uint64_t* out) const override {
    if (i < 0 || i >= (int)trace_.size()) {
      set_error("trace index out of range");
      return -EINVAL;
    }
    M::to_tuple(trace_[i], out);
    return M::TUPLE_WORDS;
  }
  int64_t level_tuples(int level, uint64_t* out, uint64_t cap) override {
    if (level == capture_level_ && !captured_.empty()) {
      for (uint64_t i = 0; i < captured_.size() && i < cap; ++i)
        M::to_tuple(captured_[i], out + i * M::TUPLE_WORDS);
      return (int64_t)captured_.size();
    }
    if (level == 1) {
      for (uint64_t i = 0; i < init_states_.size() && i < cap; ++i)
        M::to_tuple(init_states_[i], out + i * M::TUPLE_WORDS);
      return (int64_t)init_states_.size();
    }
    set_error("level %d not captured", level);
    return -EINVAL;
  }

 private:
  template <class F>
  void timed(int k, F&& f) {
    // (timing 2: events bracket the roofline kernel only; ten events per
    // level cost the NP=2 check 6 ms and Model_1 4 ms of host/queue time)
    if (timing_ == 1 || (timing_ == 2 && (k == KK_EXPAND || k == KK_NARROW))) {
      if (ev_used_ + 2 > ev_pool_.size()) {
        ev_pool_.resize(ev_used_ + 2);
        (void)ev_pool_[ev_used_].create();
        (void)ev_pool_[ev_used_ + 1].create();
      }
      hipEvent_t a = ev_pool_[ev_used_], b = ev_pool_[ev_used_ + 1];
      (void)hipEventRecord(a, st_);
      f();
      (void)hipEventRecord(b, st_);
      ev_kind_.push_back(k);
      ev_used_ += 2;
    } else {
      f();
    }
    ++klaunch_[k];
  }
  // after the level's sync: accumulate every timed launch
  void collect_times() {
    for (size_t q = 0; q < ev_kind_.size(); ++q) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev_pool_[2 * q], ev_pool_[2 * q + 1]) == hipSuccess)
        ktime_ms_[ev_kind_[q]] += ms;
    }
    ev_kind_.clear();
    ev_used_ = 0;
  }

  // parent_host: the parent state when the caller already holds it (the
  // queued path); otherwise it is read from the frontier (cur_)
  int report_error(kc_result* res, uint64_t key, int level, uint64_t level_gidx, uint64_t n,
                   const State* parent_host = nullptr) {
    const int kind = (int)(key & 0xff);
    const int pos = (int)((key >> 8) & 0xff);
    const uint64_t pidx = key >> 16;
    if (pidx >= n) {
      set_error("kubecheck: bad error key");
      return -EIO;
    }
    res->err_kind = kind;
    // path to the parent through the parent pointers (TLC's trace file);
    // without them only the parent itself, still in the current frontier
    std::vector<State> path;
    if (cfg_.keep_trace) {
      KC_TRY(path_to(level_gidx + pidx, path));
    } else if (parent_host) {
      path.assign(1, *parent_host);
    } else {
      path.resize(1);
      KC_HIP_TRY(hipMemcpy(&path[0], cur_ + pidx, sizeof(State), hipMemcpyDeviceToHost));
    }
    const State& s = path.back();
    const typename M::Plan pl = M::plan(s, flags_);
    if (kind == E_ASSERT) {
      res->err_action = M::slot_action(s, pl.fail_slot);
      res->err_self = pl.fail_slot < M::A ? pl.fail_slot
                      : pl.fail_slot < 2 * M::A ? pl.fail_slot - M::A
                                               : M::A + (pl.fail_slot - 2 * M::A);
      res->err_level = level;
    } else if (kind == E_INVARIANT) {
      int slot, j;
      M::locate(pl, pos, slot, j);
      State x;
      M::apply(s, slot, j, flags_, x);
      res->err_invariant = M::check(x, flags_.inv_mask);
      path.push_back(x);
      res->err_level = level + 1;
    } else if (kind == E_ACTION_PROPERTY) {
      // the step s -> x that violates the property: the behaviour is the
      // path to s, then x (which may be a state seen levels ago)
      int slot, j;
      M::locate(pl, pos, slot, j);
      State x;
      M::apply(s, slot, j, flags_, x);
      const unsigned bad = M::step_violations(s, x, slot, flags_);
      if (!bad) {
        set_error("kubecheck: the step of an action-property error key violates none");
        return -EIO;
      }
      res->err_invariant = ctz(bad);
      res->err_action = M::slot_action(s, slot);
      res->err_self = slot < M::A ? slot : slot < 2 * M::A ? slot - M::A : M::A + (slot - 2 * M::A);
      path.push_back(x);
      res->err_level = level + 1;
    } else {
      res->err_level = level;
    }
    if (cfg_.keep_trace) {
      trace_ = path;
      res->trace_len = (int)path.size();
    }
    return 0;
  }

  // Rebuild the states on the path to global state index g by walking the
  // parent pointers (TLC's trace file) and replaying successors on the host.
  int path_to(uint64_t g, std::vector<State>& out) {
    if (!cfg_.keep_trace) {
      set_error("kubecheck: trace requested but keep_trace=0");
      return -EINVAL;
    }
    std::vector<std::pair<uint64_t, uint8_t>> chain;
    if (cfg_.trace_host) {
      KC_HIP_TRY(hipStreamSynchronize(st_));
      for (;;) {
        const unsigned long long p = tf_.parent()[g];
        chain.push_back({g, tf_.ord()[g]});
        if (p == ~0ull) break;
        g = p;
        if (chain.size() > KC_MAX_LEVELS + 2) {
          set_error("kubecheck: corrupt parent chain");
          return -EIO;
        }
      }
    } else {
      // one lane walks the chain in HBM, one readback (instead of two
      // synchronous 8-B copies per level: the time to a counterexample)
      constexpr uint32_t cap = KC_MAX_LEVELS + 3;
      KC_TRY(h_chain_.alloc(cap + 1));
      hipLaunchKernelGGL(k_parent_chain, dim3(1), dim3(64), 0, st_, tf_.parent(), tf_.ord(), (uint64_t)g,
                         h_chain_ + 1, cap, h_chain_.p);
      KC_HIP_TRY(hipGetLastError());
      KC_HIP_TRY(hipStreamSynchronize(st_));
      const uint64_t len = h_chain_[0];
      if (len == 0 || len > cap) {
        set_error("kubecheck: corrupt parent chain");
        return -EIO;
      }
      for (uint64_t k = 0; k < len; ++k) chain.push_back({h_chain_[1 + k] >> 8, (uint8_t)(h_chain_[1 + k] & 0xff)});
    }
    std::reverse(chain.begin(), chain.end());
    out.clear();
    out.push_back(init_states_.at(chain[0].second));
    for (size_t k = 1; k < chain.size(); ++k) {
      const State& s = out.back();
      const typename M::Plan pl = M::plan(s, flags_);
      int slot, j;
      M::locate(pl, chain[k].second, slot, j);
      State x;
      M::apply(s, slot, j, flags_, x);
      out.push_back(x);
    }
    return 0;
  }

  void finish(kc_result* res, uint64_t left) {
    // the striped totals are read once, at the end (levels read only the head)
    if (hipMemcpy(h_ctr_, d_ctr_, sizeof(Counters), hipMemcpyDeviceToHost) != hipSuccess)
      set_error("kubecheck: counter readback failed");
    uint64_t gen = 0;
    for (int a = 0; a < A_COUNT; ++a) {
      res->act_gen[a] = h_ctr_->act_gen(a);
      res->act_dist[a] = h_ctr_->act_dist(a);
      gen += res->act_gen[a];
    }
    res->generated = res->init + gen;
    res->depth = res->nlevels;
    res->queue_left = left;
    res->cut_state = h_ctr_->cut_state() + init_cut_;
    res->cut_action = h_ctr_->cut_action();
    res->step_checked = h_ctr_->step_checked();
    for (int k = 0; k < AP_COUNT; ++k) res->step_violations[k] = h_ctr_->step_violations(k);
    res->complete = (left == 0 && res->err_kind == 0 && !(cfg_.max_levels && res->nlevels >= cfg_.max_levels && left));
    const double d = (double)res->distinct, gg = (double)res->generated;
    res->collision_optimistic = d * (gg - d) / 18446744073709551616.0;
    res->fpset_slots = cs_.capacity();
    res->fpset_probes = h_ctr_->probes() + narrow_probes_;
    for (int b = 0; b < OUTDEG_BINS; ++b) res->outdeg_hist[b] = h_ctr_->outdeg(b);
    res->batch_inserts = h_ctr_->settles();
    res->cand_overflow_records = h_ctr_->cand_ovf();
    res->cand_buffer_peak_bytes = cand_buf_peak_;
    res->narrow_levels = narrow_levels_;
    if (spill_) {
      ColdStats cst;
      sp_.cold.stats(&cst);
      unsigned long long hits = 0;
      if (hipMemcpy(&hits, sp_.d_spctr, 8, hipMemcpyDeviceToHost) != hipSuccess) set_error("kubecheck: spill counter readback");
      res->seen_flushes = sp_.flushes;
      res->seen_cold_fps = cst.keys;
      res->seen_cold_queries = sp_.queries;
      res->seen_cold_hits = hits;
      res->seen_cold_runs = cst.runs;
      res->seen_disk_bytes = cst.disk_written;
      res->seen_peak_hbm_bytes = cs_.nslots * cs_.slot_bytes() + sp_.arena.cap + cst.peak_meta_bytes;
      res->seen_filter_tests = cst.filter_tests;
      res->seen_filter_passed = cst.filter_passed;
      res->seen_merges = cst.merges;
      res->seen_seconds = sp_seconds_;
      res->seen_flush_seconds = sp_flush_seconds_;
      res->seen_merge_seconds = cst.merge_seconds;
      res->seen_check_seconds = sp_check_seconds_;
      if (cfg_.verbose)
        fprintf(stderr, "kubecheck seen-set spill: %.3f s host (flushes %.3f: pin %.3f merge %.3f meta+copy %.3f files %.3f;"
                        " checks %.3f), %llu flushes, %llu runs (%llu with %llu keys in HBM), %llu merges, %.1f GB uploaded,"
                        " %llu streaming merge-probes\n",
                sp_seconds_, sp_flush_seconds_, cst.pin_seconds, cst.merge_seconds, cst.meta_seconds, cst.evict_seconds,
                sp_check_seconds_, (unsigned long long)sp_.flushes, (unsigned long long)cst.runs,
                (unsigned long long)cst.cached_runs, (unsigned long long)cst.cached_keys,
                (unsigned long long)cst.merges, cst.cache_uploaded / 1e9, (unsigned long long)cst.merge_probes);
    }
    if (q_) {
      kc_squeue_stats qs;
      q_->stats(&qs);
      res->frontier_spilled_bytes = qs.spilled_host_bytes + qs.spilled_disk_bytes;
      res->frontier_reloaded_bytes = qs.reloaded_bytes;
      res->frontier_peak_hbm_bytes = qs.peak_hbm_bytes;
    }
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count();
  }

  // One launch of k_narrow from the host loop's state; on return the
  // engine's cur_ holds the frontier of level nr.level.
  struct NarrowRun {
    uint64_t new_total = 0, peak = 0;
    int levels = 0, reason = 0;
    bool counted = false;          // coverage: k_cover ran over the run's first level
  };
  int run_narrow(LevelCursor& c, int stop, NarrowRun& nr) {
    const uint64_t n = c.n, level_gidx = c.level_gidx, cand = c.cand;
    const int level = c.level;
    constexpr uint64_t kBuf = 1ull << 16;            // frontier room (states) of a narrow run
    constexpr uint64_t kNew = 1ull << 20;            // new states one run may add
    const uint64_t bufs = std::max(cand, kBuf);
    KC_TRY(cur_.grow(bufs, st_, true));
    KC_TRY(next_.grow(bufs, st_));
    const uint64_t need_par = level_gidx + n + std::max(cand, kNew) + 1;
    if (cfg_.keep_trace) KC_TRY(tf_.grow(cfg_.trace_host, need_par, st_, true));
    KC_TRY(cs_.reserve(std::max(cand, kNew), st_));
    NarrowCtl& h = *h_ns_;
    memset(&h, 0, offsetof(NarrowCtl, widths));
    h.n = n;
    h.level_gidx = level_gidx;
    h.cand = cand;
    h.level = (uint32_t)level;
    h.cur_is_b = 0;
    h.buf_cap = std::min(cur_.cap, next_.cap);
    h.par_cap = cfg_.keep_trace ? tf_.cap() : ~0ull;
    h.room = cs_.capacity() / 2 > cs_.count ? cs_.capacity() / 2 - cs_.count : 0;
    h.stop_level = (uint32_t)stop;
    h.err[0] = h.err[1] = ~0ull;
    h.epoch = ++narrow_epoch_;
    h.reason = narrow_exit_reason(h);
    h.active = h.reason == 0;
    nr = NarrowRun{};
    if (!h.active) {                             // this level cannot run narrow (c stays)
      nr.reason = h.reason;
      return 0;
    }
    KC_HIP_TRY(hipMemcpyAsync(d_ns_, h_ns_, offsetof(NarrowCtl, widths), hipMemcpyHostToDevice, st_));
    // both level tables clear (the last level of the previous run left one dirty)
    KC_HIP_TRY(hipMemsetAsync(d_nsc_, 0, sizeof(NarrowScratch), st_));
    if (env_flag("KC_NARROW_TRACE", false)) KC_TRY(d_ntrace_.alloc(kNtraceBytes / 8));
    if (d_ntrace_) KC_HIP_TRY(hipMemsetAsync(d_ntrace_, 0, kNtraceBytes, st_));
    // NARROW_BATCH levels' launches per host sync; they all read the control
    // block, so the ones after the run has ended return at once
    State *a = cur_.p, *b = next_.p;
    uint32_t lev = 0;                            // level launches enqueued in this run
    if (cover_on_) {
      KC_TRY(cover_count(0, n));
      nr.counted = true;
    }
    if (pred_on_) {
      KC_TRY(pred_count(0, n));
      nr.counted = true;
    }
    // the run's first level is expanded on its own; every k_nfinish then
    // expands the states it emits for the level after it
    hipLaunchKernelGGL(k_nexpand<M>, dim3(NARROW_WG * NARROW_SUB), dim3(NARROW_THREADS), 0, st_, a, b, flags_,
                       cfg_.check_deadlock, 0u, d_ns_.p, d_nsc_.p, d_ctr_.p, d_ntrace_.p);
    for (;;) {
      // (round 6 captured a batch's launches into a hipGraph, replayed with
      // one hipGraphLaunch: Model_1 2.79-2.82 ms against 2.80 — the cost of
      // a level is its in-kernel chain, not the launches; removed,
      // profiles/r06g_model1_narrow_graph_ab.log)
      timed(KK_NARROW, [&] {
        // (coverage: the run stops after its first level, which one k_nfinish closes)
        for (int k = 0; k < (cover_on_ || pred_on_ ? 1 : narrow_batch_); ++k, ++lev)
          hipLaunchKernelGGL(k_nfinish<M>, dim3(NARROW_FWG), dim3(NARROW_THREADS), 0, st_, a, b, flags_,
                             cfg_.check_deadlock, tf_.parent(), tf_.ord(), cfg_.keep_trace, lev, d_ns_.p, d_nsc_.p,
                             cs_.t, cs_.nslots, d_ctr_.p, d_ntrace_.p, cs_.word_shift());
      });
      KC_HIP_TRY(hipGetLastError());
      KC_HIP_TRY(hipMemcpyAsync(h_ns_, d_ns_, offsetof(NarrowCtl, close_acc), hipMemcpyDeviceToHost, st_));
      KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, kCtrHead, hipMemcpyDeviceToHost, st_));
      KC_HIP_TRY(hipStreamSynchronize(st_));
      if (h_ctr_->overflow) {
        set_error("kubecheck: state with more than %d successors", M::MAXSUCC);
        return -ENOMEM;
      }
      if (!h.active) break;
    }
    collect_times();
    if (d_ntrace_) KC_TRY(print_ntrace(lev));
    KC_HIP_TRY(hipMemcpy(h_ns_->widths + level, d_ns_->widths + level,
                         sizeof(uint64_t) * std::min<uint64_t>(h.levels + 1, KC_MAX_LEVELS - level),
                         hipMemcpyDeviceToHost));
    c.n = h.n;
    c.level_gidx = h.level_gidx;
    c.cand = h.cand;
    c.level = (int)h.level;
    nr.levels = (int)h.levels;
    nr.reason = h.reason;
    nr.new_total = h.new_total;
    nr.peak = 0;
    for (int L = level; L < c.level && L < KC_MAX_LEVELS; ++L) nr.peak = std::max<uint64_t>(nr.peak, h.widths[L]);
    if (nr.reason == NX_ERROR) h_ctr_->err_key = h.err_key;
    cs_.count += h.new_total;
    narrow_levels_ += h.levels;
    narrow_probes_ += h.probes;
    if (h.cur_is_b) cur_.swap(next_);
    return 0;
  }

  // Deferred frontier: the rebuild arguments of the level starting at global
  // index level_gidx, whose parents (the previous frontier, from prev_gidx)
  // are in next_; the states go to cur_.
  DeferArgs defer_args(uint64_t level_gidx, uint64_t prev_gidx) const {
    DeferArgs df;
    df.prev = next_.p;
    df.out = cur_.p;
    if (!cfg_.keep_trace || cfg_.trace_host) {
      df.link = link_cur_;
    } else {
      df.parent = tf_.parent();
      df.ord = tf_.ord();
      df.gidx0 = level_gidx;
      df.prev_gidx0 = prev_gidx;
    }
    if (pc_valid_) df.prev_counts = pc_prev_;
    return df;
  }
  // Materialise a deferred frontier of n states into cur_ (k_materialize):
  // invariants checked (a violation -> kDeferRetry), actions counted, and
  // the exact successor count of the level into c.cand.
  int materialize(LevelCursor& c) {
    KC_TRY(cur_.grow(c.n, st_));
    const DeferArgs df = defer_args(c.level_gidx, c.prev_gidx);
    hipLaunchKernelGGL(k_materialize<M>, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, st_, df, c.n, flags_,
                       d_ctr_.p);
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, sizeof(Counters), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    if (h_ctr_->defer_flags) return kDeferRetry;
    const uint64_t tot = h_ctr_->next_cand();
    c.cand = tot - c.cand_total;
    c.cand_total = tot;
    return 0;
  }

  // The chunk's candidate overflow list (engine_kernels.h CandOvf), sized by
  // the level's successor count `bound` (no chunk of the level has more), and
  // the peak of the candidate buffers (verbose: per level).
  int cand_overflow(uint64_t bound, int level, uint64_t n) {
    bound = std::max<uint64_t>(bound, 1);
    KC_TRY(ovf_fp_.grow_tight(bound, st_));
    KC_TRY(ovf_lk_.grow_tight(bound, st_));
    KC_TRY(ovf_tile_.grow_tight(bound, st_));
    // empty when allocated and at every run's start (run(); a run that
    // stopped mid-level may have left entries); k_advance empties it again
    // after every chunk, so a level needs no reset launch of its own
    if (!d_ovf_cnt_) {
      KC_TRY(d_ovf_cnt_.alloc(1));
      KC_HIP_TRY(hipMemsetAsync(d_ovf_cnt_, 0, 8, st_));
    }
    claim_args_.ovf = CandOvf{d_ovf_cnt_, ovf_fp_, ovf_lk_, ovf_tile_,
                              std::min(ovf_fp_.cap, std::min(ovf_lk_.cap, ovf_tile_.cap))};
    const uint64_t b = rcount_.cap * 4 + rec_fp_.cap * 8 + rec_lk_.cap * 4 + ovf_fp_.cap * 8 + ovf_lk_.cap * 4 +
                       ovf_tile_.cap * 4;
    cand_buf_peak_ = std::max(cand_buf_peak_, b);
    if (cfg_.verbose)
      fprintf(stderr, "kubecheck: level %d width %llu: candidate buffers %.1f MiB (%.1f B per parent)\n", level,
              (unsigned long long)n, b / 1048576.0, n ? (double)b / (double)n : 0.0);
    return 0;
  }
  DeviceArray<unsigned long long> ovf_fp_;
  DeviceArray<unsigned int> ovf_lk_, ovf_tile_;
  uint64_t cand_buf_peak_ = 0;
  DeviceArray<unsigned long long> d_ovf_cnt_;
  // deferred frontier (DeferArgs): links of the level being expanded / being
  // emitted, when they are not the (device) trace
  DeviceArray<unsigned long long> link_cur_, link_next_;
  // plans (Plan::counts) of the frontier being expanded / of the previous one
  DeviceArray<unsigned long long> pc_cur_, pc_prev_;
  bool pc_valid_ = false;
  static constexpr int kDeferRetry = -100000;
  bool defer_ = false, defer_now_ = false;
  double defer_slack_ = 1.25;
  uint64_t defer_fallbacks_ = 0;
  // deferred-frontier redo from a level (redo_from): per level mod 3, the
  // counters as the level left them (k_advance), the host state as it began
  // and its states' successor count
  struct HostSnap {
    LevelCursor c;                      // (c.level = -1: none)
    uint64_t cs_count = 0, distinct = 0, peak = 0, nslots = 0;
    int nlevels = 0;
  };
  DeviceArray<Counters> d_snap_;      // [3]
  int snap_lv_[3] = {-1, -1, -1};
  HostSnap hs_[3];
  uint64_t succ_[3] = {0, 0, 0};
  int succ_lv_[3] = {-1, -1, -1};
  int exact_until_ = 0;               // levels <= this run on the exact path (after a redo)
  bool redo_on_ = true;               // KC_DEFER_REDO=0: an anomaly redoes the run from Init
  bool defer_direct_ = true;          // KC_DEFER_DIRECT=0: an invariant anomaly is redone too

  // Level L's k_claim rebuilt a state violating an invariant (and found
  // nothing else): the error TLC reports is the first such state of level L
  // in BFS order, the lowest rebuilt index (defer_inv_n).  The materialising
  // path finds it in level L - 1's emit and stops there, so the result is
  // put back as that emit left it: counters of level L - 1 (its k_advance
  // snapshot) with level L's per-action distinct counts (counted here by the
  // rebuild), level L's claims of level L + 1 dropped from the ClaimSet, L - 1
  // levels expanded; the trace is the path to the state through the parent
  // pointers.  1: not possible here (the caller redoes from L - 1).
  int report_deferred_invariant(kc_result* res, const LevelCursor& c) {
    const int L = c.level;
    const uint64_t level_gidx = c.level_gidx, n = c.n;
    if (!cfg_.keep_trace || headcopy_ || !d_snap_ || L < 2 || snap_lv_[(L - 1) % 3] != L - 1) return 1;
    // (k_advance copied it with the level head and reset it)
    const unsigned long long inv_n = h_ctr_->defer_inv_n;
    if (!inv_n) return 1;
    const uint64_t idx = ~(uint64_t)inv_n;
    if (idx >= n) {
      set_error("kubecheck: deferred invariant index %llu past the level's %llu states", (unsigned long long)idx,
                (unsigned long long)n);
      return -EIO;
    }
    KC_TRY(counter_snap(L));
    hipLaunchKernelGGL(k_counters_restore, dim3(1), dim3(64), 0, st_, d_ctr_.p, d_snap_[(L - 1) % 3].s,
                       d_snap_[L % 3].s);
    // (first-claim mode writes no claim words: there is no level to drop by,
    // and a drop keyed on the empty word would clear every wide-level entry;
    // the run ends here and the next one clears the table)
    if (!first_claim_)
      hipLaunchKernelGGL(k_claimset_drop, dim3(table_grid(cs_.nslots)), dim3(256), 0, st_, cs_.t, cs_.nslots,
                         (uint32_t)L + 1);
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipStreamSynchronize(st_));
    std::vector<State> path;
    KC_TRY(path_to(level_gidx + idx, path));
    res->err_kind = E_INVARIANT;
    res->err_invariant = M::check(path.back(), flags_.inv_mask);
    res->err_level = L;
    res->nlevels = L - 1;
    res->level_width[L - 1] = 0;
    trace_ = path;
    res->trace_len = (int)path.size();
    return 0;
  }

  // The counters after level `lv` (end of a narrow run, or the start) into
  // snapshot lv mod 3.
  int counter_snap(int lv) {
    KC_TRY(d_snap_.alloc(3));
    KC_HIP_TRY(hipMemcpyAsync(d_snap_[lv % 3].s, d_ctr_->s, sizeof(d_ctr_->s), hipMemcpyDeviceToDevice, st_));
    snap_lv_[lv % 3] = lv;
    return 0;
  }
  // Put the run back as level X found it (L = the level that met the
  // anomaly, X = L or L - 1): ClaimSet entries of levels > X dropped,
  // counters of level X - 1 restored (k_counters_restore), the host state of X's start; X's
  // states are cur_ (X = L: k_claim rebuilt or had them) or next_ (X = L -
  // 1: the previous frontier).  Levels <= L then run exactly.  False: not
  // possible exactly (the caller redoes the run from Init).
  // On success c is level X's start, materialised.
  bool redo_from(int X, uint64_t dc_here, kc_result* res, LevelCursor& c) {
    const int L = c.level;
    const bool mat = c.mat;
    if (!redo_on_ || X < 1 || !d_snap_ || snap_lv_[(X - 1) % 3] != X - 1 || hs_[X % 3].c.level != X) return false;
    // level X's own snapshot: X = L - 1 completed; X = L's k_advance wrote it (the anomaly is seen after)
    if (X != L && snap_lv_[X % 3] != X) return false;
    if (X == L && headcopy_) return false;
    const HostSnap& h = hs_[X % 3];
    if (h.nslots != cs_.nslots) return false;      // rehashed since: dropping entries would break probe chains
    uint64_t succ;
    if (X == L) {
      succ = mat ? c.cand : dc_here;               // k_claim rebuilt the states into cur_ and counted them
    } else {
      if (mat || succ_lv_[X % 3] != X) return false;   // (X's states are the previous frontier, next_)
      succ = succ_[X % 3];
    }
    const unsigned grid = (unsigned)std::min<uint64_t>(8192, (cs_.nslots + 255) / 256);
    hipLaunchKernelGGL(k_claimset_drop, dim3(grid), dim3(256), 0, st_, cs_.t, cs_.nslots, (uint32_t)X + 1);
    hipLaunchKernelGGL(k_counters_restore, dim3(1), dim3(64), 0, st_, d_ctr_.p, d_snap_[(X - 1) % 3].s,
                       d_snap_[X % 3].s);
    hipLaunchKernelGGL(k_level_reset, dim3(1), dim3(64), 0, st_, d_ctr_.p);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st_) != hipSuccess) return false;
    if (X != L) cur_.swap(next_);
    c = h.c;                       // (level X, as it began)
    c.cand = succ;
    c.mat = true;
    cs_.count = h.cs_count;
    res->distinct = h.distinct;
    res->peak_frontier = h.peak;
    res->nlevels = h.nlevels;
    exact_until_ = L;
    res->defer_fallback = 1;
    res->defer_redo_level = (uint64_t)X;
    ++defer_fallbacks_;
    return true;
  }

  // ---- seen-set spill (cfg.seen_hbm_bytes > 0; the tier is SeenSpill,
  // engine_spill.h).  The engine's part: the flush never finds more than
  // hot_limit keys, a chunk's cold check takes every winner at once (q_max
  // bounds the chunk: spill_cut), and a location is 32 bits.
  int spill_setup() {
    typename SeenSpill<uint32_t>::Policy pol;
    const uint64_t hot_limit = SeenSpill<uint32_t>::hot_slots(cfg_.seen_hbm_bytes) / 2;
    pol.flush_cap = hot_limit;
    pol.q_max = std::max<uint64_t>(CLAIM_TILE * 32, hot_limit / 3) / 256 * 256;
    pol.who = "kubecheck";
    pol.dir = cfg_.spill_dir ? cfg_.spill_dir : "";
    KC_TRY(sp_.setup(cfg_, cs_, st_, pol));
    hot_count_ = 0;
    sp_seconds_ = sp_flush_seconds_ = sp_check_seconds_ = 0;
    sp_sync_check_ = env_flag("KC_SPILL_SYNC", false);
    return 0;
  }

  // Cut [cur, cur + len) to a chunk whose successors (an upper bound on its
  // hot-table insertions) fit both the table's room and q_max; flush the
  // hot table into the cold tier first when the room alone would make the
  // chunk less than half as long as q_max allows.
  int spill_cut(const State* cur, uint64_t len, uint64_t* cut) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t q_max = sp_.q_max, hot_limit = sp_.hot_limit;
    const uint64_t plan_len = std::min<uint64_t>(len, std::max<uint64_t>(CLAIM_TILE, q_max / 2 / 256 * 256));
    const uint64_t tiles = (plan_len + 255) / 256;
    KC_TRY(sp_tsum_.grow(tiles, st_));
    KC_TRY(h_tsum_.grow(tiles, st_));
    hipLaunchKernelGGL(k_tile_succ<M>, dim3((unsigned)tiles), dim3(256), 0, st_, cur, plan_len, flags_, sp_tsum_.p);
    KC_HIP_TRY(hipMemcpyAsync(h_tsum_, sp_tsum_, tiles * 4, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    auto pick = [&](uint64_t cap) {
      uint64_t acc = 0, c = 0;
      for (uint64_t t = 0; t < tiles; ++t) {
        if (acc + h_tsum_[t] > cap) break;
        acc += h_tsum_[t];
        c = std::min(plan_len, (t + 1) * 256);
      }
      return c;
    };
    const uint64_t room = hot_limit > hot_count_ ? hot_limit - hot_count_ : 0;
    uint64_t c = pick(std::min(room, q_max));
    if (c < plan_len && c < pick(q_max) / 2 && hot_count_ > 0) {
      KC_TRY(spill_flush());
      c = pick(q_max);
    }
    if (c == 0) {
      set_error("kubecheck: a 256-parent tile has %u successors, more than the seen-set's hot table takes per chunk "
                "(%llu); raise seen_hbm_bytes", h_tsum_[0], (unsigned long long)q_max);
      return -ENOMEM;
    }
    *cut = c;
    sp_seconds_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }

  // Hot table -> one sorted cold run; the table starts over empty.
  int spill_flush() {
    const auto t0 = std::chrono::steady_clock::now();
    KC_TRY(sp_.flush(cs_, sp_.hot_limit, st_));
    hot_count_ = 0;
    sp_flush_seconds_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }

  // After the chunk's claim + settle + tile scan: its winners w.r.t. the hot
  // tier are checked against the cold tier; those found lose (k_spill_apply)
  // and the tile offsets are recomputed.
  int spill_check(const State* cur, uint64_t cn, unsigned tiles) {
    const auto t0 = std::chrono::steady_clock::now();
    const auto q = sp_.carve();
    hipLaunchKernelGGL(k_spill_queries<M>, dim3(tiles), dim3(256), 0, st_, cur, cn, flags_, newmask_.p, toff_.p, q.qk,
                       q.ql);
    KC_HIP_TRY(hipMemcpyAsync(sp_.h_spctr + 2, toff_ + tiles, 4, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    const uint64_t m = (uint32_t)sp_.h_spctr[2];
    if (m > sp_.q_max) {
      set_error("kubecheck: chunk has %llu new fingerprints > %llu", (unsigned long long)m,
                (unsigned long long)sp_.q_max);
      return -EIO;
    }
    hot_count_ += m;
    sp_.queries += m;
    if (m && !sp_.cold.empty()) {
      hipcub::DoubleBuffer<uint64_t> kb(q.qk, q.qk2);
      hipcub::DoubleBuffer<uint32_t> vb(q.ql, q.ql2);
      size_t tb = sp_.sp_qtmp_bytes;
      KC_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(q.tmp, tb, kb, vb, (int)m, 0, 64, st_));
      KC_HIP_TRY(hipMemsetAsync(q.found, 0, m, st_));
      KC_TRY(sp_.cold.probe(kb.Current(), m, q.found, sp_.d_spctr, st_));
      hipLaunchKernelGGL(k_spill_apply, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st_, kb.Current(),
                         vb.Current(), q.found, m, newmask_.p, ttot_.p, cs_.t, cs_.nslots, d_ctr_.p);
      hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, ttot_.p, tiles, toff_.p, tscan_reg_);
      KC_HIP_TRY(hipGetLastError());
      if (sp_sync_check_) KC_HIP_TRY(hipStreamSynchronize(st_));   // (KC_SPILL_SYNC=1: time the check itself)
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    sp_seconds_ += dt;
    sp_check_seconds_ += dt;
    return 0;
  }

  bool spill_ = false;
  SeenSpill<uint32_t> sp_;
  uint64_t hot_count_ = 0;            // entries of the hot table
  DeviceArray<uint32_t> sp_tsum_;
  PinnedArray<uint32_t> h_tsum_;
  double sp_seconds_ = 0, sp_flush_seconds_ = 0, sp_check_seconds_ = 0;
  bool sp_sync_check_ = false;

  // ---- frontiers in the StateQueue (cfg.frontier_hbm_bytes > 0; squeue.h).
  // The queue holds level L's states followed by level L+1's as they are
  // made.  Each chunk of <= one segment of parents is read in place from the
  // head (front), expanded by the same kernels as the in-HBM path, and its
  // new states go straight into a run reserved at the tail; segments past
  // the HBM budget spill to host RAM / disk and come back when the head
  // reaches them.  A chunk's parents are popped one chunk later, after the
  // sync that would report an error found among them.  One host sync per
  // chunk: its new-state count sizes the reservation.  Same kernels, same
  // order keys: results equal the in-HBM path's.
  int run_queued(kc_result* res, uint64_t n, uint64_t cand, const std::vector<State>& init) {
    if (!q_) {
      SegQueue::Config qc;
      qc.words = M::W;
      qc.device = cfg_.device;
      qc.seg_states = cfg_.frontier_segment_states ? cfg_.frontier_segment_states : (1ull << 22);
      qc.hbm_bytes = cfg_.frontier_hbm_bytes;
      qc.host_bytes = cfg_.frontier_host_bytes;
      qc.dir = cfg_.spill_dir ? cfg_.spill_dir : "";
      q_.reset(new SegQueue());
      KC_TRY(q_->init(qc));
    }
    KC_TRY(h_last_.alloc(4));
    KC_TRY(q_->clear(st_));
    KC_TRY(q_->enqueue_host(reinterpret_cast<const uint64_t*>(init.data()), n, st_));
    const uint64_t chunk = std::min<uint64_t>(
        std::min<uint64_t>(cfg_.chunk_states ? cfg_.chunk_states : kMaxChunk, kMaxChunk), q_->seg_states());
    uint64_t level_gidx = 0, cand_total = 0;
    int level = 1;
    State err_parent{};
    hipLaunchKernelGGL(k_level_reset, dim3(1), dim3(64), 0, st_, d_ctr_.p);
    while (n > 0) {
      if (cfg_.max_levels && level >= cfg_.max_levels) break;
      if (n >= (1ull << 32)) {
        set_error("kubecheck: level wider than 2^32 states");
        return -ENOMEM;
      }
      const uint64_t next_gidx = level_gidx + n;
      if (cfg_.keep_trace) KC_TRY(tf_.grow(cfg_.trace_host, next_gidx + cand + 1, st_, true));
      if (!spill_) KC_TRY(cs_.reserve(cand, st_));
      // (no chunk sums here: first-claim mode is off with the queue)
      KC_TRY(size_chunk_buffers(std::min(n, chunk), cand, level, n));
      const uint32_t succ_level = (uint32_t)level + 1;
      uint64_t start = 0, level_new = 0, popped = 0, pend = 0;
      unsigned long long seen_err = ~0ull;
      bool have_parent = false;
      // after a sync: overflow, and a new minimum error key, whose parent
      // (in this chunk or the one before, neither popped yet) is copied out
      auto check = [&](uint64_t hi) -> int {
        const Counters& c = *h_ctr_;
        if (c.overflow || c.batch_used) {
          set_error("kubecheck: state with more than %d successors or full table", M::MAXSUCC);
          return -ENOMEM;
        }
        if (c.err_key != seen_err) {
          seen_err = c.err_key;
          const uint64_t pidx = seen_err >> 16;
          if (pidx < popped || pidx >= hi) {
            set_error("kubecheck: bad error key");
            return -EIO;
          }
          const uint64_t* p = nullptr;
          uint64_t got = 0;
          KC_TRY(q_->front(pidx - popped, 1, &p, &got, st_));
          KC_HIP_TRY(hipMemcpyAsync(&err_parent, p, sizeof(State), hipMemcpyDeviceToHost, st_));
          KC_HIP_TRY(hipStreamSynchronize(st_));
          have_parent = true;
        }
        return 0;
      };
      while (start < n) {
        const uint64_t* p = nullptr;
        uint64_t m = 0;
        KC_TRY(q_->front(start - popped, std::min(chunk, n - start), &p, &m, st_));
        if (m == 0) {
          set_error("kubecheck: StateQueue holds fewer states than the level");
          return -EIO;
        }
        const State* cur = reinterpret_cast<const State*>(p);
        // seen-set spill: a chunk whose insertions fit the hot table (may flush it)
        if (spill_) KC_TRY(spill_cut(cur, m, &m));
        ++res->levels_chunks;
        const unsigned tiles = (unsigned)((m + CLAIM_TILE - 1) / CLAIM_TILE);
        timed(KK_EXPAND, [&] { claim(cur, m, start, tiles, succ_level, claim_args_); });
        timed(KK_RESOLVE, [&] { launch_settle(m, start, tiles, succ_level, spill_ ? ttot_.p : (uint32_t*)nullptr); });
        if (spill_) {
          // the tile-count path: the cold check clears winners and recounts tiles
          timed(KK_SCAN, [&] {
            hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, ttot_.p, tiles, toff_.p, tscan_reg_);
          });
          KC_TRY(spill_check(cur, m, tiles));
          KC_HIP_TRY(hipMemcpyAsync(h_last_, toff_ + tiles, 4, hipMemcpyDeviceToHost, st_));
          h_last_[1] = 0;
        } else {
          KC_TRY(scan_newmask(m));
          KC_HIP_TRY(hipMemcpyAsync(h_last_, offsets_ + m - 1, 4, hipMemcpyDeviceToHost, st_));
          KC_HIP_TRY(hipMemcpyAsync(h_last_ + 1, newmask_ + m - 1, 4, hipMemcpyDeviceToHost, st_));
        }
        KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, kCtrHead, hipMemcpyDeviceToHost, st_));
        KC_HIP_TRY(hipStreamSynchronize(st_));
        collect_times();
        KC_TRY(check(start + m));
        const uint64_t nn = (uint64_t)h_last_[0] + NewCount()(h_last_[1]);
        uint64_t* dst = nullptr;
        if (nn) KC_TRY(q_->reserve(nn, &dst, st_));
        timed(KK_EMIT, [&] {
          hipLaunchKernelGGL(k_emit<M>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st_, cur, m, start,
                             flags_, newmask_.p, offsets_.p, reinterpret_cast<State*>(dst), level_new, level_gidx,
                             next_gidx, tf_.parent(), tf_.ord(), cfg_.keep_trace, d_ctr_.p,
                             spill_ ? (const uint32_t*)toff_.p : (const uint32_t*)nullptr);
        });
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(K_ADVANCE_THREADS), 0, st_, offsets_.p, newmask_.p, m, d_ctr_.p,
                           spill_ ? (const uint32_t*)toff_.p : (const uint32_t*)nullptr, (uint64_t)(spill_ ? tiles : 0),
                           (unsigned long long*)nullptr, claim_args_.ovf.count);
        KC_HIP_TRY(hipGetLastError());
        if (nn) KC_TRY(q_->commit(nn, st_));
        level_new += nn;
        if (pend) KC_TRY(q_->pop(pend, st_));
        popped += pend;
        pend = m;
        start += m;
      }
      KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, kCtrHead, hipMemcpyDeviceToHost, st_));
      KC_HIP_TRY(hipStreamSynchronize(st_));
      collect_times();
      KC_TRY(check(n));
      if (h_ctr_->chunk_base != level_new) {
        set_error("kubecheck: StateQueue level count %llu != %llu", (unsigned long long)level_new,
                  (unsigned long long)h_ctr_->chunk_base);
        return -EIO;
      }
      const uint64_t cand_now = h_ctr_->cand_total;
      hipLaunchKernelGGL(k_level_reset, dim3(1), dim3(64), 0, st_, d_ctr_.p);   // next level's head
      cs_.count = spill_ ? hot_count_ : cs_.count + level_new;
      res->peak_frontier = std::max<uint64_t>(res->peak_frontier, n);
      if (seen_err != ~0ull) {
        KC_TRY(report_error(res, seen_err, level, level_gidx, n, have_parent ? &err_parent : nullptr));
        res->distinct += level_new;
        finish(res, 0);
        return 0;
      }
      if (pend) KC_TRY(q_->pop(pend, st_));
      res->distinct += level_new;
      if (cfg_.verbose) {
        kc_squeue_stats qs;
        q_->stats(&qs);
        fprintf(stderr, "kubecheck: level %d width %llu -> %llu new, %llu distinct; queue %llu HBM / %llu host / %llu disk segments\n",
                level, (unsigned long long)n, (unsigned long long)level_new, (unsigned long long)res->distinct,
                (unsigned long long)qs.seg_hbm, (unsigned long long)qs.seg_host, (unsigned long long)qs.seg_disk);
      }
      if (capture_level_ == level + 1 && level_new) {
        captured_.resize(level_new);
        KC_TRY(q_->peek_host(0, level_new, reinterpret_cast<uint64_t*>(captured_.data()), st_));
      }
      level_gidx = next_gidx;
      n = level_new;
      cand = cand_now - cand_total;
      cand_total = cand_now;
      ++level;
      KC_TRY(record_level(res, level, n));
    }
    last_level_ = res->nlevels;
    last_n_ = n;
    finish(res, n);
    return 0;
  }

  // KC_NARROW_TRACE=1: per-phase timestamps of the narrow kernels (thread 0
  // of every workgroup), summarised on stderr after each narrow run
  static constexpr size_t kNtraceBytes = (NTRACE_FOFF + NTRACE_LEVELS * NARROW_FWG * NTRACE_PH) * 8;
  int print_ntrace(uint32_t launches) {
    std::vector<unsigned long long> t(kNtraceBytes / 8);
    KC_HIP_TRY(hipMemcpy(t.data(), d_ntrace_, kNtraceBytes, hipMemcpyDeviceToHost));
    const int FW = NARROW_FWG;
    constexpr int P = NTRACE_PH;
    double all[P] = {}, w0[P] = {}, span = 0, gap = 0, close = 0, pub_spread = 0;
    int nl = 0, ng = 0;
    unsigned long long prev_end = 0;
    for (uint32_t l = 0; l < launches && l < NTRACE_LEVELS; ++l) {
      const unsigned long long* f = &t[NTRACE_FOFF + (uint64_t)l * FW * P];
      if (!f[1]) {                                     // inactive launch
        prev_end = 0;
        continue;
      }
      unsigned long long f0 = ~0ull, f9 = 0, f10 = 0, f4min = ~0ull, f4max = 0;
      for (int w = 0; w < FW; ++w) {
        const unsigned long long* q = f + w * P;
        f0 = std::min(f0, q[0]);
        f4min = std::min(f4min, q[3]);
        f4max = std::max(f4max, q[3]);
        f9 = std::max(f9, q[9]);
        if (q[10]) f10 = q[10];
        for (int k = 1; k <= 9; ++k) all[k] += (double)(q[k] - q[k - 1]) / FW;
      }
      for (int k = 1; k <= 9; ++k) w0[k] += (double)(f[k] - f[k - 1]);   // workgroup 0 (always live)
      close += (double)(f10 - f9);
      span += (double)(f10 - f0);
      pub_spread += (double)(f4max - f4min);
      if (prev_end && f0 > prev_end) {
        gap += (double)(f0 - prev_end);
        ++ng;
      }
      prev_end = f10;
      ++nl;
    }
    if (!nl) return 0;
    const double u = 0.01 / nl;             // 100 MHz ticks -> us, per level
    static const char* names[P] = {"", "start", "successors+ClaimSet", "mask scan", "publish+wait", "emit",
                                   "task scan", "expand tasks", "clear", "counters", "", ""};
    std::string a = "kubecheck narrow trace (" + std::to_string(nl) + " levels, us per level; mean over workgroups / workgroup 0):";
    char buf[96];
    for (int k = 1; k <= 9; ++k) {
      snprintf(buf, sizeof buf, " %s %.2f/%.2f,", names[k], all[k] * u, w0[k] * u);
      a += buf;
    }
    snprintf(buf, sizeof buf, " close %.2f; span %.2f; publish spread %.2f; gap between levels %.2f\n", close * u,
             span * u, pub_spread * u, ng ? gap * 0.01 / ng : 0.0);
    a += buf;
    fputs(a.c_str(), stderr);
    return 0;
  }
  DeviceArray<unsigned long long> d_ntrace_;

  Flags flags_{};
  uint64_t init_cut_ = 0;       // Init states discarded by a state constraint (ConModel)
  bool cover_on_ = false, cover_valid_ = false;
  // user-defined invariants: the program (host copy and the run's device
  // copy), the current level's result block and the closed levels' blocks
  bool pred_on_ = false, pred_valid_ = false;
  int pred_ninv_ = 0;
  std::vector<PredInstr> pred_prog_;
  DeviceArray<PredInstr> d_pred_prog_;
  DeviceArray<unsigned long long> d_pred_;
  PinnedArray<unsigned long long> h_pred_;
  std::vector<std::pair<int, std::array<uint64_t, PRED_OUT_WORDS>>> pred_levels_;   // (level, its block)
  DeviceArray<unsigned long long> d_cover_;      // the current level's sums
  PinnedArray<unsigned long long> h_cover_;
  std::vector<std::pair<int, std::array<uint64_t, KC_COVER_N>>> cover_levels_;   // (level, its sums), closed levels
  ShardArgs claim_args_{};
  bool queued_ = false;
  std::unique_ptr<SegQueue> q_;
  PinnedArray<uint32_t> h_last_;     // a chunk's last offset and mask
  DeviceArray<NarrowCtl> d_ns_;
  PinnedArray<NarrowCtl> h_ns_;
  DeviceArray<NarrowScratch> d_nsc_;
  bool narrow_on_ = true;
  uint64_t narrow_probes_ = 0;
  uint32_t narrow_epoch_ = 0;
  DevClaimSet cs_;
  DeviceArray<State> cur_, next_;
  TraceFile tf_;                    // in HBM, or in pinned host RAM with cfg.trace_host
  DeviceArray<uint32_t> newmask_, offsets_;
  DeviceArray<uint32_t> abl_mask_;
  DeviceArray<Counters> d_ctr_abl_; // KC_ABLATE: scratch counters of the k_emit variants
  // Default: settle pass B counts each tile's new states and one workgroup
  // scans the tile counts (k_tile_scan); KC_TSCAN=0: the per-parent hipcub
  // scan instead.  KC_HEADCOPY=1: the level head read back by a copy launch
  // plus a reset launch instead of k_advance's direct write.  (Same-box A/B,
  // NP=2 with events on every kernel: 165.7 ms both off, 163.9 direct head,
  // 162.5 both on; profiles/r02o_ab1.txt.)
  bool tscan_ = false, headcopy_ = false;
  int narrow_batch_ = NARROW_BATCH;
  int tscan_reg_ = 1;   // KC_TSCAN_REG=0: k_tile_scan's loop path (levels > 65,536 tiles) at any width
  // settle passes A and B of a chunk's tiles (k_settle_rec, one workgroup
  // per tile; round 5 measured 2 / 4 / 8 tiles per workgroup no faster,
  // DESIGN §7.3), then the overflow list's pass B
  void launch_settle(uint64_t cn, uint64_t start, unsigned tiles, uint32_t succ_level, uint32_t* ttot,
                     bool ovf_in_scan = false) {
    hipLaunchKernelGGL(k_settle_rec<0>, dim3(tiles + SETTLE_OVF_BLOCKS), dim3(CLAIM_TILE), 0, st_, cn, start,
                       cs_.t, cs_.nslots, succ_level, rcount_.p, rec_fp_.p, rec_lk_.p, newmask_.p, d_ctr_.p, 0u,
                       (uint32_t*)nullptr, tiles, claim_args_.ovf);
    hipLaunchKernelGGL(k_settle_rec<1>, dim3(tiles), dim3(CLAIM_TILE), 0, st_, cn, start, cs_.t, cs_.nslots,
                       succ_level, rcount_.p, rec_fp_.p, rec_lk_.p, newmask_.p, d_ctr_.p, 0u, ttot);
    if (!ovf_in_scan)   // (else k_ovf_tile_scan settles it)
      hipLaunchKernelGGL(k_settle_ovf<1>, dim3(SETTLE_OVF_GRID), dim3(256), 0, st_, claim_args_.ovf, cn, start, cs_.t,
                         cs_.nslots, succ_level, newmask_.p, d_ctr_.p, 0u, ttot);
  }
  // k_chunk_scan's chunk sums (zeroed at allocation, at every run's start
  // and by each scan)
  bool chunk_scan_ = true;
  DeviceArray<uint32_t> csum_;
  DeviceArray<uint64_t> init_fps_;
  DeviceArray<int> init_res_;
  bool first_claim_ = false;   // KC_FIRST_CLAIM=1: k_claim FIRST, no settle passes (multi-worker TLC semantics)
  DeviceArray<uint32_t> ttot_, toff_;
  DeviceArray<unsigned int> rcount_, rec_lk_;
  DeviceArray<unsigned long long> rec_fp_;
  DeviceArray<uint8_t> scan_tmp_;
  DeviceArray<Counters> d_ctr_;
  PinnedArray<Counters> h_ctr_;
  PinnedArray<uint64_t> h_chain_;      // [0] length, then the parent chain (k_parent_chain)
  std::chrono::steady_clock::time_point t0_;   // the run's start
  std::vector<OwnedEvent> ev_pool_;
  std::vector<int> ev_kind_;
  size_t ev_used_ = 0;
  std::vector<State> init_states_, trace_, captured_;
  uint64_t last_n_ = 0;
  int last_level_ = 0;
  // checkpoint / recover: run()'s own checkpoints (set_checkpoint), the level
  // top the last run stopped at (checkpoint) and the armed recovery (recover)
  bool ck_on_ = false;
  int ck_every_ = 0, ck_l0_ = 1;
  double ck_seconds_ = 0;
  uint64_t ck_stage_bytes_ = 0;
  std::string ck_dir_;
  std::chrono::steady_clock::time_point ck_last_;
  CkptStage ck_stage_;
  std::unique_ptr<Counters> ck_ctr_;     // host copy of the counters, out and in
  LevelCursor stop_cur_;
  RunTotals stop_totals_;
  bool stop_valid_ = false;
  std::string rec_dir_;
  struct kc_checkpoint_info rec_info_ {};
  bool rec_armed_ = false;
};

template <class M>
size_t EngineT<M>::trace_text(char* buf, size_t cap) const {
  std::string s;
  for (size_t i = 0; i < trace_.size(); ++i) {
    s += "State " + std::to_string(i + 1) + ":\n";
    std::vector<uint64_t> t(M::TUPLE_WORDS);
    M::to_tuple(trace_[i], t.data());
    s += format_tuple(t.data(), cfg_.nc, cfg_.np, cfg_.ns, (cfg_.invariants & 4) != 0);
    s += "\n";
  }
  if (buf && cap) {
    const size_t k = std::min(cap - 1, s.size());
    memcpy(buf, s.data(), k);
    buf[k] = 0;
  }
  return s.size() + 1;
}

#ifdef KC_ENGINE_SYM_TU
// eff = sym_effective(cfg): a mask with a non-trivial group
std::unique_ptr<EngineBase> make_engine_sym(const kc_model_config& cfg, int eff) {
#define KC_MAKE(a, b, c, m)                                           \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c && eff == m)          \
    return std::unique_ptr<EngineBase>(new EngineT<SymModel<a, b, c, m>>(cfg));
  KC_FOR_EACH_SYM_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}
#elif defined(KC_ENGINE_CON_TU)
std::unique_ptr<EngineBase> make_engine_con(const kc_model_config& cfg) {
#define KC_MAKE(a, b, c)                                              \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c)                      \
    return std::unique_ptr<EngineBase>(new EngineT<ConModel<a, b, c>>(cfg));
  KC_FOR_EACH_CON_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}
#elif defined(KC_ENGINE_ACT_TU)
std::unique_ptr<EngineBase> make_engine_act(const kc_model_config& cfg) {
#define KC_MAKE(a, b, c)                                              \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c)                      \
    return std::unique_ptr<EngineBase>(new EngineT<ActModel<a, b, c>>(cfg));
  KC_FOR_EACH_ACT_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}
#else
std::unique_ptr<EngineBase> make_engine(const kc_model_config& cfg) {
  // action properties: the ActModel instantiations (engine_act.hip); with
  // the mask 0 the plain engine runs (kc_engine_create refused them together
  // with constraints or symmetry)
  if (cfg.action_properties) return make_engine_act(cfg);
  // a constraint: the ConModel instantiations (engine_con.hip); with the
  // three fields at their defaults the plain engine runs
  if (con_active(cfg.constraint_stored, cfg.constraint_inflight, cfg.action_constraints)) return make_engine_con(cfg);
  // symmetry with a non-trivial group: the SymModel instantiations
  // (engine_sym.hip); a mask that selects no group runs the plain engine
  if (const int eff = sym_effective(cfg.nc, cfg.np, cfg.symmetry)) return make_engine_sym(cfg, eff);
#define KC_MAKE(a, b, c)                                              \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c)                      \
    return std::unique_ptr<EngineBase>(new EngineT<Model<a, b, c>>(cfg));
  KC_FOR_EACH_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}
#endif

}  // namespace kc

#ifndef KC_ENGINE_DERIVED_TU

using namespace kc;

struct kc_engine {
  std::unique_ptr<EngineBase> impl;
};

extern "C" {

void kc_model_config_default(kc_model_config* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  c->nc = c->np = c->ns = 1;
  c->can_fail = c->can_timeout = 1;
  c->check_deadlock = 1;
  c->keep_trace = 1;
  c->invariants = 3;
  c->constraint_stored = c->constraint_inflight = -1;
}

int kc_engine_create(const kc_model_config* cfg, kc_engine** out) {
  if (!cfg || !out) { set_error("kc_engine_create: NULL argument"); return -EINVAL; }
  *out = nullptr;
  if (cfg->symmetry & ~3) {
    set_error("kc_engine_create: symmetry %d outside 0..3 (bit 0 clients, bit 1 PVC controllers)", cfg->symmetry);
    return -EINVAL;
  }
  if (const int eff = sym_effective(cfg->nc, cfg->np, cfg->symmetry)) {
    // variant 5's Init store names actor 0 in a version vector: not closed
    // under a group that moves actor 0
    if (cfg->variant == 5 && ((eff & 1) || cfg->nc == 0)) {
      set_error("kc_engine_create: variant 5 is not symmetric under symmetry=%d (its Init store names actor 0)", cfg->symmetry);
      return -EINVAL;
    }
  }
  const bool con = con_active(cfg->constraint_stored, cfg->constraint_inflight, cfg->action_constraints);
  if (con) {
    // constraints: the in-HBM single-GPU BFS only
    if (cfg->action_constraints & ~AC_ALL) {
      set_error("kc_engine_create: action_constraints %d outside 0..%d (bit 0 ServeClientsFirst)",
                cfg->action_constraints, AC_ALL);
      return -EINVAL;
    }
    if (cfg->symmetry) {
      set_error("kc_engine_create: constraints are not supported under symmetry (TLC needs a symmetric constraint; "
                "ServeClientsFirst and the bounds under `clients` would each need an argument)");
      return -EINVAL;
    }
    if (cfg->seen_hbm_bytes || cfg->frontier_hbm_bytes || cfg->trace_host) {
      set_error("kc_engine_create: constraints are not supported with seen_hbm_bytes, frontier_hbm_bytes or trace_host");
      return -EINVAL;
    }
  }
  if (cfg->action_properties) {
    // action properties: the in-HBM single-GPU BFS only
    if (cfg->action_properties & ~AP_ALL) {
      set_error("kc_engine_create: action_properties %d outside 0..%d (bit 0 NoBlindUpdate, bit 1 OneReplyPerStep, "
                "bit 2 StoreNeverShrinks)", cfg->action_properties, AP_ALL);
      return -EINVAL;
    }
    if (con) {
      set_error("kc_engine_create: action properties are not supported with constraints (a step out of the model "
                "would need TLC's rule for both)");
      return -EINVAL;
    }
    if (cfg->symmetry) {
      set_error("kc_engine_create: action properties are not supported under symmetry (a step is checked between "
                "real states, the seen-set holds orbits)");
      return -EINVAL;
    }
    if (cfg->seen_hbm_bytes || cfg->frontier_hbm_bytes || cfg->trace_host) {
      set_error("kc_engine_create: action properties are not supported with seen_hbm_bytes, frontier_hbm_bytes or "
                "trace_host");
      return -EINVAL;
    }
  }
  auto impl = make_engine(*cfg);
  if (!impl) {
    set_error("kc_engine_create: unsupported model nc=%d np=%d ns=%d%s", cfg->nc, cfg->np, cfg->ns,
              con ? " with constraints" : cfg->action_properties ? " with action properties" : "");
    return -EINVAL;
  }
  KC_TRY(impl->setup());
  *out = new kc_engine{std::move(impl)};
  return 0;
}

void kc_engine_destroy(kc_engine* e) { delete e; }

int kc_engine_run(kc_engine* e, kc_result* res) {
  if (!e || !res) { set_error("kc_engine_run: NULL argument"); return -EINVAL; }
  return e->impl->run(res);
}

size_t kc_engine_trace_text(kc_engine* e, char* buf, size_t cap) {
  return e ? e->impl->trace_text(buf, cap) : 0;
}

int kc_engine_trace_tuple(kc_engine* e, int i, uint64_t* out) {
  if (!e || !out) { set_error("kc_engine_trace_tuple: NULL"); return -EINVAL; }
  return e->impl->trace_tuple(i, out);
}

int64_t kc_engine_level_tuples(kc_engine* e, int level, uint64_t* out, uint64_t cap) {
  if (!e) { set_error("kc_engine_level_tuples: NULL"); return -EINVAL; }
  return e->impl->level_tuples(level, out, cap);
}

int kc_engine_capture_level(kc_engine* e, int level) {
  if (!e) { set_error("kc_engine_capture_level: NULL"); return -EINVAL; }
  e->impl->set_capture(level);
  return 0;
}

int kc_engine_set_coverage(kc_engine* e, int on) {
  if (!e) { set_error("kc_engine_set_coverage: NULL"); return -EINVAL; }
  return e->impl->set_coverage(on != 0);
}

int kc_engine_set_invariants(kc_engine* e, const uint64_t* program, int n_instr) {
  if (!e) { set_error("kc_engine_set_invariants: NULL"); return -EINVAL; }
  if (n_instr < 0) { set_error("kc_engine_set_invariants: negative n_instr"); return -EINVAL; }
  return e->impl->set_invariants(program, n_instr);
}

int kc_engine_invariant_stats(kc_engine* e, uint64_t* out, int cap) {
  if (!e) { set_error("kc_engine_invariant_stats: NULL"); return -EINVAL; }
  return e->impl->invariant_stats(out, cap);
}

int kc_engine_coverage(kc_engine* e, uint64_t* out, int cap) {
  if (!e) { set_error("kc_engine_coverage: NULL"); return -EINVAL; }
  return e->impl->coverage(out, cap);
}

int kc_engine_checkpoint(kc_engine* e, const char* dir) {
  if (!e) { set_error("kc_engine_checkpoint: NULL"); return -EINVAL; }
  return e->impl->checkpoint(dir);
}

int kc_engine_set_checkpoint(kc_engine* e, const kc_checkpoint_options* opt) {
  if (!e) { set_error("kc_engine_set_checkpoint: NULL"); return -EINVAL; }
  return e->impl->set_checkpoint(opt);
}

int kc_engine_recover(kc_engine* e, const char* dir) {
  if (!e) { set_error("kc_engine_recover: NULL"); return -EINVAL; }
  return e->impl->recover(dir);
}

int kc_engine_instantiation(kc_engine* e) {
  if (!e) { set_error("kc_engine_instantiation: NULL"); return -EINVAL; }
  return e->impl->instantiation();
}

int kc_engine_narrow_times(kc_engine* e, double* ms, uint64_t* launches, uint64_t* levels) {
  if (!e || !ms || !launches || !levels) { set_error("kc_engine_narrow_times: NULL"); return -EINVAL; }
  e->impl->narrow_times(ms, launches, levels);
  return 0;
}

int kc_engine_check_fps(kc_engine* e, uint64_t* min_gap, double* prob) {
  if (!e || !min_gap || !prob) { set_error("kc_engine_check_fps: NULL"); return -EINVAL; }
  return e->impl->check_fps(min_gap, prob);
}

int kc_engine_kernel_times(kc_engine* e, double* ms4, uint64_t* launches4) {
  if (!e) { set_error("kc_engine_kernel_times: NULL"); return -EINVAL; }
  e->impl->kernel_times(ms4, launches4);
  return 0;
}

}  // extern "C"
#endif  // KC_ENGINE_DERIVED_TU
