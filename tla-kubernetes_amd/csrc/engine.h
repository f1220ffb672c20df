// engine.h — type-erased engine interface behind the kc_engine_* C-ABI.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>

#include "../../include/kubecheck.h"

namespace kc {

// Kernel kinds timed by the engine (kc_engine_kernel_times order).
enum KernelKind { KK_EXPAND = 0, KK_RESOLVE = 1, KK_SCAN = 2, KK_EMIT = 3, KK_COUNT = 4 };
// diagnostic-only ablation timings (KC_ABLATE=1 in the environment): extra
// launches of cut-down k_claim / k_emit variants on scratch buffers, printed to stderr
enum AblateKind { KA_LDS = KK_COUNT, KA_COMPUTE = KK_COUNT + 1, KA_PLAN = KK_COUNT + 2,
                  KA_E1 = KK_COUNT + 3, KA_E2 = KK_COUNT + 4, KA_E3 = KK_COUNT + 5,
                  KA_FPCHEAP = KK_COUNT + 6, KA_NOAPPLY = KK_COUNT + 7, KA_TOTAL = KK_COUNT + 8 };
// the narrow-level kernel (engine_narrow.h): levels it ran, launches, time
constexpr int KK_NARROW = KA_TOTAL;
constexpr int KK_ALL = KA_TOTAL + 1;

class EngineBase {
 public:
  // the config is kept by value; its one string is copied too
  explicit EngineBase(const kc_model_config& cfg) : cfg_(cfg), spill_dir_(cfg.spill_dir ? cfg.spill_dir : "") {
    cfg_.spill_dir = cfg.spill_dir ? spill_dir_.c_str() : nullptr;
  }
  virtual ~EngineBase() = default;
  virtual int setup() = 0;
  virtual int run(kc_result* res) = 0;
  virtual size_t trace_text(char* buf, size_t cap) const = 0;
  virtual int trace_tuple(int i, uint64_t* out) const = 0;
  virtual int64_t level_tuples(int level, uint64_t* out, uint64_t cap) = 0;
  virtual int state_words() const = 0;
  virtual int instantiation() const = 0;
  virtual int tuple_words() const = 0;
  virtual int check_fps(uint64_t* min_gap, double* prob) = 0;
  void set_capture(int level) { capture_level_ = level; }
  // expression-level coverage (cover.h): count every expanded state's base
  // counters from the next run on; the last run's sums
  virtual int set_coverage(bool on) = 0;
  virtual int coverage(uint64_t* out, int cap) const = 0;
  // user-defined invariants (pred.h): evaluate the program on
  // every expanded state from the next run on (n_instr = 0: off); the last
  // run's states evaluated and violations per invariant
  virtual int set_invariants(const uint64_t* program, int n_instr) = 0;
  virtual int invariant_stats(uint64_t* out, int cap) const = 0;
  // checkpoint / recover: write the state the last run
  // stopped with; checkpoint from inside run(); arm the next run to start
  // from a checkpoint
  virtual int checkpoint(const char* dir) = 0;
  virtual int set_checkpoint(const kc_checkpoint_options* opt) = 0;
  virtual int recover(const char* dir) = 0;
  void set_timing(bool on) { timing_ = on ? 1 : 0; }
  void kernel_times(double* ms, uint64_t* launches) const {
    for (int k = 0; k < KK_COUNT; ++k) {
      if (ms) ms[k] = ktime_ms_[k];
      if (launches) launches[k] = klaunch_[k];
    }
  }
  void narrow_times(double* ms, uint64_t* launches, uint64_t* levels) const {
    *ms = ktime_ms_[KK_NARROW];
    *launches = klaunch_[KK_NARROW];
    *levels = narrow_levels_;
  }

 protected:
  kc_model_config cfg_;
  std::string spill_dir_;
  int capture_level_ = 0;
  int timing_ = 0;   // 1: HIP events on every kernel; 2: on k_claim only
  double ktime_ms_[KK_ALL] = {};
  uint64_t klaunch_[KK_ALL] = {};
  uint64_t narrow_levels_ = 0;
  bool ablate_ = false;
};

std::unique_ptr<EngineBase> make_engine(const kc_model_config& cfg);
// the engine under symmetry reduction (engine_sym.hip); eff = a mask with a
// non-trivial group (kubeapi_spec.h sym_effective); nullptr for other models
std::unique_ptr<EngineBase> make_engine_sym(const kc_model_config& cfg, int eff);
// the engine under constraints (engine_con.hip: EngineT<ConModel<..>>);
// nullptr for a model outside KC_FOR_EACH_CON_MODEL
std::unique_ptr<EngineBase> make_engine_con(const kc_model_config& cfg);
// the engine under action properties (engine_act.hip: EngineT<ActModel<..>>);
// nullptr for a model outside KC_FOR_EACH_ACT_MODEL
std::unique_ptr<EngineBase> make_engine_act(const kc_model_config& cfg);
const char* action_name(int a);
// k_cover (cover.hip) over n packed states of cfg's plain Model on `stream`
// (a hipStream_t): their coverage base counters added into d_sums[KC_COVER_N]
int cover_launch(const kc_model_config& cfg, const void* states, uint64_t n, unsigned long long* d_sums,
                 void* stream);
// TLA+-style rendering of a canonical tuple (spec_abi.cpp)
std::string format_tuple(const uint64_t* tuple, int nc, int np, int ns, bool ghost = false);

}  // namespace kc
