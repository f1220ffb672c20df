// simulate.hip — simulation mode (TLC -simulate) on one GPU: seeded random
// walks, one lane per walk, each state checked against the invariants, the
// Asserts and deadlock (include/kubecheck.h, "Simulation").
//
// A walk's choices are a pure function of (seed, walk, step) (simulate.h), so
// the device keeps only each walk's current state and one status word; the
// host replays a walk (kc_sim_replay) to print it, and kc_sim_trace checks the
// replay against what the device recorded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kubecheck.h"
#include "engine.h"
#include "engine_util.h"
#include "fpset_host.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "simulate.h"

namespace kc {

namespace {

constexpr int SIM_BLOCK = 256;
constexpr int SIM_DEFAULT_STEPS = 32;   // steps per launch
// LDS histogram bins: the actions, then the ways a walk ends
constexpr int SIM_NBIN = A_COUNT + SIM_NKIND;
constexpr uint64_t SIM_WALK_MASK = (1ull << 40) - 1;

// Device counters of one run.
struct SimCounters {
  unsigned long long bin[SIM_NBIN];   // steps per action, walks per end kind
  unsigned long long err_key;         // min over error walks of trace_len << 40 | walk
  unsigned long long inserted;        // DISTINCT: fingerprints newly inserted
  unsigned long long full;            // DISTINCT: fpset_insert found the table full
};

struct SimArgs {
  uint64_t* state;            // word i of walk w at [i * num_walks + w]
  uint32_t* status;           // sim_status per walk
  uint64_t num_walks;
  uint64_t seed_mixed;        // sim_mix(seed)
  int depth;
  int steps;                  // iterations of this launch
  int check_deadlock;
  Flags flags;
  SimCounters* ctr;
  unsigned long long* slots;  // DISTINCT: the DevFpset
  uint64_t nbuckets;
};

__device__ __forceinline__ void sim_flush_bins(const unsigned int* hist, SimCounters* ctr) {
  if (threadIdx.x < SIM_NBIN) {
    const unsigned int v = hist[threadIdx.x];
    if (v) atomicAdd(&ctr->bin[threadIdx.x], (unsigned long long)v);
  }
}

// s_0 and the status of every walk; with DISTINCT the Init states' fingerprints.
template <class M, bool DISTINCT>
__global__ void __launch_bounds__(SIM_BLOCK) k_sim_init(SimArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
  if (w >= a.num_walks) return;
  const uint64_t key = sim_key(a.seed_mixed, w);
  const int i0 = (int)sim_pick(sim_rand_key(key, 0), (uint64_t)M::num_init());
  typename M::State s;
  M::init_state(i0, s, a.flags.variant);
#pragma unroll
  for (int i = 0; i < M::W_RAW; ++i) a.state[(uint64_t)i * a.num_walks + w] = s.w[i];
  a.status[w] = sim_status(SIM_RUNNING, 0, 0, 0);
  if constexpr (DISTINCT) {
    const int r = fpset_insert(a.slots, a.nbuckets, M::fingerprint(s));
    if (r > 0) atomicAdd(&a.ctr->inserted, 1ull);
    if (r < 0) atomicAdd(&a.ctr->full, 1ull);
  }
}

// At most a.steps steps of every walk still running.  One lane per walk; the
// state is loaded into registers, advanced and stored back.
template <class M, bool DISTINCT>
__global__ void __launch_bounds__(SIM_BLOCK) k_sim_walk(SimArgs a) {
  __shared__ unsigned int hist[SIM_NBIN];
  if (threadIdx.x < SIM_NBIN) hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t w = (uint64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
  uint32_t st = w < a.num_walks ? a.status[w] : sim_status(SIM_DEPTH, 0, 0, 0);
  if (sim_status_kind(st) == SIM_RUNNING) {
    typename M::State s;
#pragma unroll
    for (int i = 0; i < M::W_RAW; ++i) s.w[i] = a.state[(uint64_t)i * a.num_walks + w];
#pragma unroll
    for (int i = M::W_RAW; i < M::W; ++i) s.w[i] = 0;
    const uint64_t key = sim_key(a.seed_mixed, w);
    uint32_t k = sim_status_k(st);
    unsigned int inserted = 0;
    bool full = false;
    for (int it = 0; it < a.steps; ++it) {
      typename M::State x;
      const SimStep r = sim_step<M>(s, k, key, a.flags, a.depth, a.check_deadlock, x);
      if (r.kind != SIM_RUNNING) {
        st = sim_status(r.kind, r.info, r.self, k);
        atomicAdd(&hist[A_COUNT + r.kind], 1u);
        if (r.kind <= SIM_DEADLOCK) atomicMin(&a.ctr->err_key, ((unsigned long long)(k + 1) << 40) | w);
        break;
      }
      atomicAdd(&hist[r.info], 1u);
      if constexpr (DISTINCT) {
        const int ins = fpset_insert(a.slots, a.nbuckets, M::fingerprint_succ(s, M::fp_fold(s), x, r.who));
        inserted += ins > 0;
        full |= ins < 0;
      }
#pragma unroll
      for (int i = 0; i < M::W_RAW; ++i) s.w[i] = x.w[i];
      ++k;
      st = sim_status(SIM_RUNNING, 0, 0, k);
    }
#pragma unroll
    for (int i = 0; i < M::W_RAW; ++i) a.state[(uint64_t)i * a.num_walks + w] = s.w[i];
    a.status[w] = st;
    if constexpr (DISTINCT) {
      if (inserted) atomicAdd(&a.ctr->inserted, (unsigned long long)inserted);
      if (full) atomicAdd(&a.ctr->full, 1ull);
    }
  }
  __syncthreads();
  sim_flush_bins(hist, a.ctr);
}

class SimBase {
 public:
  virtual ~SimBase() = default;
  virtual int setup() = 0;
  virtual int run(kc_sim_result* res) = 0;
  virtual int walks(uint32_t* kind, uint32_t* len, uint64_t* tuples) = 0;
  virtual int trace(uint64_t walk, uint64_t* tuples, int* actions, int cap) = 0;
  virtual int tuple_words() const = 0;
  kc_model_config cfg;
  kc_sim_config sim;
};

template <class M>
class SimT : public SimBase {
 public:
  ~SimT() override { (void)hipSetDevice(cfg.device); }   // (the members free themselves on it)
  int tuple_words() const override { return M::TUPLE_WORDS; }

  int setup() override {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      set_error("kubecheck: no HIP device visible (simulation has no CPU fallback)");
      return -ENODEV;
    }
    if (cfg.device < 0 || cfg.device >= ndev) {
      set_error("kubecheck: bad device %d", cfg.device);
      return -EINVAL;
    }
    KC_HIP_TRY(hipSetDevice(cfg.device));
    KC_TRY(st_.create(hipStreamNonBlocking));
    KC_TRY(ev0_.create());
    KC_TRY(ev1_.create());
    KC_TRY(d_state_.alloc(sim.num_walks * M::W_RAW));
    KC_TRY(d_status_.alloc(sim.num_walks));
    KC_TRY(d_ctr_.alloc(1));
    return h_ctr_.alloc(1);
  }

  int run(kc_sim_result* res) override {
    KC_HIP_TRY(hipSetDevice(cfg.device));
    const auto t0 = std::chrono::steady_clock::now();
    memset(res, 0, sizeof *res);
    res->err_action = res->err_self = res->err_invariant = -1;
    ran_ = false;
    const bool distinct = sim.count_distinct != 0;
    const uint64_t nw = sim.num_walks;
    int spl = sim.steps_per_launch > 0 ? sim.steps_per_launch : SIM_DEFAULT_STEPS;
    if (spl > sim.depth) spl = sim.depth;

    SimCounters zero;
    memset(&zero, 0, sizeof zero);
    zero.err_key = ~0ull;
    KC_HIP_TRY(hipMemcpyAsync(d_ctr_, &zero, sizeof zero, hipMemcpyHostToDevice, st_));
    if (distinct) {
      // every walk's Init state is one of num_init(); the walk launches
      // reserve their own room below
      KC_TRY(fs_.init(4096, st_));
    }
    SimArgs a{};
    a.state = d_state_;
    a.status = d_status_;
    a.num_walks = nw;
    a.seed_mixed = sim_mix(sim.seed);
    a.depth = sim.depth;
    a.steps = spl;
    a.check_deadlock = cfg.check_deadlock;
    a.flags = flags_of(cfg);
    a.ctr = d_ctr_;
    a.slots = fs_.slots;
    a.nbuckets = fs_.nbuckets;
    const dim3 grid((unsigned)((nw + SIM_BLOCK - 1) / SIM_BLOCK)), block(SIM_BLOCK);
    if (distinct)
      hipLaunchKernelGGL((k_sim_init<M, true>), grid, block, 0, st_, a);
    else
      hipLaunchKernelGGL((k_sim_init<M, false>), grid, block, 0, st_, a);
    KC_HIP_TRY(hipGetLastError());
    KC_TRY(read_counters());

    // A walk of `depth` states takes depth iterations (the last one only
    // checks its final state), so ceil(depth / spl) launches end every walk.
    double kernel_ms = 0;
    uint64_t launches = 0;
    for (int done = 0; done < sim.depth; done += spl) {
      const uint64_t live = nw - ended();
      if (live == 0) break;
      if (sim.stop_on_error && h_ctr_->err_key != ~0ull) break;
      a.steps = sim.depth - done < spl ? sim.depth - done : spl;
      if (distinct) {
        fs_.count = h_ctr_->inserted;
        KC_TRY(fs_.reserve(live * (uint64_t)a.steps, st_));
        a.slots = fs_.slots;
        a.nbuckets = fs_.nbuckets;
      }
      KC_HIP_TRY(hipEventRecord(ev0_, st_));
      if (distinct)
        hipLaunchKernelGGL((k_sim_walk<M, true>), grid, block, 0, st_, a);
      else
        hipLaunchKernelGGL((k_sim_walk<M, false>), grid, block, 0, st_, a);
      KC_HIP_TRY(hipGetLastError());
      KC_HIP_TRY(hipEventRecord(ev1_, st_));
      KC_TRY(read_counters());
      float ms = 0;
      KC_HIP_TRY(hipEventElapsedTime(&ms, ev0_, ev1_));
      kernel_ms += ms;
      ++launches;
    }

    for (int i = 0; i < KC_NACTIONS; ++i) {
      res->act_steps[i] = h_ctr_->bin[i];
      res->steps += h_ctr_->bin[i];
    }
    res->walks_error = h_ctr_->bin[A_COUNT + SIM_ASSERT] + h_ctr_->bin[A_COUNT + SIM_INVARIANT] +
                       h_ctr_->bin[A_COUNT + SIM_DEADLOCK];
    res->walks_depth = h_ctr_->bin[A_COUNT + SIM_DEPTH];
    res->walks_terminated = h_ctr_->bin[A_COUNT + SIM_TERMINATED];
    res->distinct_visited = distinct ? h_ctr_->inserted : 0;
    res->fpset_slots = distinct ? fs_.capacity() : 0;
    res->launches = launches;
    res->kernel_ms = kernel_ms;
    if (h_ctr_->err_key != ~0ull) {
      const uint64_t walk = h_ctr_->err_key & SIM_WALK_MASK;
      uint32_t st = 0;
      KC_HIP_TRY(hipMemcpyAsync(&st, d_status_ + walk, sizeof st, hipMemcpyDeviceToHost, st_));
      KC_HIP_TRY(hipStreamSynchronize(st_));
      res->err_kind = sim_status_kind(st);
      res->err_walk = walk;
      res->trace_len = (int)sim_status_k(st) + 1;
      if (res->err_kind == SIM_ASSERT) {
        res->err_action = sim_status_info(st);
        res->err_self = sim_status_self(st);
      } else if (res->err_kind == SIM_INVARIANT) {
        res->err_invariant = sim_status_info(st);
      }
      if ((uint64_t)res->trace_len != h_ctr_->err_key >> 40 || res->err_kind < SIM_ASSERT ||
          res->err_kind > SIM_DEADLOCK) {
        set_error("kc_sim_run: walk %llu's status %#x does not match its error key", (unsigned long long)walk, st);
        return -EIO;
      }
    }
    ran_ = true;
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }

  int walks(uint32_t* kind, uint32_t* len, uint64_t* tuples) override {
    if (!ran_) { set_error("kc_sim_walks: no completed run"); return -EINVAL; }
    KC_HIP_TRY(hipSetDevice(cfg.device));
    const uint64_t nw = sim.num_walks;
    std::vector<uint32_t> st(nw);
    KC_HIP_TRY(hipMemcpyAsync(st.data(), d_status_, nw * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    std::vector<uint64_t> words;
    if (tuples) {
      words.resize(nw * M::W_RAW);
      KC_HIP_TRY(hipMemcpyAsync(words.data(), d_state_, words.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st_));
    }
    KC_HIP_TRY(hipStreamSynchronize(st_));
    for (uint64_t w = 0; w < nw; ++w) {
      if (kind) kind[w] = (uint32_t)sim_status_kind(st[w]);
      if (len) len[w] = sim_status_k(st[w]) + 1;
      if (tuples) {
        typename M::State s;
        for (int i = 0; i < M::W; ++i) s.w[i] = i < M::W_RAW ? words[(uint64_t)i * nw + w] : 0;
        M::to_tuple(s, tuples + w * M::TUPLE_WORDS);
      }
    }
    return 0;
  }

  // Replay `walk` on the host and check it against the device's record.
  int trace(uint64_t walk, uint64_t* tuples, int* actions, int cap) override {
    if (!ran_) { set_error("kc_sim_trace: no completed run"); return -EINVAL; }
    if (walk >= sim.num_walks) { set_error("kc_sim_trace: walk %llu of %llu", (unsigned long long)walk,
                                           (unsigned long long)sim.num_walks); return -EINVAL; }
    KC_HIP_TRY(hipSetDevice(cfg.device));
    uint32_t st = 0;
    uint64_t fw[M::W_RAW];
    KC_HIP_TRY(hipMemcpyAsync(&st, d_status_ + walk, sizeof st, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipMemcpy2DAsync(fw, sizeof(uint64_t), d_state_ + walk, sim.num_walks * sizeof(uint64_t),
                                sizeof(uint64_t), M::W_RAW, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    const int dkind = sim_status_kind(st), dlen = (int)sim_status_k(st) + 1;
    // a walk stopped early (stop_on_error) is replayed up to the state it reached
    const int depth = dkind == SIM_RUNNING ? dlen : sim.depth;
    std::vector<uint64_t> all((size_t)dlen * M::TUPLE_WORDS);
    std::vector<int> acts(dlen);
    int rkind = 0;
    const int rlen = kc_sim_replay(&cfg, sim.seed, depth, walk, all.data(), acts.data(), dlen, &rkind);
    if (rlen < 0) return rlen;
    if (rlen != dlen || (dkind != SIM_RUNNING && rkind != dkind)) {
      set_error("kc_sim_trace: walk %llu: the device recorded kind %d after %d states, the replay kind %d after %d",
                (unsigned long long)walk, dkind, dlen, rkind, rlen);
      return -EIO;
    }
    typename M::State s;
    for (int i = 0; i < M::W; ++i) s.w[i] = i < M::W_RAW ? fw[i] : 0;
    std::vector<uint64_t> ft(M::TUPLE_WORDS);
    M::to_tuple(s, ft.data());
    if (memcmp(ft.data(), all.data() + (size_t)(dlen - 1) * M::TUPLE_WORDS, M::TUPLE_WORDS * sizeof(uint64_t)) != 0) {
      set_error("kc_sim_trace: walk %llu: the replay's final state differs from the device's", (unsigned long long)walk);
      return -EIO;
    }
    for (int i = 0; i < dlen && i < cap; ++i) {
      if (tuples) memcpy(tuples + (size_t)i * M::TUPLE_WORDS, all.data() + (size_t)i * M::TUPLE_WORDS,
                         M::TUPLE_WORDS * sizeof(uint64_t));
      if (actions) actions[i] = acts[i];
    }
    return dlen;
  }

 private:
  uint64_t ended() const {
    uint64_t n = 0;
    for (int kd = SIM_ASSERT; kd < SIM_NKIND; ++kd) n += h_ctr_->bin[A_COUNT + kd];
    return n;
  }
  // the counters of everything launched so far; a full table is an error
  int read_counters() {
    KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, sizeof(SimCounters), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    if (h_ctr_->full) {
      set_error("kc_sim_run: the visited-state table is full (%llu slots)", (unsigned long long)fs_.capacity());
      return -ENOMEM;
    }
    return 0;
  }

  OwnedStream st_;   // (first: destroyed after every buffer below)
  DeviceArray<uint64_t> d_state_;
  DeviceArray<uint32_t> d_status_;
  DeviceArray<SimCounters> d_ctr_;
  PinnedArray<SimCounters> h_ctr_;
  DevFpset fs_;
  bool ran_ = false;
  OwnedEvent ev0_, ev1_;
};

std::unique_ptr<SimBase> make_sim(const kc_model_config& cfg) {
#define KC_MAKE(a, b, c) \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c) return std::unique_ptr<SimBase>(new SimT<Model<a, b, c>>());
  KC_FOR_EACH_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}

}  // namespace

}  // namespace kc

using namespace kc;

struct kc_sim {
  std::unique_ptr<SimBase> impl;
};

extern "C" {

int kc_sim_create(const kc_model_config* cfg, const kc_sim_config* sim, kc_sim** out) {
  if (!cfg || !sim || !out) { set_error("kc_sim_create: NULL argument"); return -EINVAL; }
  *out = nullptr;
  if (cfg->symmetry) {
    set_error("kc_sim_create: symmetry is not supported (random walks keep no seen-set to reduce)");
    return -EINVAL;
  }
  if (con_active(cfg->constraint_stored, cfg->constraint_inflight, cfg->action_constraints)) {
    set_error("kc_sim_create: constraints are not supported (the walks step through Next alone)");
    return -EINVAL;
  }
  if (cfg->action_properties) {
    set_error("kc_sim_create: action properties are not supported (the walks check invariants only)");
    return -EINVAL;
  }
  if (sim->num_walks < 1 || sim->num_walks > KC_SIM_MAX_WALKS) {
    set_error("kc_sim_create: num_walks %llu outside 1..2^30", (unsigned long long)sim->num_walks);
    return -EINVAL;
  }
  if (sim->depth < 1 || sim->depth > KC_SIM_MAX_DEPTH) {
    set_error("kc_sim_create: depth %d outside 1..%d", sim->depth, KC_SIM_MAX_DEPTH);
    return -EINVAL;
  }
  if (sim->steps_per_launch < 0) {
    set_error("kc_sim_create: steps_per_launch %d < 0", sim->steps_per_launch);
    return -EINVAL;
  }
  auto impl = make_sim(*cfg);
  if (!impl) {
    set_error("kc_sim_create: unsupported model nc=%d np=%d ns=%d", cfg->nc, cfg->np, cfg->ns);
    return -EINVAL;
  }
  impl->cfg = *cfg;
  impl->cfg.spill_dir = nullptr;   // BFS-only fields are not used
  impl->sim = *sim;
  KC_TRY(impl->setup());
  *out = new kc_sim{std::move(impl)};
  return 0;
}

void kc_sim_destroy(kc_sim* s) { delete s; }

int kc_sim_run(kc_sim* s, kc_sim_result* res) {
  if (!s || !res) { set_error("kc_sim_run: NULL argument"); return -EINVAL; }
  return s->impl->run(res);
}

int kc_sim_walks(kc_sim* s, uint32_t* kind_out, uint32_t* len_out, uint64_t* final_tuples_out) {
  if (!s) { set_error("kc_sim_walks: NULL"); return -EINVAL; }
  return s->impl->walks(kind_out, len_out, final_tuples_out);
}

int kc_sim_trace(kc_sim* s, uint64_t walk, uint64_t* tuples_out, int* actions_out, int cap) {
  if (!s) { set_error("kc_sim_trace: NULL"); return -EINVAL; }
  return s->impl->trace(walk, tuples_out, actions_out, cap);
}

int64_t kc_sim_trace_text(kc_sim* s, uint64_t walk, char* buf, size_t cap) {
  if (!s) { set_error("kc_sim_trace_text: NULL"); return -EINVAL; }
  const int n = s->impl->trace(walk, nullptr, nullptr, 0);
  if (n < 0) return n;
  const int tw = s->impl->tuple_words();
  std::vector<uint64_t> t((size_t)n * tw);
  const int n2 = s->impl->trace(walk, t.data(), nullptr, n);
  if (n2 < 0) return n2;
  const kc_model_config& c = s->impl->cfg;
  std::string text;
  for (int i = 0; i < n; ++i) {
    text += "State " + std::to_string(i + 1) + ":\n";
    text += format_tuple(t.data() + (size_t)i * tw, c.nc, c.np, c.ns, (c.invariants & 4) != 0);
    text += "\n";
  }
  if (buf && cap) {
    const size_t k = std::min(cap - 1, text.size());
    memcpy(buf, text.data(), k);
    buf[k] = 0;
  }
  return (int64_t)text.size() + 1;
}

}  // extern "C"
