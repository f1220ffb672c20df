// liveness.hip — KubeAPI.tla's temporal properties under WF_vars(Next), or
// under per-process weak fairness, on one GPU (include/kubecheck.h,
// "Liveness").
//
// Three phases under WF_vars(Next), all on one stream, everything in HBM:
//   build  the reachable graph by a level-synchronous BFS of its own: states in
//          discovery order (a level is a contiguous index range), parent and
//          level per state, a {fingerprint, index} table and CSR edges;
//   trim   alive = stay; rounds of "an alive, non-terminal state with no alive
//          successor other than itself dies" until a round removes nothing.
//          What is left is L; the property is violated iff L is not empty;
//   lasso  a shortest prefix to L (the parent chain) and a walk inside L that
//          closes a cycle or ends in a terminal state.
//
// Per-process fairness (fairness = 1) keeps build and trim (the trim is then
// only the cheap first cut: what it removes lies on no cycle of S and reaches
// no terminal state) and adds, on the CSR graph as built, no transposed copy:
//   scc    the SCCs of the alive subgraph by rounds of forward max-colour
//          propagation and a pull-style backward closure from each colour's
//          root;
//   fair   per SCC its size and the witness mask (processes disabled in a
//          member, processes of the edges inside it); F = the fair SCCs and
//          the terminal states; L = what reaches F inside S, pull-style;
//   lasso  the prefix, then legs of a restricted level-synchronous reach with
//          parents: into F, to each still-missing witness, back to the
//          cycle's first state.
//
// No data crosses workgroups inside a launch except through atomics: the
// table's CAS decides who inserts a fingerprint, and a lane that finds one
// inserted in the same launch records the SLOT (the inserter may not have
// stored its index yet); k_live_resolve turns slots into indices afterwards.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kubecheck.h"
#include "engine.h"
#include "engine_util.h"
#include "fpset_dev.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "live_graph.h"
#include "live_prog.h"
#include "liveness.h"
#include "simulate.h"

namespace kc {

namespace {

constexpr uint64_t LIVE_DEFAULT_STATES = 1ull << 24;
constexpr uint64_t LIVE_MIN_STATES = 16;            // every model's Init states fit
constexpr uint64_t LIVE_MAX_STATES = 1ull << 27;    // edge offsets stay below 2^31
constexpr uint64_t LIVE_EDGES_PER_STATE = 8;        // edge capacity = 8 x max_states
enum : unsigned { LIVE_OVF_STATES = 1, LIVE_OVF_EDGES = 2, LIVE_OVF_TABLE = 4 };

// 1 = this lane inserted fp, 0 = it was there, -1 = no empty slot; slot = where.
// A stale copy can only show a filled slot as empty; the CAS settles it.
__device__ __forceinline__ int live_insert(LiveSlot* t, uint64_t nslots, uint64_t fp, uint64_t& slot) {
  uint64_t i = bucket_of(fp, nslots);
  for (uint64_t probe = 0; probe < nslots; ++probe) {
    const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(t + i);
    if (e.x == fp) { slot = i; return 0; }
    if (e.x == 0ull) {
      const unsigned long long old = atomicCAS(&t[i].fp, 0ull, (unsigned long long)fp);
      if (old == 0ull) { slot = i; return 1; }
      if (old == fp) { slot = i; return 0; }
    }
    i = i + 1 == nslots ? 0 : i + 1;
  }
  return -1;
}

// The next state index for every lane that calls this together: one atomicAdd
// per wave, by the first active lane.
__device__ __forceinline__ uint32_t live_wave_alloc(unsigned int* ctr) {
  const unsigned long long m = __ballot(1);
  const int lane = (int)(threadIdx.x & 63);
  const int leader = __ffsll(m) - 1;
  unsigned int base = 0;
  if (lane == leader) base = atomicAdd(ctr, (unsigned int)__popcll(m));
  base = (unsigned int)__shfl((int)base, leader, 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

template <class M>
__device__ __forceinline__ void live_load(const uint64_t* states, uint32_t i, typename M::State& s) {
  const ulonglong2* p = reinterpret_cast<const ulonglong2*>(states + (uint64_t)i * M::W);
#pragma unroll
  for (int k = 0; k < M::W / 2; ++k) {
    const ulonglong2 v = p[k];
    s.w[2 * k] = v.x;
    s.w[2 * k + 1] = v.y;
  }
}
template <class M>
__device__ __forceinline__ void live_store(uint64_t* states, uint32_t i, const typename M::State& s) {
  ulonglong2* p = reinterpret_cast<ulonglong2*>(states + (uint64_t)i * M::W);
#pragma unroll
  for (int k = 0; k < M::W / 2; ++k) p[k] = make_ulonglong2(s.w[2 * k], s.w[2 * k + 1]);
}

// The Init states: indices 0 .. num_init - 1, level 1.
template <class M>
__global__ void __launch_bounds__(64) k_live_init(LiveArgs a) {
  const uint32_t k = threadIdx.x;
  if (k >= (uint32_t)M::num_init() || k >= a.max_states) return;
  typename M::State s;
  M::init_state((int)k, s, a.flags.variant);
  uint64_t slot = 0;
  if (live_insert(a.table, a.nslots, M::fingerprint(s), slot) <= 0) return;   // Init states are distinct
  live_store<M>(a.states, k, s);
  a.parent[k] = LIVE_NONE;
  a.level[k] = 1;
  a.table[slot].value = k;
}

// One lane per state of the frontier [lo, hi): its successors in
// kc_spec_successors order, each inserted into the table; the inserting lane
// takes the next index and writes the state, its parent and its level.
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_expand(LiveArgs a, uint32_t lo, uint32_t hi, uint32_t lvl) {
  const uint32_t i = lo + blockIdx.x * LIVE_BLOCK + threadIdx.x;
  const bool on = i < hi;
  const int lane = (int)(threadIdx.x & 63);
  typename M::State s;
  typename M::Plan pl{0, 0, -1, -1};
  int total = 0;
  if (on) {
    live_load<M>(a.states, i, s);
    pl = M::plan(s, a.flags);
    if (pl.fail_pos >= 0) {
      const int fs = pl.fail_slot;
      const int self = fs < M::A ? fs : fs < 2 * M::A ? fs - M::A : M::A + (fs - 2 * M::A);
      atomicMin(&a.ctr->err_key, ((unsigned long long)M::slot_action(s, fs) << 8) | (unsigned long long)self);
    } else {
      total = pl.total;
    }
  }
  // this wave's edge range: an inclusive scan of the out-degrees, one add
  int incl = total;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const int wtot = __shfl(incl, 63, 64);
  unsigned long long base = 0;
  if (lane == 63 && wtot) base = atomicAdd(&a.ctr->nedges, (unsigned long long)wtot);
  base = __shfl(base, 63, 64);
  const unsigned long long e0 = base + (unsigned long long)(incl - total);
  if (!on) return;
  if (e0 + (unsigned long long)total > a.max_edges) {
    atomicOr(&a.ctr->overflow, (unsigned)LIVE_OVF_EDGES);
    a.row[i] = make_uint2(0u, 0u);
    return;
  }
  a.row[i] = make_uint2((uint32_t)e0, (uint32_t)total);
  const uint64_t fold = M::fp_fold(s);
  for (int t = 0; t < total; ++t) {
    int slot, j, who;
    sim_locate<M>(pl, t, slot, j);
    typename M::State x;
    M::apply(s, slot, j, a.flags, x, who);
    const uint64_t fp = M::fingerprint_succ(s, fold, x, who);
    uint64_t ts = 0;
    const int r = live_insert(a.table, a.nslots, fp, ts);
    if (r < 0) {
      atomicOr(&a.ctr->overflow, (unsigned)LIVE_OVF_TABLE);
      break;
    }
    if (r > 0) {
      const uint32_t idx = live_wave_alloc(&a.ctr->nstates);
      if (idx >= a.max_states) {
        atomicOr(&a.ctr->overflow, (unsigned)LIVE_OVF_STATES);
        break;
      }
      live_store<M>(a.states, idx, x);
      a.parent[idx] = i;
      a.level[idx] = lvl + 1;
      a.table[ts].value = idx;
    }
    a.edges[e0 + t] = (uint32_t)ts;
    if (a.eproc) a.eproc[e0 + t] = (uint8_t)live_slot_process<M>(slot);
  }
}

// alive = stay; terminal = no successor other than the state itself
template <class M>
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_mark(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool stay = false, term = false;
  if (i < n) {
    typename M::State s;
    live_load<M>(a.states, i, s);
    stay = live_stay<M>(s, a.prop);
    term = live_terminal_of(a, i);
    a.alive[i] = stay;
    a.terminal[i] = term;
  }
  live_wave_count(stay, &a.ctr->stay);
  live_wave_count(stay && term, &a.ctr->stay_terminal);
}

class LiveBase {
 public:
  virtual ~LiveBase() = default;
  virtual int setup() = 0;
  virtual int run(kc_live_result* res) = 0;
  virtual int set_formula(int form, const PredInstr* code, int n_instr) = 0;
  virtual int trace(uint64_t* tuples, int* actions, int cap) = 0;
  virtual int alive(uint64_t* tuples, uint8_t* alive, uint64_t cap) = 0;
  virtual int64_t edge_procs(uint32_t* src, uint32_t* dst, uint8_t* proc, uint64_t cap) = 0;
  virtual int tuple_words() const = 0;
  virtual int state_words() const = 0;
  kc_model_config cfg;
  kc_live_config live;
  uint64_t trigger_stay = 0, trigger_live = 0;   // the last run's, 0 for the built-in properties
};

template <class M>
class LiveT : public LiveBase {
 public:
  ~LiveT() override { (void)hipSetDevice(cfg.device); }   // (the members free themselves on it)
  int tuple_words() const override { return M::TUPLE_WORDS; }
  int state_words() const override { return M::W; }

  int setup() override {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      set_error("kubecheck: no HIP device visible (liveness checking has no CPU fallback)");
      return -ENODEV;
    }
    if (cfg.device < 0 || cfg.device >= ndev) {
      set_error("kubecheck: bad device %d", cfg.device);
      return -EINVAL;
    }
    const uint64_t cap = live.max_states;
    memset(&a_, 0, sizeof a_);
    a_.max_states = cap;
    a_.max_edges = cap * LIVE_EDGES_PER_STATE;
    a_.nslots = cap * 2;
    a_.flags = flags_of(cfg);
    a_.prop = live.property;
    KC_HIP_TRY(hipSetDevice(cfg.device));
    KC_TRY(st_.create(hipStreamNonBlocking));
    // an owner of n elements, and the kernels' plain struct reads its pointer
    auto own = [](auto& arr, auto*& p, uint64_t n) {
      KC_TRY(arr.alloc(n));
      p = arr;
      return 0;
    };
    KC_TRY(own(states_, a_.states, cap * M::W));
    KC_TRY(own(parent_, a_.parent, cap));
    KC_TRY(own(level_, a_.level, cap));
    KC_TRY(own(row_, a_.row, cap));
    KC_TRY(own(edges_, a_.edges, a_.max_edges));
    KC_TRY(own(table_, a_.table, a_.nslots));
    KC_TRY(own(alive_, a_.alive, cap));
    KC_TRY(own(terminal_, a_.terminal, cap));
    KC_TRY(own(stamp_, a_.stamp, cap));
    // per-process fairness: the lasso is the prefix and at most P + 2 legs, each shorter than the graph
    a_.path_cap = live.fairness == LF_Process ? cap * (uint64_t)(M::P + 3) : cap;
    a_.pmask = (1u << M::P) - 1u;
    KC_TRY(own(path_, a_.path, a_.path_cap));
    if (live.fairness == LF_Process) {
      KC_TRY(own(eproc_, a_.eproc, a_.max_edges));
      KC_TRY(own(enabled_, a_.enabled, cap));
      KC_TRY(own(color_, a_.color, cap));
      KC_TRY(own(comp_, a_.comp, cap));
      KC_TRY(own(sccw_, a_.sccw, cap));
      KC_TRY(own(fair_, a_.fair, cap));
      KC_TRY(own(bpar_, a_.bpar, cap));
    }
    KC_TRY(own(ctr_, a_.ctr, 1));
    return h_ctr_.alloc(1);
  }

  // A user formula (a handle of kc_live_create_formula): the program goes to
  // the device and the trigger bytes are allocated, both on first use.
  int set_formula(int form, const PredInstr* code, int n_instr) override {
    if (live.property != KC_LIVE_USER) {
      set_error("kc_live_set_formula: the handle was created with the built-in property %d "
                "(kc_live_create_formula makes one that takes formulas)", live.property);
      return -EINVAL;
    }
    static_assert(live_prog_width_ok(M::W), "k_live_mark_prog: no instantiation for this W");
    if (const char* why = live_formula_check(form, code, n_instr, M::W)) {
      set_error("kc_live_set_formula: %s", why);
      return -EINVAL;
    }
    KC_HIP_TRY(hipSetDevice(cfg.device));
    KC_TRY(trig_.alloc(a_.max_states));
    KC_TRY(prog_.alloc(KC_PRED_MAX_INSTR));
    KC_HIP_TRY(hipMemcpyAsync(prog_, code, (size_t)n_instr * sizeof(PredInstr), hipMemcpyHostToDevice, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));   // (code is the caller's)
    a_.trig = trig_;
    a_.prog = prog_;
    a_.prog_n = n_instr;
    a_.form = form;
    ran_ = false;
    return 0;
  }

  int run(kc_live_result* res) override {
    using clock = std::chrono::steady_clock;
    KC_HIP_TRY(hipSetDevice(cfg.device));
    const auto t0 = clock::now();
    memset(res, 0, sizeof *res);
    res->err_action = res->err_self = -1;
    res->loop_start = -1;
    ran_ = false;
    n_ = ne_ = 0;
    trace_.clear();
    trigger_stay = trigger_live = 0;

    // ---- build
    LiveCounters zero;
    memset(&zero, 0, sizeof zero);
    zero.err_key = ~0ull;
    zero.first_alive = LIVE_NONE;
    zero.nstates = (unsigned)M::num_init();
    KC_HIP_TRY(hipMemcpyAsync(a_.ctr, &zero, sizeof zero, hipMemcpyHostToDevice, st_));
    KC_HIP_TRY(hipMemsetAsync(a_.table, 0, a_.nslots * sizeof(LiveSlot), st_));
    hipLaunchKernelGGL((k_live_init<M>), dim3(1), dim3(64), 0, st_, a_);
    KC_HIP_TRY(hipGetLastError());
    uint32_t lo = 0, hi = (uint32_t)M::num_init(), lvl = 1;
    for (;;) {
      hipLaunchKernelGGL((k_live_expand<M>), dim3(live_grid(hi - lo)), dim3(LIVE_BLOCK), 0, st_, a_, lo, hi, lvl);
      KC_HIP_TRY(hipGetLastError());
      KC_TRY(read_counters());
      if (h_ctr_->err_key != ~0ull) {
        // an Assert: no verdict (the BFS engine is the tool for safety)
        res->err_kind = E_ASSERT;
        res->err_action = (int)(h_ctr_->err_key >> 8);
        res->err_self = (int)(h_ctr_->err_key & 0xff);
        res->states = std::min<uint64_t>(h_ctr_->nstates, a_.max_states);
        res->init = (uint64_t)M::num_init();
        res->depth = (int)lvl;
        res->build_ms = ms_since(t0);
        res->seconds = res->build_ms / 1e3;
        return 0;
      }
      if (h_ctr_->overflow) {
        if (h_ctr_->overflow & (LIVE_OVF_STATES | LIVE_OVF_TABLE))
          set_error("kc_live_run: the reachable graph has more than max_states = %llu states "
                    "(kc_live_config.max_states)", (unsigned long long)a_.max_states);
        else
          set_error("kc_live_run: the reachable graph has more than %llu edges (%llu per state of max_states = %llu)",
                    (unsigned long long)a_.max_edges, (unsigned long long)LIVE_EDGES_PER_STATE,
                    (unsigned long long)a_.max_states);
        return -ENOMEM;
      }
      lo = hi;
      hi = h_ctr_->nstates;
      if (hi == lo) break;
      ++lvl;
    }
    const uint32_t n = hi;
    const uint64_t ne = h_ctr_->nedges;
    if (ne) {
      hipLaunchKernelGGL(k_live_resolve, dim3(live_grid(ne)), dim3(LIVE_BLOCK), 0, st_, a_, ne);
      KC_HIP_TRY(hipGetLastError());
    }
    KC_HIP_TRY(hipStreamSynchronize(st_));
    const auto t1 = clock::now();
    res->states = n;
    res->edges = ne;
    res->init = (uint64_t)M::num_init();
    res->depth = (int)lvl;
    res->build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();

    // ---- mark, then the trim, the SCCs and the lasso (live_graph.h)
    if (a_.trig) live_mark_prog_launch(M::W, a_, n, st_);
    else hipLaunchKernelGGL((k_live_mark<M>), dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
    n_ = n;
    ne_ = ne;
    uint32_t len = 0, kind = 0, loop = 0;
    LiveDriver drv(a_, st_, h_ctr_, n, M::P);
    KC_TRY(drv.run(live.fairness == LF_Process ? 1 : 0, t1, res, len, kind, loop));
    trigger_stay = drv.trig_stay;
    trigger_live = drv.trig_live;

    // ---- counterexample
    if (res->violated) {
      if ((uint64_t)len * M::W > d_trace_.cap) KC_TRY(d_trace_.renew((uint64_t)len * M::W));
      hipLaunchKernelGGL(k_live_gather, dim3(live_grid(len)), dim3(LIVE_BLOCK), 0, st_, a_.states, a_.path, len,
                         (int)M::W, d_trace_);
      KC_HIP_TRY(hipGetLastError());
      trace_.resize((size_t)len * M::W);
      KC_HIP_TRY(hipMemcpyAsync(trace_.data(), d_trace_, trace_.size() * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                st_));
      KC_HIP_TRY(hipStreamSynchronize(st_));
      res->kind = (int)kind;
      res->prefix_len = (int)h_ctr_->lasso_prefix;
      res->trace_len = (int)len;
      res->loop_start = res->kind == 1 ? (int)loop : -1;
    }
    ran_ = true;
    res->seconds = ms_since(t0) / 1e3;
    return 0;
  }

  // The counterexample of the last run: the states gathered from the device,
  // each step's action found by enumerating the successors on the host.
  int trace(uint64_t* tuples, int* actions, int cap) override {
    if (!ran_) { set_error("kc_live_trace: no completed run"); return -EINVAL; }
    const int len = (int)(trace_.size() / M::W);
    const Flags f = flags_of(cfg);
    typename M::State prev{};
    for (int i = 0; i < len && i < cap; ++i) {
      typename M::State s;
      for (int w = 0; w < M::W; ++w) s.w[w] = trace_[(size_t)i * M::W + w];
      if (tuples) M::to_tuple(s, tuples + (size_t)i * M::TUPLE_WORDS);
      if (actions) {
        actions[i] = -1;
        if (i > 0) {
          const typename M::Plan pl = M::plan(prev, f);
          bool found = false;
          for (int t = 0; pl.fail_pos < 0 && t < pl.total && !found; ++t) {
            int slot, j;
            M::locate(pl, t, slot, j);
            typename M::State x;
            M::apply(prev, slot, j, f, x);
            if (memcmp(x.w, s.w, sizeof x.w) == 0) {
              actions[i] = M::slot_action(prev, slot);
              found = true;
            }
          }
          if (!found) {
            set_error("kc_live_trace: state %d is not a successor of state %d", i + 1, i);
            return -EIO;
          }
        }
      }
      prev = s;
    }
    return len;
  }

  int alive(uint64_t* tuples, uint8_t* alive_out, uint64_t cap) override {
    if (!ran_) { set_error("kc_live_alive: no completed run"); return -EINVAL; }
    if (cap < n_ || (!tuples && !alive_out)) return (int)n_;
    KC_HIP_TRY(hipSetDevice(cfg.device));
    std::vector<uint64_t> words;
    if (tuples) {
      words.resize((size_t)n_ * M::W);
      KC_HIP_TRY(hipMemcpyAsync(words.data(), a_.states, words.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st_));
    }
    if (alive_out) KC_HIP_TRY(hipMemcpyAsync(alive_out, a_.alive, n_, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    if (tuples) {
      for (uint64_t i = 0; i < n_; ++i) {
        typename M::State s;
        for (int w = 0; w < M::W; ++w) s.w[w] = words[i * M::W + w];
        M::to_tuple(s, tuples + i * M::TUPLE_WORDS);
      }
    }
    return (int)n_;
  }

  int64_t edge_procs(uint32_t* src, uint32_t* dst, uint8_t* proc, uint64_t cap) override {
    if (!ran_ || !a_.eproc) { set_error("kc_live_edge_procs: no completed run with fairness = 1"); return -EINVAL; }
    if (cap < ne_ || !src || !dst || !proc) return (int64_t)ne_;
    KC_HIP_TRY(hipSetDevice(cfg.device));
    std::vector<uint2> row(n_);
    KC_HIP_TRY(hipMemcpyAsync(row.data(), a_.row, n_ * sizeof(uint2), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipMemcpyAsync(dst, a_.edges, ne_ * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipMemcpyAsync(proc, a_.eproc, ne_, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    for (uint64_t i = 0; i < n_; ++i)
      for (uint32_t k = 0; k < row[i].y && (uint64_t)row[i].x + k < ne_; ++k) src[row[i].x + k] = (uint32_t)i;
    return (int64_t)ne_;
  }

 private:
  static double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  }
  int read_counters() {
    KC_HIP_TRY(hipMemcpyAsync(h_ctr_, a_.ctr, sizeof(LiveCounters), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    return 0;
  }

  OwnedStream st_;   // (first: destroyed after every buffer below)
  LiveArgs a_{};     // the kernels' view of the buffers below
  DeviceArray<uint64_t> states_, d_trace_;
  DeviceArray<uint32_t> parent_, level_, edges_, stamp_, path_, color_, comp_, bpar_;
  DeviceArray<uint2> row_, sccw_;
  DeviceArray<LiveSlot> table_;
  DeviceArray<uint8_t> alive_, terminal_, eproc_, enabled_, fair_, trig_;
  DeviceArray<PredInstr> prog_;   // a user formula's program (trig_ and this: only then)
  DeviceArray<LiveCounters> ctr_;
  PinnedArray<LiveCounters> h_ctr_;
  std::vector<uint64_t> trace_;   // the counterexample's packed states
  uint64_t n_ = 0, ne_ = 0;
  bool ran_ = false;
};

std::unique_ptr<LiveBase> make_live(const kc_model_config& cfg) {
#define KC_MAKE(a, b, c) \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c) return std::unique_ptr<LiveBase>(new LiveT<Model<a, b, c>>());
  KC_FOR_EACH_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}

}  // namespace

}  // namespace kc

using namespace kc;

struct kc_live {
  std::unique_ptr<LiveBase> impl;
};

// kc_live_create (code = nullptr) and kc_live_create_formula: every argument is
// checked before the device is touched, the formula's program among them.
static int live_create(const kc_model_config* cfg, const kc_live_config* live, int form, const PredInstr* code,
                       int n_instr, kc_live** out) {
  if (!cfg || !live || !out) { set_error("kc_live_create: NULL argument"); return -EINVAL; }
  *out = nullptr;
  if (cfg->symmetry) {
    set_error("kc_live_create: symmetry is not supported (liveness checking under symmetry reduction is unsound)");
    return -EINVAL;
  }
  if (con_active(cfg->constraint_stored, cfg->constraint_inflight, cfg->action_constraints)) {
    set_error("kc_live_create: constraints are not supported (the behaviour graph is built from Next alone)");
    return -EINVAL;
  }
  auto impl = make_live(*cfg);
  if (!impl) {
    set_error("kc_live_create: unsupported model nc=%d np=%d ns=%d", cfg->nc, cfg->np, cfg->ns);
    return -EINVAL;
  }
  if (code) {
    if (live->property != KC_LIVE_USER) {
      set_error("kc_live_create_formula: property %d is not KC_LIVE_USER (a built-in property takes no formula)",
                live->property);
      return -EINVAL;
    }
    if (const char* why = live_formula_check(form, code, n_instr, impl->state_words())) {
      set_error("kc_live_create_formula: %s", why);
      return -EINVAL;
    }
  } else if (!live_prop_ok(cfg->nc, live->property)) {
    set_error("kc_live_create: property %d is not defined for nc=%d (0-2 need one client; 3 any model; "
              "KC_LIVE_USER comes with its formula: kc_live_create_formula)", live->property, cfg->nc);
    return -EINVAL;
  }
  impl->cfg = *cfg;
  impl->cfg.spill_dir = nullptr;   // BFS-only fields are not used
  if (live->fairness != LF_Next && live->fairness != LF_Process) {
    set_error("kc_live_create: fairness %d is neither 0 (WF_vars(Next)) nor 1 (per process)", live->fairness);
    return -EINVAL;
  }
  impl->live = *live;
  if (impl->live.max_states == 0) impl->live.max_states = LIVE_DEFAULT_STATES;
  if (impl->live.max_states < LIVE_MIN_STATES || impl->live.max_states > LIVE_MAX_STATES) {
    set_error("kc_live_create: max_states %llu outside 16..2^27", (unsigned long long)live->max_states);
    return -EINVAL;
  }
  KC_TRY(impl->setup());
  if (code) KC_TRY(impl->set_formula(form, code, n_instr));
  *out = new kc_live{std::move(impl)};
  return 0;
}

extern "C" {

int kc_live_create(const kc_model_config* cfg, const kc_live_config* live, kc_live** out) {
  return live_create(cfg, live, 0, nullptr, 0, out);
}

int kc_live_create_formula(const kc_model_config* cfg, const kc_live_config* live, int form, const uint64_t* program,
                           int n_instr, kc_live** out) {
  if (!program) { set_error("kc_live_create_formula: NULL argument"); return -EINVAL; }
  return live_create(cfg, live, form, reinterpret_cast<const PredInstr*>(program), n_instr, out);
}

void kc_live_destroy(kc_live* l) { delete l; }

int kc_live_run(kc_live* l, kc_live_result* res) {
  if (!l || !res) { set_error("kc_live_run: NULL argument"); return -EINVAL; }
  return l->impl->run(res);
}

int kc_live_set_formula(kc_live* l, int form, const uint64_t* program, int n_instr) {
  if (!l || !program) { set_error("kc_live_set_formula: NULL argument"); return -EINVAL; }
  return l->impl->set_formula(form, reinterpret_cast<const PredInstr*>(program), n_instr);
}

int kc_live_trigger_counts(kc_live* l, uint64_t* trigger_stay_out, uint64_t* trigger_live_out) {
  if (!l || !trigger_stay_out || !trigger_live_out) { set_error("kc_live_trigger_counts: NULL argument"); return -EINVAL; }
  *trigger_stay_out = l->impl->trigger_stay;
  *trigger_live_out = l->impl->trigger_live;
  return 0;
}

int kc_live_trace(kc_live* l, uint64_t* tuples_out, int* actions_out, int cap) {
  if (!l) { set_error("kc_live_trace: NULL"); return -EINVAL; }
  return l->impl->trace(tuples_out, actions_out, cap);
}

int64_t kc_live_trace_text(kc_live* l, char* buf, size_t cap) {
  if (!l) { set_error("kc_live_trace_text: NULL"); return -EINVAL; }
  const int n = l->impl->trace(nullptr, nullptr, 0);
  if (n < 0) return n;
  const int tw = l->impl->tuple_words();
  std::vector<uint64_t> t((size_t)n * tw);
  const int n2 = l->impl->trace(t.data(), nullptr, n);
  if (n2 < 0) return n2;
  const kc_model_config& c = l->impl->cfg;
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

int kc_live_alive(kc_live* l, uint64_t* tuples_out, uint8_t* alive_out, uint64_t cap) {
  if (!l) { set_error("kc_live_alive: NULL"); return -EINVAL; }
  return l->impl->alive(tuples_out, alive_out, cap);
}

int64_t kc_live_edge_procs(kc_live* l, uint32_t* src_out, uint32_t* dst_out, uint8_t* proc_out, uint64_t cap) {
  if (!l) { set_error("kc_live_edge_procs: NULL"); return -EINVAL; }
  return l->impl->edge_procs(src_out, dst_out, proc_out, cap);
}

// host only: the process of the step to successor `ordinal`, through the code k_live_expand runs
int kc_live_step_process(const kc_model_config* cfg, const uint64_t* tuple, int ordinal) {
  if (!cfg || !tuple) { set_error("kc_live_step_process: NULL"); return -EINVAL; }
#define KC_STEP(a, b, c)                                                                          \
  if (cfg->nc == a && cfg->np == b && cfg->ns == c) {                                             \
    using M = Model<a, b, c>;                                                                     \
    M::State s;                                                                                   \
    if (!M::from_tuple(tuple, s)) {                                                               \
      set_error("kc_live_step_process: tuple outside the lowered domain");                        \
      return -EINVAL;                                                                             \
    }                                                                                             \
    const M::Plan pl = M::plan(s, flags_of(*cfg));                                                \
    if (pl.fail_pos >= 0 || ordinal < 0 || ordinal >= pl.total) {                                 \
      set_error("kc_live_step_process: the state has no successor %d", ordinal);                  \
      return -EINVAL;                                                                             \
    }                                                                                             \
    int slot, j;                                                                                  \
    sim_locate<M>(pl, ordinal, slot, j);                                                          \
    return live_slot_process<M>(slot);                                                            \
  }
  KC_FOR_EACH_MODEL(KC_STEP)
#undef KC_STEP
  set_error("kc_live_step_process: unsupported model nc=%d np=%d ns=%d", cfg->nc, cfg->np, cfg->ns);
  return -EINVAL;
}

// host only: stay(tuple) of a property, through the code the kernels run
int kc_live_stay(const kc_model_config* cfg, int property, const uint64_t* tuple) {
  if (!cfg || !tuple) { set_error("kc_live_stay: NULL"); return -EINVAL; }
#define KC_STAY(a, b, c)                                                                          \
  if (cfg->nc == a && cfg->np == b && cfg->ns == c) {                                             \
    using M = Model<a, b, c>;                                                                     \
    if (!live_prop_ok(M::NC, property)) {                                                         \
      set_error("kc_live_stay: property %d is not defined for nc=%d", property, cfg->nc);         \
      return -EINVAL;                                                                             \
    }                                                                                             \
    M::State s;                                                                                   \
    if (!M::from_tuple(tuple, s)) { set_error("kc_live_stay: tuple outside the lowered domain"); return -EINVAL; } \
    return live_stay<M>(s, property) ? 1 : 0;                                                     \
  }
  KC_FOR_EACH_MODEL(KC_STAY)
#undef KC_STAY
  set_error("kc_live_stay: unsupported model nc=%d np=%d ns=%d", cfg->nc, cfg->np, cfg->ns);
  return -EINVAL;
}

}  // extern "C"
