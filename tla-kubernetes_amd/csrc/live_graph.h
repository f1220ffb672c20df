// live_graph.h — the part of the liveness checker that works on the graph as
// built and does not depend on the model type: the kernels' view of the
// buffers (LiveArgs, LiveCounters, LiveLeg), the kernels of the trim, the SCC
// decomposition, F and the closure to L and the lassos, and LiveDriver, the
// host loops that launch them.  liveness.hip (LiveT<M>: setup, the build,
// k_live_mark<M>, the trace) and the test-only live_selftest.hip include it and
// run the same code; liveness.hip's header comment has the phases.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "owned.h"
#include "pred.h"

namespace kc {

namespace {

constexpr int LIVE_BLOCK = 256;
constexpr uint32_t LIVE_NONE = 0xffffffffu;

// 16-B table slot, probed with one 16-B load as ClaimEntry is.  fp 0 = empty;
// value = the state's index, stored by the lane whose CAS inserted fp and read
// only by later launches.
struct LiveSlot {
  unsigned long long fp;
  unsigned long long value;
};

struct LiveCounters {
  unsigned long long nedges;          // edge slots handed out
  unsigned long long err_key;         // min over Assert states of action << 8 | self; ~0 = none
  unsigned long long stay;            // |S|
  unsigned long long stay_terminal;   // terminal states in S (they never die)
  unsigned long long removed;         // states the trim rounds removed so far
  unsigned int nstates;
  unsigned int overflow;              // LIVE_OVF_*
  unsigned int first_alive;           // smallest index in L
  unsigned int lasso_kind, lasso_len, lasso_loop, lasso_prefix;
  unsigned int pad;
  // per-process fairness
  unsigned long long scc_open;        // states the reset launches left unassigned, summed
  unsigned long long changed;         // states a push / pull / close / reach launch changed, summed
  unsigned long long sccs, fair_sccs, fair_states;
  unsigned long long live, live_terminal;   // |L| and its terminal states
  unsigned int hit;                   // reach: the smallest target index of the first level with one
  unsigned int lasso_cur;             // the lasso's last state
  unsigned int lasso_cov;             // processes the cycle has a witness for so far
  unsigned int lasso_term, lasso_scc; // terminal[lasso_cur], comp[lasso_cur]
  unsigned int lasso_err;             // the path buffer is full
  // a user formula (LiveArgs::trig set; 0 otherwise)
  unsigned long long trig_stay;       // |S /\ T|
  unsigned long long trig_live;       // |L /\ T|
};

struct LiveArgs {
  uint64_t* states;       // state i at [i * M::W]
  uint32_t* parent;       // BFS parent (LIVE_NONE for Init states)
  uint32_t* level;        // BFS level, Init = 1
  uint2* row;             // {first edge, out-degree}
  uint32_t* edges;        // successor's table slot, then (k_live_resolve) its index
  LiveSlot* table;
  uint64_t nslots;
  uint8_t* alive;
  uint8_t* terminal;
  uint32_t* stamp;        // lasso: position in path + 1, 0 = not visited
  uint32_t* path;         // lasso: prefix, then the walk inside L
  LiveCounters* ctr;
  uint64_t max_states, max_edges;
  Flags flags;
  int prop;
  // per-process fairness (all null under WF_vars(Next))
  uint8_t* eproc;         // parallel to edges: the process that takes the step
  uint8_t* enabled;       // mask of the processes with a successor other than the state
  uint32_t* color;        // SCC rounds: the largest index of an unassigned ancestor
  uint32_t* comp;         // the SCC's root (its largest index at the round that found it); LIVE_NONE = unassigned
  uint2* sccw;            // at an SCC's root: {states, witness mask}
  uint8_t* fair;          // in F
  uint32_t* bpar;         // reach: the state that discovered this one
  uint64_t path_cap;      // entries of path
  uint32_t pmask;         // (1 << P) - 1
  // a user formula (all null / 0 for the built-in properties)
  uint8_t* trig;          // in the trigger set T
  const PredInstr* prog;  // END 0 = P, END 1 = Q (pred.h), in device memory
  int prog_n;             // its instructions
  int form;               // 0: T = P (P ~> Q); 1: T = the Init states (<>Q)
};

// alive[] while F and L are computed: bit 0 = survived the trim, bit 1 = reaches F
enum : uint8_t { LIVE_TRIMMED = 1, LIVE_REACHES = 3 };

// One leg of the lasso: a reach from the lasso's last state, inside the whole
// of L (scc = LIVE_NONE) or one SCC, to the first level holding a target.
enum : int {
  LEG_FAIR = 0,      // a state of F
  LEG_WITNESS = 1,   // a state with process arg disabled, or with an arg step inside the SCC
  LEG_STATE = 2      // a predecessor of state arg (the cycle's first; never the leg's own start)
};
struct LiveLeg {
  int target;
  uint32_t arg;
  uint32_t scc;
};

// counter += lanes of this wave with pred (every lane of the wave calls it)
__device__ __forceinline__ void live_wave_count(bool pred, unsigned long long* ctr) {
  const unsigned long long m = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

// edges: table slot -> state index (every index is stored by now)
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_resolve(LiveArgs a, uint64_t nedges) {
  const uint64_t e = (uint64_t)blockIdx.x * LIVE_BLOCK + threadIdx.x;
  if (e >= nedges) return;
  const uint32_t slot = a.edges[e];
  a.edges[e] = slot < a.nslots ? (uint32_t)a.table[slot].value : LIVE_NONE;
}

// terminal(i): no successor other than the state itself
__device__ __forceinline__ bool live_terminal_of(const LiveArgs& a, uint32_t i) {
  const uint2 r = a.row[i];
  for (uint32_t k = 0; k < r.y; ++k)
    if (a.edges[r.x + k] != i) return false;
  return true;
}

// One round: an alive, non-terminal state with no alive successor other than
// itself dies.  In place: a lane may or may not see this round's deaths, which
// changes the number of rounds only (alive bits only ever fall, and a round
// that removes nothing wrote nothing, so what it read was current).
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_trim(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool die = false;
  if (i < n && a.alive[i] && !a.terminal[i]) {
    const uint2 r = a.row[i];
    die = true;
    for (uint32_t k = 0; k < r.y; ++k) {
      const uint32_t t = a.edges[r.x + k];
      if (t != i && t < n && a.alive[t]) { die = false; break; }
    }
    if (die) a.alive[i] = 0;
  }
  live_wave_count(die, &a.ctr->removed);
}

// the smallest index in L = its smallest (level, index): levels are index ranges
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_first(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  const unsigned long long m = __ballot(i < n && a.alive[i]);
  if ((threadIdx.x & 63) == 0 && m) atomicMin(&a.ctr->first_alive, i + (uint32_t)(__ffsll(m) - 1));
}

// A user formula: the smallest index in L /\ T, and |L /\ T|
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_first_trig(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  const unsigned long long m = __ballot(i < n && a.alive[i] && a.trig[i]);
  if ((threadIdx.x & 63) == 0 && m) {
    atomicMin(&a.ctr->first_alive, i + (uint32_t)(__ffsll(m) - 1));
    atomicAdd(&a.ctr->trig_live, (unsigned long long)__popcll(m));
  }
}

// A single lane: the parent chain of the first L state into path[0 .. prefix),
// then from that state the first alive successor other than itself, in
// kc_spec_successors order, until a stamped state (a cycle) or a terminal one.
__global__ void __launch_bounds__(64) k_live_lasso(LiveArgs a, uint32_t n) {
  if (blockIdx.x || threadIdx.x) return;
  LiveCounters* c = a.ctr;
  c->lasso_kind = 0;
  c->lasso_len = c->lasso_loop = c->lasso_prefix = 0;
  uint32_t cur = c->first_alive;
  if (cur >= n) return;
  const uint32_t prefix = a.level[cur];
  if (prefix < 1 || prefix > n) return;
  uint32_t p = cur;
  for (uint32_t k = prefix; k-- > 0;) {
    if (p >= n) return;
    a.path[k] = p;
    p = a.parent[p];
  }
  uint32_t len = prefix, kind = 0, loop = 0;
  a.stamp[cur] = len;
  for (;;) {
    if (a.terminal[cur]) { kind = 2; break; }
    const uint2 r = a.row[cur];
    uint32_t nx = LIVE_NONE;
    for (uint32_t k = 0; k < r.y; ++k) {
      const uint32_t t = a.edges[r.x + k];
      if (t != cur && t < n && a.alive[t]) { nx = t; break; }
    }
    if (nx == LIVE_NONE) break;            // not a fixed point: reported as an error
    if (a.stamp[nx]) { kind = 1; loop = a.stamp[nx] - 1; break; }
    if (len >= a.max_states) break;
    a.path[len++] = nx;
    a.stamp[nx] = len;
    cur = nx;
  }
  c->lasso_kind = kind;
  c->lasso_len = len;
  c->lasso_loop = loop;
  c->lasso_prefix = prefix;
}

// ---- per-process fairness ---------------------------------------------------
// All kernels below are one lane per state over the whole index range, no
// frontier; a state outside the alive set is skipped.  `open` = alive and not
// yet assigned to an SCC.

__device__ __forceinline__ bool live_open(const LiveArgs& a, uint32_t n, uint32_t t) {
  return t < n && a.alive[t] && a.comp[t] == LIVE_NONE;
}

// enabled(s): the processes with a successor other than s
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_enabled(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint2 r = a.row[i];
  unsigned m = 0;
  for (uint32_t k = 0; k < r.y; ++k)
    if (a.edges[r.x + k] != i) m |= 1u << a.eproc[r.x + k];
  a.enabled[i] = (uint8_t)m;
}

// Start of an SCC round: an open state with no open successor other than itself
// is an SCC of its own; every other open state takes its index as its colour.
// In place: a lane that misses a neighbour's assignment keeps its state open
// for this round, where it comes out as its own root.
__global__ void __launch_bounds__(LIVE_BLOCK) k_scc_reset(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool open = false;
  if (live_open(a, n, i)) {
    const uint2 r = a.row[i];
    for (uint32_t k = 0; k < r.y; ++k) {
      const uint32_t t = a.edges[r.x + k];
      if (t != i && live_open(a, n, t)) { open = true; break; }
    }
    if (open) a.color[i] = i;
    else a.comp[i] = i;
  }
  live_wave_count(open, &a.ctr->scc_open);
}

// One round of forward max-colour propagation among the open states.  In place:
// colours only rise, and every value is the index of an open ancestor, so a
// stale read costs rounds only; a round that raised nothing wrote nothing, so
// what it read was current and color = the largest open ancestor everywhere.
__global__ void __launch_bounds__(LIVE_BLOCK) k_scc_push(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool ch = false;
  if (live_open(a, n, i)) {
    const uint32_t c = a.color[i];
    const uint2 r = a.row[i];
    for (uint32_t k = 0; k < r.y; ++k) {
      const uint32_t t = a.edges[r.x + k];
      if (t != i && live_open(a, n, t) && a.color[t] < c) {
        atomicMax(&a.color[t], c);
        ch = true;
      }
    }
  }
  live_wave_count(ch, &a.ctr->changed);
}

// One round of the backward closure: a root (its colour is its own index) joins
// its SCC, and so does an open state with a successor of its colour that has
// joined.  comp[t] == c cannot be left from an earlier SCC round: c is the
// index of a state that was open at this round's reset.
__global__ void __launch_bounds__(LIVE_BLOCK) k_scc_pull(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool ch = false;
  if (live_open(a, n, i)) {
    const uint32_t c = a.color[i];
    if (c == i) {
      ch = true;
    } else {
      const uint2 r = a.row[i];
      for (uint32_t k = 0; k < r.y; ++k) {
        const uint32_t t = a.edges[r.x + k];
        if (t != i && t < n && a.alive[t] && a.comp[t] == c) { ch = true; break; }
      }
    }
    if (ch) a.comp[i] = c;
  }
  live_wave_count(ch, &a.ctr->changed);
}

// Per SCC, at its root: the number of states, and the OR of the processes
// disabled in a member and of the processes of the edges inside it.
__global__ void __launch_bounds__(LIVE_BLOCK) k_scc_accum(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  if (i >= n || !a.alive[i]) return;
  const uint32_t c = a.comp[i];
  if (c >= n) return;
  unsigned w = ~(unsigned)a.enabled[i] & a.pmask;
  const uint2 r = a.row[i];
  for (uint32_t k = 0; k < r.y; ++k) {
    const uint32_t t = a.edges[r.x + k];
    if (t != i && t < n && a.alive[t] && a.comp[t] == c) w |= 1u << a.eproc[r.x + k];
  }
  atomicAdd(&a.sccw[c].x, 1u);
  if (w) atomicOr(&a.sccw[c].y, w);
}

// F: the terminal states and the states of the fair SCCs
__global__ void __launch_bounds__(LIVE_BLOCK) k_fair_mark(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool f = false, root = false, froot = false;
  if (i < n) {
    if (a.alive[i]) {
      const uint32_t c = a.comp[i];
      const uint2 w = c < n ? a.sccw[c] : make_uint2(0u, 0u);
      const bool fair_scc = w.x > 1 && w.y == a.pmask;
      f = a.terminal[i] || fair_scc;
      root = w.x > 1 && c == i;
      froot = root && fair_scc;
      if (f) a.alive[i] = LIVE_REACHES;
    }
    a.fair[i] = f;
  }
  live_wave_count(f, &a.ctr->fair_states);
  live_wave_count(root, &a.ctr->sccs);
  live_wave_count(froot, &a.ctr->fair_sccs);
}

// One round of the closure to L: a trimmed state with a successor that reaches
// F reaches F.  In place, as k_live_trim (bits only ever rise).
__global__ void __launch_bounds__(LIVE_BLOCK) k_fair_close(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool ch = false;
  if (i < n && a.alive[i] == LIVE_TRIMMED) {
    const uint2 r = a.row[i];
    for (uint32_t k = 0; k < r.y; ++k) {
      const uint32_t t = a.edges[r.x + k];
      if (t != i && t < n && a.alive[t] == LIVE_REACHES) { ch = true; break; }
    }
    if (ch) a.alive[i] = LIVE_REACHES;
  }
  live_wave_count(ch, &a.ctr->changed);
}

// alive = in L
__global__ void __launch_bounds__(LIVE_BLOCK) k_fair_finish(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool in = false, term = false;
  if (i < n) {
    in = a.alive[i] == LIVE_REACHES;
    term = in && a.terminal[i];
    a.alive[i] = in;
  }
  live_wave_count(in, &a.ctr->live);
  live_wave_count(term, &a.ctr->live_terminal);
}

__device__ __forceinline__ bool live_in_leg(const LiveArgs& a, uint32_t n, uint32_t t, const LiveLeg& leg) {
  return t < n && a.alive[t] && (leg.scc == LIVE_NONE || a.comp[t] == leg.scc);
}
// the target of v's first step of process p that stays inside the leg's domain
__device__ __forceinline__ uint32_t live_step_of(const LiveArgs& a, uint32_t n, uint32_t v, uint32_t p,
                                                 const LiveLeg& leg) {
  const uint2 r = a.row[v];
  for (uint32_t k = 0; k < r.y; ++k) {
    const uint32_t t = a.edges[r.x + k];
    if (t != v && a.eproc[r.x + k] == p && live_in_leg(a, n, t, leg)) return t;
  }
  return LIVE_NONE;
}
__device__ __forceinline__ bool live_is_target(const LiveArgs& a, uint32_t n, uint32_t v, const LiveLeg& leg) {
  if (leg.target == LEG_FAIR) return a.fair[v] != 0;
  if (leg.target == LEG_STATE) return v == leg.arg;
  return !((a.enabled[v] >> leg.arg) & 1u) || live_step_of(a, n, v, leg.arg, leg) != LIVE_NONE;
}

// A single lane: the parent chain of the first L state into path[0 .. prefix)
__global__ void __launch_bounds__(64) k_live_chain(LiveArgs a, uint32_t n) {
  if (blockIdx.x || threadIdx.x) return;
  LiveCounters* c = a.ctr;
  c->lasso_kind = c->lasso_len = c->lasso_loop = c->lasso_prefix = 0;
  const uint32_t cur = c->first_alive;
  if (cur >= n) return;
  const uint32_t prefix = a.level[cur];
  if (prefix < 1 || prefix > n || prefix > a.path_cap) return;
  uint32_t p = cur;
  for (uint32_t k = prefix; k-- > 0;) {
    if (p >= n) return;
    a.path[k] = p;
    p = a.parent[p];
  }
  c->lasso_len = c->lasso_prefix = prefix;
  c->lasso_cur = cur;
}

// A single lane, before a leg's reach (stamp is all 0): the lasso's last state
// is level 1.
__global__ void __launch_bounds__(64) k_live_seed(LiveArgs a, uint32_t n, LiveLeg leg) {
  if (blockIdx.x || threadIdx.x) return;
  LiveCounters* c = a.ctr;
  const uint32_t cur = c->lasso_cur;
  c->hit = LIVE_NONE;
  if (cur >= n) return;
  a.stamp[cur] = 1;
  if (leg.target != LEG_STATE && live_is_target(a, n, cur, leg)) c->hit = cur;
}

// One level of a leg's reach: a state of level lvl gives its unvisited
// successors inside the leg's domain level lvl + 1; the lane whose CAS stamps a
// state is its parent.  stamp = level, 0 = not visited.
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_reach(LiveArgs a, uint32_t n, LiveLeg leg, uint32_t lvl) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool ch = false;
  if (i < n && a.stamp[i] == lvl) {
    const uint2 r = a.row[i];
    for (uint32_t k = 0; k < r.y; ++k) {
      const uint32_t t = a.edges[r.x + k];
      if (t == i || !live_in_leg(a, n, t, leg) || a.stamp[t] != 0) continue;
      if (atomicCAS(&a.stamp[t], 0u, lvl + 1) != 0u) continue;
      a.bpar[t] = i;
      ch = true;
      if (live_is_target(a, n, t, leg)) atomicMin(&a.ctr->hit, t);
    }
  }
  live_wave_count(ch, &a.ctr->changed);
}

// A single lane, after a leg's reach found ctr->hit: the path from the lasso's
// last state to the hit is appended (LEG_STATE: to the hit's parent), then for
// a witness that is a step, the step; the cycle's witnesses are brought up to
// date from what was appended.  The state LEG_FAIR ends in is the cycle's first.
__global__ void __launch_bounds__(64) k_live_walk(LiveArgs a, uint32_t n, LiveLeg leg) {
  if (blockIdx.x || threadIdx.x) return;
  LiveCounters* c = a.ctr;
  const uint32_t hit = c->hit, len = c->lasso_len;
  if (hit >= n || len < 1) { c->lasso_err = 1; return; }
  uint32_t steps = a.stamp[hit] - 1, end = hit;
  if (leg.target == LEG_STATE) {
    if (steps < 1) { c->lasso_err = 1; return; }
    --steps;
    end = a.bpar[hit];
  }
  if (steps >= n || (uint64_t)len + steps + 1 > a.path_cap) { c->lasso_err = 1; return; }
  uint32_t v = end;
  for (uint32_t k = len + steps; k-- > len;) {
    a.path[k] = v;
    v = a.bpar[v];
  }
  uint32_t nl = len + steps;
  if (leg.target == LEG_WITNESS && ((a.enabled[hit] >> leg.arg) & 1u)) {
    const uint32_t t = live_step_of(a, n, hit, leg.arg, leg);
    if (t == LIVE_NONE) { c->lasso_err = 1; return; }
    a.path[nl++] = t;
  }
  unsigned cov = c->lasso_cov;
  for (uint32_t k = len - 1; k + 1 < nl; ++k) {
    const uint32_t x = a.path[k], y = a.path[k + 1];
    const uint2 r = a.row[x];
    for (uint32_t e = 0; e < r.y; ++e)
      if (a.edges[r.x + e] == y) cov |= 1u << a.eproc[r.x + e];
    cov |= ~(unsigned)a.enabled[y] & a.pmask;
  }
  const uint32_t cur = a.path[nl - 1];
  if (leg.target == LEG_FAIR) {
    c->lasso_loop = nl - 1;
    cov = ~(unsigned)a.enabled[cur] & a.pmask;
  }
  c->lasso_len = nl;
  c->lasso_cur = cur;
  c->lasso_cov = cov;
  c->lasso_term = a.terminal[cur];
  c->lasso_scc = a.comp[cur];
}

// out[k] = state path[k], W words each
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_gather(const uint64_t* states, const uint32_t* path, uint32_t len,
                                                            int W, uint64_t* out) {
  const uint32_t k = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  if (k >= len) return;
  const uint64_t* s = states + (uint64_t)path[k] * W;
  for (int w = 0; w < W; ++w) out[(uint64_t)k * W + w] = s[w];
}

inline unsigned live_grid(uint64_t n) { return (unsigned)((n + LIVE_BLOCK - 1) / LIVE_BLOCK); }
// The host loops over a graph of n states and P processes as built in `a`
// (alive = stay and terminal already marked): every launch goes to `st`, every
// counter read into the pinned `h_ctr`.
class LiveDriver {
 public:
  LiveDriver(const LiveArgs& a, hipStream_t st, LiveCounters* h_ctr, uint32_t n, int P)
      : a_(a), st_(st), h_ctr_(h_ctr), n_(n), P_(P) {}

  static double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  }
  int read_counters() {
    KC_HIP_TRY(hipMemcpyAsync(h_ctr_, a_.ctr, sizeof(LiveCounters), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    return 0;
  }

  uint64_t trig_stay = 0, trig_live = 0;   // a user formula's |S /\ T| and |L /\ T| after run

  // Everything after the mark launch (issued at t1): the trim, under
  // per-process fairness the SCCs, F and L, and the counterexample into
  // path[0 .. len).
  int run(int fairness, std::chrono::steady_clock::time_point t1, kc_live_result* res, uint32_t& len, uint32_t& kind,
          uint32_t& loop) {
    const uint32_t n = n_;
    uint64_t removed = 0, rounds = 0;
    for (;;) {
      hipLaunchKernelGGL(k_live_trim, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
      KC_HIP_TRY(hipGetLastError());
      KC_TRY(read_counters());
      ++rounds;
      if (h_ctr_->removed == removed) break;
      removed = h_ctr_->removed;
    }
    res->trim_ms = ms_since(t1);
    res->rounds = rounds;
    res->stay_states = h_ctr_->stay;
    res->live_states = h_ctr_->stay - removed;
    res->live_terminal = h_ctr_->stay_terminal;
    res->violated = res->live_states > 0;
    if (fairness == 1) KC_TRY(fair_sccs(n, res));
    // a user formula: L is final; violated iff a state of L is in the trigger
    // set, and the counterexample starts at the first such state
    if (a_.trig) {
      hipLaunchKernelGGL(k_live_first_trig, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
      KC_HIP_TRY(hipGetLastError());
      KC_TRY(read_counters());
      trig_stay = h_ctr_->trig_stay;
      trig_live = h_ctr_->trig_live;
      res->violated = h_ctr_->first_alive < n;
    }

    // ---- counterexample
    if (res->violated) {
      if (fairness == 1) {
        KC_TRY(fair_lasso(n, res, len, kind, loop));
      } else {
        KC_HIP_TRY(hipMemsetAsync(a_.stamp, 0, (size_t)n * sizeof(uint32_t), st_));
        if (!a_.trig) {
          hipLaunchKernelGGL(k_live_first, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
          KC_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_live_lasso, dim3(1), dim3(64), 0, st_, a_, n);
        KC_HIP_TRY(hipGetLastError());
        KC_TRY(read_counters());
        len = h_ctr_->lasso_len;
        kind = h_ctr_->lasso_kind;
        loop = h_ctr_->lasso_loop;
        if (kind < 1 || kind > 2 || len < 1 || len > n || h_ctr_->lasso_prefix < 1 || h_ctr_->lasso_prefix > len) {
          set_error("kc_live_run: no counterexample from state %u although %llu states are live",
                    h_ctr_->first_alive, (unsigned long long)res->live_states);
          return -EIO;
        }
      }
    }
    return 0;
  }

 private:
  // Per-process fairness, after the trim: the SCCs of the alive subgraph, F,
  // L (alive = L at the end) and the result's counters.
  int fair_sccs(uint32_t n, kc_live_result* res) {
    const auto t0 = std::chrono::steady_clock::now();
    const dim3 grid(live_grid(n)), block(LIVE_BLOCK);
    uint64_t launches = 0;
    KC_HIP_TRY(hipMemsetAsync(a_.comp, 0xff, (size_t)n * sizeof(uint32_t), st_));
    KC_HIP_TRY(hipMemsetAsync(a_.sccw, 0, (size_t)n * sizeof(uint2), st_));
    hipLaunchKernelGGL(k_live_enabled, grid, block, 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
    uint64_t open = 0, changed = 0;
    // a launch, a counter read: did it change anything?
    auto step = [&](void (*k)(LiveArgs, uint32_t)) -> int {
      hipLaunchKernelGGL(k, grid, block, 0, st_, a_, n);
      KC_HIP_TRY(hipGetLastError());
      KC_TRY(read_counters());
      ++launches;
      const bool ch = h_ctr_->changed != changed;
      changed = h_ctr_->changed;
      return ch ? 1 : 0;
    };
    for (;;) {
      hipLaunchKernelGGL(k_scc_reset, grid, block, 0, st_, a_, n);
      KC_HIP_TRY(hipGetLastError());
      KC_TRY(read_counters());
      ++launches;
      if (h_ctr_->scc_open == open) break;       // nothing is left open
      open = h_ctr_->scc_open;
      for (int r = 1; r > 0;) KC_TRY(r = step(k_scc_push));
      for (int r = 1; r > 0;) KC_TRY(r = step(k_scc_pull));
    }
    hipLaunchKernelGGL(k_scc_accum, grid, block, 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fair_mark, grid, block, 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
    for (int r = 1; r > 0;) KC_TRY(r = step(k_fair_close));
    hipLaunchKernelGGL(k_fair_finish, grid, block, 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
    KC_TRY(read_counters());
    res->sccs = h_ctr_->sccs;
    res->fair_sccs = h_ctr_->fair_sccs;
    res->fair_states = h_ctr_->fair_states;
    res->scc_rounds = launches;
    res->live_states = h_ctr_->live;
    res->live_terminal = h_ctr_->live_terminal;
    res->violated = res->fair_states > 0;
    res->scc_ms = ms_since(t0);
    return 0;
  }

  // One leg: reach from the lasso's last state to the first level with a
  // target, then append the path to it.
  int fair_leg(uint32_t n, const LiveLeg& leg) {
    const dim3 grid(live_grid(n)), block(LIVE_BLOCK);
    KC_HIP_TRY(hipMemsetAsync(a_.stamp, 0, (size_t)n * sizeof(uint32_t), st_));
    hipLaunchKernelGGL(k_live_seed, dim3(1), dim3(64), 0, st_, a_, n, leg);
    KC_HIP_TRY(hipGetLastError());
    KC_TRY(read_counters());
    for (uint32_t lvl = 1; h_ctr_->hit == LIVE_NONE; ++lvl) {
      const uint64_t before = h_ctr_->changed;
      hipLaunchKernelGGL(k_live_reach, grid, block, 0, st_, a_, n, leg, lvl);
      KC_HIP_TRY(hipGetLastError());
      KC_TRY(read_counters());
      if (h_ctr_->hit == LIVE_NONE && (h_ctr_->changed == before || lvl >= n)) {
        set_error("kc_live_run: no counterexample: leg %d (arg %u, SCC %u) from state %u reaches no target",
                  leg.target, leg.arg, leg.scc, h_ctr_->lasso_cur);
        return -EIO;
      }
    }
    hipLaunchKernelGGL(k_live_walk, dim3(1), dim3(64), 0, st_, a_, n, leg);
    KC_HIP_TRY(hipGetLastError());
    KC_TRY(read_counters());
    if (h_ctr_->lasso_err) {
      set_error("kc_live_run: no counterexample: the path of leg %d (arg %u) does not fit", leg.target, leg.arg);
      return -EIO;
    }
    return 0;
  }

  // The counterexample under per-process fairness into path[0 .. len).
  int fair_lasso(uint32_t n, kc_live_result* res, uint32_t& len, uint32_t& kind, uint32_t& loop) {
    if (!a_.trig) {
      hipLaunchKernelGGL(k_live_first, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
      KC_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_live_chain, dim3(1), dim3(64), 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
    KC_TRY(read_counters());
    if (h_ctr_->lasso_prefix < 1) {
      set_error("kc_live_run: no counterexample from state %u although %llu states are live",
                h_ctr_->first_alive, (unsigned long long)res->live_states);
      return -EIO;
    }
    KC_TRY(fair_leg(n, LiveLeg{LEG_FAIR, 0u, LIVE_NONE}));
    if (h_ctr_->lasso_term) {
      kind = 2;
      len = h_ctr_->lasso_len;
      return 0;
    }
    const uint32_t scc = h_ctr_->lasso_scc, first = h_ctr_->lasso_cur;
    loop = h_ctr_->lasso_loop;
    for (uint32_t p = 0; p < (uint32_t)P_; ++p)
      if (!((h_ctr_->lasso_cov >> p) & 1u)) KC_TRY(fair_leg(n, LiveLeg{LEG_WITNESS, p, scc}));
    if (h_ctr_->lasso_cur != first) KC_TRY(fair_leg(n, LiveLeg{LEG_STATE, first, scc}));
    len = h_ctr_->lasso_len;
    if (h_ctr_->lasso_cur == first) --len;      // the last step taken already closed the cycle
    if (len <= loop || h_ctr_->lasso_cov != a_.pmask) {
      set_error("kc_live_run: no counterexample: the cycle from state %u is empty or lacks a witness (%x)", first,
                h_ctr_->lasso_cov);
      return -EIO;
    }
    kind = 1;
    return 0;
  }

  const LiveArgs& a_;
  hipStream_t st_;
  LiveCounters* h_ctr_;
  uint32_t n_;
  int P_;
};

}  // namespace

}  // namespace kc
