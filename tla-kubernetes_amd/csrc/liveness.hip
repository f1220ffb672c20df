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
#include "liveness.h"
#include "simulate.h"

namespace kc {

namespace {

constexpr int LIVE_BLOCK = 256;
constexpr uint64_t LIVE_DEFAULT_STATES = 1ull << 24;
constexpr uint64_t LIVE_MIN_STATES = 16;            // every model's Init states fit
constexpr uint64_t LIVE_MAX_STATES = 1ull << 27;    // edge offsets stay below 2^31
constexpr uint64_t LIVE_EDGES_PER_STATE = 8;        // edge capacity = 8 x max_states
constexpr uint32_t LIVE_NONE = 0xffffffffu;
enum : unsigned { LIVE_OVF_STATES = 1, LIVE_OVF_EDGES = 2, LIVE_OVF_TABLE = 4 };

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

// counter += lanes of this wave with pred (every lane of the wave calls it)
__device__ __forceinline__ void live_wave_count(bool pred, unsigned long long* ctr) {
  const unsigned long long m = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr, (unsigned long long)__popcll(m));
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

// edges: table slot -> state index (every index is stored by now)
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_resolve(LiveArgs a, uint64_t nedges) {
  const uint64_t e = (uint64_t)blockIdx.x * LIVE_BLOCK + threadIdx.x;
  if (e >= nedges) return;
  const uint32_t slot = a.edges[e];
  a.edges[e] = slot < a.nslots ? (uint32_t)a.table[slot].value : LIVE_NONE;
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
    const uint2 r = a.row[i];
    term = true;
    for (uint32_t k = 0; k < r.y; ++k)
      if (a.edges[r.x + k] != i) { term = false; break; }
    a.alive[i] = stay;
    a.terminal[i] = term;
  }
  live_wave_count(stay, &a.ctr->stay);
  live_wave_count(stay && term, &a.ctr->stay_terminal);
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

class LiveBase {
 public:
  virtual ~LiveBase() = default;
  virtual int setup() = 0;
  virtual int run(kc_live_result* res) = 0;
  virtual int trace(uint64_t* tuples, int* actions, int cap) = 0;
  virtual int alive(uint64_t* tuples, uint8_t* alive, uint64_t cap) = 0;
  virtual int64_t edge_procs(uint32_t* src, uint32_t* dst, uint8_t* proc, uint64_t cap) = 0;
  virtual int tuple_words() const = 0;
  kc_model_config cfg;
  kc_live_config live;
};

template <class M>
class LiveT : public LiveBase {
 public:
  ~LiveT() override { (void)hipSetDevice(cfg.device); }   // (the members free themselves on it)
  int tuple_words() const override { return M::TUPLE_WORDS; }

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

    // ---- mark and trim
    hipLaunchKernelGGL((k_live_mark<M>), dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
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
    n_ = n;
    ne_ = ne;
    if (live.fairness == LF_Process) KC_TRY(fair_sccs(n, res));

    // ---- counterexample
    if (res->violated) {
      uint32_t len = 0, kind = 0, loop = 0;
      if (live.fairness == LF_Process) {
        KC_TRY(fair_lasso(n, res, len, kind, loop));
      } else {
        KC_HIP_TRY(hipMemsetAsync(a_.stamp, 0, (size_t)n * sizeof(uint32_t), st_));
        hipLaunchKernelGGL(k_live_first, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
        KC_HIP_TRY(hipGetLastError());
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
    hipLaunchKernelGGL(k_live_first, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st_, a_, n);
    KC_HIP_TRY(hipGetLastError());
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
    for (uint32_t p = 0; p < (uint32_t)M::P; ++p)
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

  OwnedStream st_;   // (first: destroyed after every buffer below)
  LiveArgs a_{};     // the kernels' view of the buffers below
  DeviceArray<uint64_t> states_, d_trace_;
  DeviceArray<uint32_t> parent_, level_, edges_, stamp_, path_, color_, comp_, bpar_;
  DeviceArray<uint2> row_, sccw_;
  DeviceArray<LiveSlot> table_;
  DeviceArray<uint8_t> alive_, terminal_, eproc_, enabled_, fair_;
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

extern "C" {

int kc_live_create(const kc_model_config* cfg, const kc_live_config* live, kc_live** out) {
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
  if (!live_prop_ok(cfg->nc, live->property)) {
    set_error("kc_live_create: property %d is not defined for nc=%d (0-2 need one client; 3 any model)",
              live->property, cfg->nc);
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
  *out = new kc_live{std::move(impl)};
  return 0;
}

void kc_live_destroy(kc_live* l) { delete l; }

int kc_live_run(kc_live* l, kc_live_result* res) {
  if (!l || !res) { set_error("kc_live_run: NULL argument"); return -EINVAL; }
  return l->impl->run(res);
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
