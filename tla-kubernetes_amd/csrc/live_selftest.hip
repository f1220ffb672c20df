// live_selftest.hip — test-only device harness for the graph part of the
// liveness checker (live_graph.h): kc_live_selftest takes a graph of the
// suite's making (CSR edges with a process each, the stay bits, the discovery
// order's parent and level), marks alive = stay and terminal through the
// helper k_live_mark<M> uses, and then runs LiveDriver::run, the call
// LiveT<M>::run makes after its build.  tests/test_gpu_live_graphs.py compares
// the results with tests/fair_model.py and tests/live_model.py.
//
// The data rules are emit_selftest.hip's: everything travels as u64 words, one
// per element; every output section is uploaded as the caller filled it and
// copied back whole (KC_EMIT_FORE guard elements, the kernels' array, the
// caller's aft guards); every index a kernel derives from the input is checked
// on the host before any launch, so a machine without a GPU answers -EINVAL
// to bad input and -ENODEV only to good input.  Nothing of the product path
// calls this file.
#include <hip/hip_runtime.h>

#include <chrono>
#include <vector>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "live_graph.h"
#include "owned.h"
#include "selftest_util.h"

namespace kc {
namespace {

using selftest::DevBuf;
using selftest::upload;

constexpr uint64_t FORE = KC_EMIT_FORE;
constexpr uint64_t kLiveTestMaxStates = 1ull << 22;
constexpr uint64_t kLiveTestMaxAft = 1ull << 10;
constexpr uint64_t kLiveTestMaxPath = 1ull << 26;

int bad(const char* what) {
  set_error("kc_live_selftest: %s", what);
  return -EINVAL;
}

// One output section of T on the device, filled from the caller's u64 words
// and copied back into them.
template <class T>
struct Section {
  DevBuf d;
  uint64_t len = 0;
  T* ptr() const { return d.as<T>() + FORE; }
  int up(const uint64_t* src, uint64_t n) {
    len = n;
    std::vector<T> h(n);
    for (uint64_t i = 0; i < n; ++i) h[i] = (T)src[i];
    return upload(d, h.data(), n * sizeof(T));
  }
  int down(uint64_t* dst) const {
    std::vector<T> h(len);
    KC_HIP_TRY(hipMemcpy(h.data(), d.p, len * sizeof(T), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < len; ++i) dst[i] = (uint64_t)h[i];
    return 0;
  }
};

template <class T>
int upload_as(DevBuf& d, const uint64_t* src, uint64_t n) {
  std::vector<T> h(n);
  for (uint64_t i = 0; i < n; ++i) h[i] = (T)src[i];
  return upload(d, h.data(), n * sizeof(T));
}

// alive = stay (given); terminal through k_live_mark<M>'s helper; the counters
// k_live_mark<M> keeps.
__global__ void __launch_bounds__(LIVE_BLOCK) k_selftest_mark(LiveArgs a, uint32_t n, const uint8_t* __restrict__ st) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool stay = false, term = false;
  if (i < n) {
    stay = st[i] != 0;
    term = live_terminal_of(a, i);
    a.alive[i] = stay;
    a.terminal[i] = term;
  }
  live_wave_count(stay, &a.ctr->stay);
  live_wave_count(stay && term, &a.ctr->stay_terminal);
}

}  // namespace
}  // namespace kc

extern "C" int kc_live_selftest(const uint64_t* par, uint64_t npar, const uint64_t* deg, const uint64_t* edges,
                                uint64_t ne, const uint64_t* eproc, const uint64_t* stay, const uint64_t* parent,
                                const uint64_t* level, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  using namespace kc;
  if (!par || npar != 5 || !deg || !stay || !parent || !level || !out || !res || nres != 16 || (ne && (!edges || !eproc)))
    return bad("par of 5 words, deg, edges, eproc, stay, parent, level, out, and res of 16 words");
  const uint64_t n = par[0], P = par[1], fairness = par[2], aft = par[4];
  if (n == 0 || n > kLiveTestMaxStates || P < 1 || P > 8 || fairness > 1 || aft > kLiveTestMaxAft)
    return bad("1 to 2^22 states, 1 to 8 processes, fairness 0 or 1, up to 2^10 aft guards");
  uint64_t path_cap = par[3];
  if (path_cap > kLiveTestMaxPath || (fairness == 0 && path_cap != 0 && path_cap < n))
    return bad("path_cap up to 2^26; under fairness 0 it is 0 or at least n (the walk is bounded by n)");
  if (path_cap == 0) path_cap = fairness ? n * (P + 3) : n;
  if (ne >> 31) return bad("2^31 edges or more");
  std::vector<uint2> row(n);
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (deg[i] > ne || sum + deg[i] > ne) return bad("the out-degrees sum to more than ne");
    row[i] = make_uint2((uint32_t)sum, (uint32_t)deg[i]);
    sum += deg[i];
    if (stay[i] > 1) return bad("a stay word that is neither 0 nor 1");
  }
  if (sum != ne) return bad("the out-degrees do not sum to ne");
  for (uint64_t e = 0; e < ne; ++e) {
    if (edges[e] >= n) return bad("an edge's target is not a state");
    if (eproc[e] >= P) return bad("an edge's process is not below P");
  }
  if (level[0] != 1) return bad("the first state's level is not 1");
  for (uint64_t i = 0; i < n; ++i) {
    if (i && level[i] < level[i - 1]) return bad("the levels fall along the index");
    if (level[i] == 1) {
      if (parent[i] != ~0ull) return bad("a level-1 state with a parent");
      continue;
    }
    const uint64_t p = parent[i];
    if (p >= i) return bad("a state's parent is not a smaller index");
    if (level[p] != level[i] - 1) return bad("a state's parent is not on the level before it");
    bool edge = false;
    for (uint32_t k = 0; k < row[p].y && !edge; ++k) edge = edges[row[p].x + k] == i;
    if (!edge) return bad("no edge from a state's parent to the state");
  }
  // six sections: alive, terminal, enabled, comp, fair of n elements, path of path_cap
  const uint64_t sec = FORE + n + aft, psec = FORE + path_cap + aft;
  if (nout != 5 * sec + psec) return bad("out holds five sections of fore + n + aft words and one of fore + path_cap + aft");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {   // (the input is valid: -EINVAL needs no GPU)
    (void)hipGetLastError();
    set_error("kc_live_selftest: no HIP device");
    return -ENODEV;
  }

  OwnedStream st;   // (first: destroyed after every buffer below)
  KC_TRY(st.create(hipStreamNonBlocking));
  DevBuf d_parent, d_level, d_row, d_edges, d_eproc, d_stay;
  DeviceArray<uint32_t> stamp, color, bpar;
  DeviceArray<uint2> sccw;
  DeviceArray<LiveCounters> ctr;
  PinnedArray<LiveCounters> h_ctr;
  Section<uint8_t> alive, terminal, enabled, fair;
  Section<uint32_t> comp, path;
  KC_TRY(upload_as<uint32_t>(d_parent, parent, n));   // (~0 becomes LIVE_NONE)
  KC_TRY(upload_as<uint32_t>(d_level, level, n));
  KC_TRY(upload(d_row, row.data(), n * sizeof(uint2)));
  KC_TRY(upload_as<uint32_t>(d_edges, edges, ne));
  KC_TRY(upload_as<uint8_t>(d_eproc, eproc, ne));
  KC_TRY(upload_as<uint8_t>(d_stay, stay, n));
  KC_TRY(alive.up(out, sec));
  KC_TRY(terminal.up(out + sec, sec));
  KC_TRY(enabled.up(out + 2 * sec, sec));
  KC_TRY(comp.up(out + 3 * sec, sec));
  KC_TRY(fair.up(out + 4 * sec, sec));
  KC_TRY(path.up(out + 5 * sec, psec));
  KC_TRY(stamp.alloc(n));
  KC_TRY(ctr.alloc(1));
  KC_TRY(h_ctr.alloc(1));

  // LiveArgs as LiveT<M>::setup fills it, the build's buffers left out
  LiveArgs a;
  memset(&a, 0, sizeof a);
  a.max_states = n;
  a.max_edges = ne;
  a.parent = d_parent.as<uint32_t>();
  a.level = d_level.as<uint32_t>();
  a.row = d_row.as<uint2>();
  a.edges = d_edges.as<uint32_t>();
  a.alive = alive.ptr();
  a.terminal = terminal.ptr();
  a.stamp = stamp;
  a.path = path.ptr();
  a.path_cap = path_cap;
  a.pmask = (1u << P) - 1u;
  a.ctr = ctr;
  if (fairness) {
    KC_TRY(color.alloc(n));
    KC_TRY(bpar.alloc(n));
    KC_TRY(sccw.alloc(n));
    a.eproc = d_eproc.as<uint8_t>();
    a.enabled = enabled.ptr();
    a.color = color;
    a.comp = comp.ptr();
    a.sccw = sccw;
    a.fair = fair.ptr();
    a.bpar = bpar;
  }
  LiveCounters zero;
  memset(&zero, 0, sizeof zero);
  zero.err_key = ~0ull;
  zero.first_alive = LIVE_NONE;
  zero.nstates = (unsigned)n;
  zero.nedges = ne;
  KC_HIP_TRY(hipMemcpyAsync(a.ctr, &zero, sizeof zero, hipMemcpyHostToDevice, st));
  memset(h_ctr.p, 0, sizeof(LiveCounters));

  const auto t1 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(k_selftest_mark, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st, a, (uint32_t)n,
                     d_stay.as<const uint8_t>());
  KC_HIP_TRY(hipGetLastError());
  kc_live_result r;
  memset(&r, 0, sizeof r);
  uint32_t len = 0, kind = 0, loop = 0;
  LiveDriver drv(a, st, h_ctr, (uint32_t)n, (int)P);
  const int rc = drv.run((int)fairness, t1, &r, len, kind, loop);
  KC_HIP_TRY(hipStreamSynchronize(st));
  if (rc != 0 && rc != -EIO) return rc;   // (-EIO: the driver's own verdict on the lasso, reported in res)

  KC_TRY(alive.down(out));
  KC_TRY(terminal.down(out + sec));
  KC_TRY(enabled.down(out + 2 * sec));
  KC_TRY(comp.down(out + 3 * sec));
  KC_TRY(fair.down(out + 4 * sec));
  KC_TRY(path.down(out + 5 * sec));
  const bool lasso = rc == 0 && r.violated;
  res[0] = r.stay_states;
  res[1] = h_ctr->stay_terminal;
  res[2] = h_ctr->removed;
  res[3] = r.rounds;
  res[4] = r.sccs;
  res[5] = r.fair_sccs;
  res[6] = r.fair_states;
  res[7] = r.live_states;
  res[8] = r.live_terminal;
  res[9] = r.scc_rounds;
  res[10] = (uint64_t)r.violated;
  res[11] = lasso ? kind : 0;
  res[12] = lasso ? h_ctr->lasso_prefix : 0;
  res[13] = lasso && kind == 1 ? loop : 0;
  res[14] = lasso ? len : 0;
  res[15] = ((uint64_t)h_ctr->lasso_err << 32) | (uint64_t)(uint32_t)(-rc);
  return 0;
}
