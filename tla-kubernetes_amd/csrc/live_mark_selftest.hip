// live_mark_selftest.hip — test-only device harness for the two kernels of a
// user formula: kc_live_mark_selftest runs k_live_mark_prog<W>
// (live_prog.h) on made packed states and a made CSR graph, copies back the
// alive, terminal and trig bytes it wrote, then loads a given alive array and
// runs k_live_first_trig (live_graph.h) on it.  tests/test_gpu_live_mark.py
// compares the results with the instruction semantics of pred.h restated in
// Python.
//
// The data rules are live_selftest.hip's: everything travels as u64 words, one
// per element; every output section is uploaded as the caller filled it and
// copied back whole (KC_EMIT_FORE guard elements, the kernels' array, the
// caller's aft guards); every index a kernel derives from the input is checked
// on the host before any launch, so a machine without a GPU answers -EINVAL
// to bad input and -ENODEV only to good input.  Nothing of the product path
// calls this file.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "live_graph.h"
#include "live_prog.h"
#include "owned.h"
#include "selftest_util.h"

namespace kc {
namespace {

using selftest::DevBuf;
using selftest::upload;

constexpr uint64_t FORE = KC_EMIT_FORE;
constexpr uint64_t kMarkTestMaxStates = 1ull << 22;
constexpr uint64_t kMarkTestMaxAft = 1ull << 10;

int bad(const char* what) {
  set_error("kc_live_mark_selftest: %s", what);
  return -EINVAL;
}

// One output section of bytes on the device, filled from the caller's u64
// words and copied back into them.
struct ByteSection {
  DevBuf d;
  uint64_t len = 0;
  uint8_t* ptr() const { return d.as<uint8_t>() + FORE; }
  int up(const uint64_t* src, uint64_t n) {
    len = n;
    std::vector<uint8_t> h(n);
    for (uint64_t i = 0; i < n; ++i) h[i] = (uint8_t)src[i];
    return upload(d, h.data(), n);
  }
  int down(uint64_t* dst) const {
    std::vector<uint8_t> h(len);
    KC_HIP_TRY(hipMemcpy(h.data(), d.p, len, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < len; ++i) dst[i] = (uint64_t)h[i];
    return 0;
  }
};

}  // namespace
}  // namespace kc

extern "C" int kc_live_mark_selftest(const uint64_t* par, uint64_t npar, const uint64_t* program, int n_instr,
                                     const uint64_t* packed_states, const uint64_t* deg, const uint64_t* edges,
                                     uint64_t ne, const uint64_t* level, const uint64_t* alive_in, uint64_t* out,
                                     uint64_t nout, uint64_t* res, uint64_t nres) {
  using namespace kc;
  if (!par || npar != 4 || !program || !packed_states || !deg || !level || !alive_in || !out || !res || nres != 5 ||
      (ne && !edges))
    return bad("par of 4 words, program, packed_states, deg, edges, level, alive_in, out, and res of 5 words");
  const uint64_t W = par[0], form = par[1], n = par[2], aft = par[3];
  if (!(W == 4 || W == 6 || W == 10)) return bad("W is 4, 6 or 10 (the state widths the models have)");
  if (n == 0 || n > kMarkTestMaxStates || aft > kMarkTestMaxAft) return bad("1 to 2^22 states, up to 2^10 aft guards");
  const PredInstr* code = reinterpret_cast<const PredInstr*>(program);
  if (const char* why = live_formula_check(form > 1 ? -1 : (int)form, code, n_instr, (int)W)) return bad(why);
  if (ne >> 31) return bad("2^31 edges or more");
  std::vector<uint2> row(n);
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (deg[i] > ne || sum + deg[i] > ne) return bad("the out-degrees sum to more than ne");
    row[i] = make_uint2((uint32_t)sum, (uint32_t)deg[i]);
    sum += deg[i];
    if (alive_in[i] > 1) return bad("an alive_in word that is neither 0 nor 1");
    if (level[i] < 1 || level[i] > 0xffffffffull) return bad("a level outside 1 .. 2^32 - 1");
  }
  if (sum != ne) return bad("the out-degrees do not sum to ne");
  for (uint64_t e = 0; e < ne; ++e)
    if (edges[e] >= n) return bad("an edge's target is not a state");
  const uint64_t sec = FORE + n + aft;
  if (nout != 3 * sec) return bad("out holds three sections of fore + n + aft words");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {   // (the input is valid: -EINVAL needs no GPU)
    (void)hipGetLastError();
    set_error("kc_live_mark_selftest: no HIP device");
    return -ENODEV;
  }

  OwnedStream st;   // (first: destroyed after every buffer below)
  KC_TRY(st.create(hipStreamNonBlocking));
  DevBuf d_states, d_prog, d_level, d_row, d_edges, d_alive_in;
  DeviceArray<LiveCounters> ctr;
  PinnedArray<LiveCounters> h_ctr;
  ByteSection alive, terminal, trig;
  std::vector<uint32_t> h32(n);
  KC_TRY(upload(d_states, packed_states, n * W * 8));
  KC_TRY(upload(d_prog, code, (uint64_t)n_instr * sizeof(PredInstr)));
  for (uint64_t i = 0; i < n; ++i) h32[i] = (uint32_t)level[i];
  KC_TRY(upload(d_level, h32.data(), n * sizeof(uint32_t)));
  KC_TRY(upload(d_row, row.data(), n * sizeof(uint2)));
  h32.resize(ne);
  for (uint64_t e = 0; e < ne; ++e) h32[e] = (uint32_t)edges[e];
  KC_TRY(upload(d_edges, h32.data(), ne * sizeof(uint32_t)));
  std::vector<uint8_t> h8(n);
  for (uint64_t i = 0; i < n; ++i) h8[i] = (uint8_t)alive_in[i];
  KC_TRY(upload(d_alive_in, h8.data(), n));
  KC_TRY(alive.up(out, sec));
  KC_TRY(terminal.up(out + sec, sec));
  KC_TRY(trig.up(out + 2 * sec, sec));
  KC_TRY(ctr.alloc(1));
  KC_TRY(h_ctr.alloc(1));

  // LiveArgs as LiveT<M>::setup and set_formula fill it, what the two kernels do not read left out
  LiveArgs a;
  memset(&a, 0, sizeof a);
  a.max_states = n;
  a.max_edges = ne;
  a.states = d_states.as<uint64_t>();
  a.level = d_level.as<uint32_t>();
  a.row = d_row.as<uint2>();
  a.edges = d_edges.as<uint32_t>();
  a.alive = alive.ptr();
  a.terminal = terminal.ptr();
  a.trig = trig.ptr();
  a.prog = d_prog.as<PredInstr>();
  a.prog_n = n_instr;
  a.form = (int)form;
  a.ctr = ctr;
  LiveCounters zero;
  memset(&zero, 0, sizeof zero);
  zero.err_key = ~0ull;
  zero.first_alive = LIVE_NONE;
  zero.nstates = (unsigned)n;
  zero.nedges = ne;
  KC_HIP_TRY(hipMemcpyAsync(a.ctr, &zero, sizeof zero, hipMemcpyHostToDevice, st));

  if (!live_mark_prog_launch((int)W, a, (uint32_t)n, st)) return bad("no k_live_mark_prog for this W");
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipStreamSynchronize(st));
  KC_TRY(alive.down(out));
  KC_TRY(terminal.down(out + sec));
  KC_TRY(trig.down(out + 2 * sec));

  // the first-trigger step on the given alive bytes and the trig bytes as marked
  KC_HIP_TRY(hipMemcpyAsync(a.alive, d_alive_in.p, n, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_live_first_trig, dim3(live_grid(n)), dim3(LIVE_BLOCK), 0, st, a, (uint32_t)n);
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipMemcpyAsync(h_ctr, a.ctr, sizeof(LiveCounters), hipMemcpyDeviceToHost, st));
  KC_HIP_TRY(hipStreamSynchronize(st));
  res[0] = h_ctr->stay;
  res[1] = h_ctr->stay_terminal;
  res[2] = h_ctr->trig_stay;
  res[3] = h_ctr->first_alive;
  res[4] = h_ctr->trig_live;
  return 0;
}
