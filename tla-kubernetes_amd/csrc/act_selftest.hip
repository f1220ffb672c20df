// act_selftest.hip — test-only device harness for the action-property hook
// (kubeapi_spec.h ActModel::step_violations): kc_act_selftest runs, one lane
// per (parent, successor, action) triple, the predicate the engine's kernels
// call after M::apply under cfg's action_properties, so tests can hold the
// device code against the host's kc_spec_step_violations element for
// element.  The host validates every tuple (bad input gets -EINVAL before a
// device is looked for) and packs it; the kernel reads 2 n states of M::W
// words and n slots and writes n masks.  Nothing of the product path calls
// this file.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/kubecheck.h"
#include "engine_util.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "selftest_util.h"

namespace kc {
namespace {

using selftest::DevBuf;

template <class M>
__global__ void __launch_bounds__(256)
k_act_step_violations(const uint64_t* __restrict__ ps, const uint64_t* __restrict__ px,
                      const int* __restrict__ slots, uint64_t n, Flags f, unsigned* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename M::State s, x;
#pragma unroll
  for (int k = 0; k < M::W; ++k) {
    s.w[k] = ps[i * M::W + k];
    x.w[k] = px[i * M::W + k];
  }
  out[i] = M::step_violations(s, x, slots[i], f);
}

template <class M>
int run_step_violations(const kc_model_config& cfg, const uint64_t* ts, const uint64_t* tx, const int* actions,
                        uint64_t n, unsigned* out) {
  std::vector<uint64_t> ps(n * M::W), px(n * M::W);
  std::vector<int> slots(n);
  for (uint64_t i = 0; i < n; ++i) {
    typename M::State s, x;
    if (!M::from_tuple(ts + i * M::TUPLE_WORDS, s) || !M::from_tuple(tx + i * M::TUPLE_WORDS, x)) {
      set_error("kc_act_selftest: pair %llu: tuple outside the lowered domain", (unsigned long long)i);
      return -EINVAL;
    }
    if (actions[i] < 0 || actions[i] >= A_COUNT) {
      set_error("kc_act_selftest: pair %llu: action %d outside 0..%d", (unsigned long long)i, actions[i], A_COUNT - 1);
      return -EINVAL;
    }
    for (int k = 0; k < M::W; ++k) {
      ps[i * M::W + k] = s.w[k];
      px[i * M::W + k] = x.w[k];
    }
    slots[i] = actions[i] == A_APIStart ? 2 * M::A : 0;   // (as kc_con_selftest; the properties read no slot)
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_act_selftest: no HIP device");
    return -ENODEV;
  }
  if (n == 0) return 0;
  DevBuf ds, dx, dsl, dout;
  KC_TRY(selftest::upload(ds, ps.data(), ps.size() * 8));
  KC_TRY(selftest::upload(dx, px.data(), px.size() * 8));
  KC_TRY(selftest::upload(dsl, slots.data(), slots.size() * sizeof(int)));
  KC_TRY(dout.alloc(n * sizeof(unsigned)));
  hipLaunchKernelGGL(k_act_step_violations<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     ds.as<const uint64_t>(), dx.as<const uint64_t>(), dsl.as<const int>(), n, flags_of(cfg),
                     dout.as<unsigned>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace
}  // namespace kc

using namespace kc;

extern "C" int kc_act_selftest(const kc_model_config* cfg, const uint64_t* tuples_s, const uint64_t* tuples_x,
                               const int* actions, uint64_t n, int* out_masks) {
  unsigned* const out = reinterpret_cast<unsigned*>(out_masks);
  if (!cfg || (n && (!tuples_s || !tuples_x || !actions || !out))) { set_error("kc_act_selftest: NULL"); return -EINVAL; }
  if (cfg->action_properties & ~AP_ALL) {
    set_error("kc_act_selftest: action_properties %d outside 0..%d", cfg->action_properties, AP_ALL);
    return -EINVAL;
  }
  if (n > (1ull << 24)) { set_error("kc_act_selftest: more than 2^24 pairs"); return -EINVAL; }
#define KC_ACT(a, b, c) \
  if (cfg->nc == a && cfg->np == b && cfg->ns == c) return run_step_violations<ActModel<a, b, c>>(*cfg, tuples_s, tuples_x, actions, n, out);
  KC_FOR_EACH_ACT_MODEL(KC_ACT)
#undef KC_ACT
  set_error("kc_act_selftest: model nc=%d np=%d ns=%d is not built with action properties", cfg->nc, cfg->np, cfg->ns);
  return -EINVAL;
}
