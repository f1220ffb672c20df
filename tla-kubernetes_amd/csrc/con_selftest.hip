// con_selftest.hip — test-only device harness for the constraint hook
// (kubeapi_spec.h ConModel::in_model): kc_con_selftest runs, one lane per
// (parent, successor, action) triple, the predicate the engine's kernels call
// after M::apply under cfg's constraint fields, so tests can hold the device
// code against the host's kc_spec_in_model element for element.  The host
// validates every tuple (bad input gets -EINVAL before a device is looked
// for) and packs it; the kernel reads 2 n states of M::W words and n slots
// and writes n ints.  Nothing of the product path calls this file.
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
k_con_in_model(const uint64_t* __restrict__ ps, const uint64_t* __restrict__ px, const int* __restrict__ slots,
               uint64_t n, Flags f, int* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename M::State s, x;
#pragma unroll
  for (int k = 0; k < M::W; ++k) {
    s.w[k] = ps[i * M::W + k];
    x.w[k] = px[i * M::W + k];
  }
  out[i] = M::in_model(s, x, slots[i], f);
}

template <class M>
int run_in_model(const kc_model_config& cfg, const uint64_t* ts, const uint64_t* tx, const int* actions, uint64_t n,
                 int* out) {
  std::vector<uint64_t> ps(n * M::W), px(n * M::W);
  std::vector<int> slots(n);
  for (uint64_t i = 0; i < n; ++i) {
    typename M::State s, x;
    if (!M::from_tuple(ts + i * M::TUPLE_WORDS, s) || !M::from_tuple(tx + i * M::TUPLE_WORDS, x)) {
      set_error("kc_con_selftest: pair %llu: tuple outside the lowered domain", (unsigned long long)i);
      return -EINVAL;
    }
    if (actions[i] < 0 || actions[i] >= A_COUNT) {
      set_error("kc_con_selftest: pair %llu: action %d outside 0..%d", (unsigned long long)i, actions[i], A_COUNT - 1);
      return -EINVAL;
    }
    for (int k = 0; k < M::W; ++k) {
      ps[i * M::W + k] = s.w[k];
      px[i * M::W + k] = x.w[k];
    }
    slots[i] = actions[i] == A_APIStart ? 2 * M::A : 0;   // (the hook tells an APIStart step by its slot)
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_con_selftest: no HIP device");
    return -ENODEV;
  }
  if (n == 0) return 0;
  DevBuf ds, dx, dsl, dout;
  KC_TRY(selftest::upload(ds, ps.data(), ps.size() * 8));
  KC_TRY(selftest::upload(dx, px.data(), px.size() * 8));
  KC_TRY(selftest::upload(dsl, slots.data(), slots.size() * sizeof(int)));
  KC_TRY(dout.alloc(n * sizeof(int)));
  hipLaunchKernelGGL(k_con_in_model<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     ds.as<const uint64_t>(), dx.as<const uint64_t>(), dsl.as<const int>(), n, flags_of(cfg),
                     dout.as<int>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace
}  // namespace kc

using namespace kc;

extern "C" int kc_con_selftest(const kc_model_config* cfg, const uint64_t* tuples_s, const uint64_t* tuples_x,
                               const int* actions, uint64_t n, int* out) {
  if (!cfg || (n && (!tuples_s || !tuples_x || !actions || !out))) { set_error("kc_con_selftest: NULL"); return -EINVAL; }
  if (cfg->action_constraints & ~AC_ALL) {
    set_error("kc_con_selftest: action_constraints %d outside 0..%d", cfg->action_constraints, AC_ALL);
    return -EINVAL;
  }
  if (n > (1ull << 24)) { set_error("kc_con_selftest: more than 2^24 pairs"); return -EINVAL; }
#define KC_CON(a, b, c) \
  if (cfg->nc == a && cfg->np == b && cfg->ns == c) return run_in_model<ConModel<a, b, c>>(*cfg, tuples_s, tuples_x, actions, n, out);
  KC_FOR_EACH_CON_MODEL(KC_CON)
#undef KC_CON
  set_error("kc_con_selftest: model nc=%d np=%d ns=%d is not built with constraints", cfg->nc, cfg->np, cfg->ns);
  return -EINVAL;
}
