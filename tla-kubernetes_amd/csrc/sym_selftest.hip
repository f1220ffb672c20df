// sym_selftest.hip — test-only device harness for the symmetric fingerprint
// (kubeapi_spec.h fp_sym, SymModel): kc_sym_selftest_fps runs, one lane per
// state, the fingerprint function the engine's kernels call under
// cfg.symmetry, so tests can hold the device code against the host's
// kc_spec_fingerprint_sym element for element.  The host validates every
// tuple (bad input gets -EINVAL before a device is looked for) and packs it;
// the kernel reads n states of M::W words and writes n words.  Nothing of the
// product path calls this file.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "selftest_util.h"

namespace kc {
namespace {

using selftest::DevBuf;

template <class M>
__global__ void __launch_bounds__(256)
k_sym_fps(const uint64_t* __restrict__ packed, uint64_t n, unsigned long long* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename M::State s;
#pragma unroll
  for (int k = 0; k < M::W; ++k) s.w[k] = packed[i * M::W + k];
  out[i] = M::fingerprint(s);
}

template <class M>
int run_fps(const uint64_t* tuples, uint64_t n, uint64_t* fps) {
  std::vector<uint64_t> packed(n * M::W);
  for (uint64_t i = 0; i < n; ++i) {
    typename M::State s;
    if (!M::from_tuple(tuples + i * M::TUPLE_WORDS, s)) {
      set_error("kc_sym_selftest_fps: tuple %llu outside the lowered domain", (unsigned long long)i);
      return -EINVAL;
    }
    for (int k = 0; k < M::W; ++k) packed[i * M::W + k] = s.w[k];
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_sym_selftest_fps: no HIP device");
    return -ENODEV;
  }
  if (n == 0) return 0;
  DevBuf in, out;
  KC_TRY(selftest::upload(in, packed.data(), packed.size() * 8));
  KC_TRY(out.alloc(n * 8));
  hipLaunchKernelGGL(k_sym_fps<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     in.as<const uint64_t>(), n, out.as<unsigned long long>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(fps, out.p, n * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace
}  // namespace kc

using namespace kc;

extern "C" int kc_sym_selftest_fps(const kc_model_config* cfg, const uint64_t* tuples, uint64_t n, uint64_t* fps) {
  if (!cfg || (n && (!tuples || !fps))) { set_error("kc_sym_selftest_fps: NULL"); return -EINVAL; }
  if (cfg->symmetry & ~3) { set_error("kc_sym_selftest_fps: symmetry %d outside 0..3", cfg->symmetry); return -EINVAL; }
  if (n > (1ull << 24)) { set_error("kc_sym_selftest_fps: more than 2^24 states"); return -EINVAL; }
  const int eff = sym_effective(cfg->nc, cfg->np, cfg->symmetry);
#define KC_SYM(a, b, c, m) \
  if (cfg->nc == a && cfg->np == b && cfg->ns == c && eff == m) return run_fps<SymModel<a, b, c, m>>(tuples, n, fps);
  KC_FOR_EACH_SYM_MODEL(KC_SYM)
#undef KC_SYM
#define KC_PLAIN(a, b, c) \
  if (cfg->nc == a && cfg->np == b && cfg->ns == c && eff == 0) return run_fps<Model<a, b, c>>(tuples, n, fps);
  KC_FOR_EACH_MODEL(KC_PLAIN)
#undef KC_PLAIN
  set_error("kc_sym_selftest_fps: unsupported model nc=%d np=%d ns=%d symmetry=%d", cfg->nc, cfg->np, cfg->ns,
            cfg->symmetry);
  return -EINVAL;
}
