// cover.hip — expression-level coverage: k_cover instantiated for every plain
// Model the engine runs, its launcher (the engine's translation units hold no
// coverage device code), and the host entry points kc_spec_cover,
// kc_cover_count and kc_cover_name.
#include <hip/hip_runtime.h>

#include "../../include/kubecheck.h"
#include "cover.h"
#include "cover_kernels.h"
#include "engine.h"
#include "engine_util.h"
#include "kc_common.h"

namespace kc {

namespace {

template <class F>
int with_model(int nc, int np, int ns, F&& f) {
#define KC_DISPATCH(a, b, c) \
  if (nc == a && np == b && ns == c) return f(Model<a, b, c>{});
  KC_FOR_EACH_MODEL(KC_DISPATCH)
#undef KC_DISPATCH
  set_error("unsupported model nc=%d np=%d ns=%d", nc, np, ns);
  return -EINVAL;
}

}  // namespace

int cover_launch(const kc_model_config& cfg, const void* states, uint64_t n, unsigned long long* d_sums,
                 void* stream) {
  if (!n) return 0;
  if (n >= (1ull << 32)) {
    set_error("kubecheck: coverage of a level wider than 2^32 states");
    return -ENOMEM;
  }
  const Flags f = flags_of(cfg);
  return with_model(cfg.nc, cfg.np, cfg.ns, [&](auto m) {
    using M = decltype(m);
    const unsigned grid = (unsigned)((n + COVER_TILE - 1) / COVER_TILE);
    hipLaunchKernelGGL(k_cover<M>, dim3(grid), dim3(COVER_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const typename M::State*>(states), n, f, d_sums);
    KC_HIP_TRY(hipGetLastError());
    return 0;
  });
}

}  // namespace kc

using namespace kc;

extern "C" {

int kc_cover_count(void) { return KC_COVER_N; }

const char* kc_cover_name(int i) { return cover_name(i); }

int kc_spec_cover(const kc_model_config* cfg, const uint64_t* tuples, uint64_t n, uint64_t* sums_out) {
  if (!cfg || !sums_out || (n && !tuples)) { set_error("kc_spec_cover: NULL"); return -EINVAL; }
  return with_model(cfg->nc, cfg->np, cfg->ns, [&](auto m) {
    using M = decltype(m);
    const Flags f = flags_of(*cfg);
    for (int k = 0; k < KC_COVER_N; ++k) sums_out[k] = 0;
    for (uint64_t i = 0; i < n; ++i) {
      typename M::State s;
      if (!M::from_tuple(tuples + i * M::TUPLE_WORDS, s)) {
        set_error("kc_spec_cover: tuple %llu outside the lowered domain", (unsigned long long)i);
        return -EINVAL;
      }
      cover_visit<M>(s, f, [&](int k, uint32_t v) { sums_out[k] += v; });
    }
    return 0;
  });
}

}  // extern "C"
