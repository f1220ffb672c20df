// pred.hip — user-defined invariants: k_pred for the state widths the models
// have, its launcher and result reset (the engine's translation units hold no
// predicate device code), and the host entry points kc_pred_eval and
// kc_pred_selftest.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "pred.h"
#include "pred_kernels.h"
#include "selftest_util.h"

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

// every W a model of KC_FOR_EACH_MODEL has is one of these
constexpr bool pred_width_ok(int W) { return W == 4 || W == 6 || W == 10; }
#define KC_PRED_CHECK_W(a, b, c) static_assert(pred_width_ok(Model<a, b, c>::W), "k_pred: no instantiation for this W");
KC_FOR_EACH_MODEL(KC_PRED_CHECK_W)
#undef KC_PRED_CHECK_W

template <int W>
void launch(const void* states, uint64_t n, uint64_t base, const PredInstr* d_prog, int n_instr,
            unsigned long long* d_out, hipStream_t st) {
  const unsigned grid = (unsigned)((n + PRED_TILE - 1) / PRED_TILE);
  hipLaunchKernelGGL(k_pred<W>, dim3(grid), dim3(PRED_THREADS), 0, st, static_cast<const uint64_t*>(states), n, base,
                     d_prog, n_instr, d_out);
}

}  // namespace

int pred_launch(int W, const void* states, uint64_t n, uint64_t base, const PredInstr* d_prog, int n_instr,
                unsigned long long* d_out, void* stream) {
  if (!n) return 0;
  if (n >= (1ull << 32) || base + n >= (1ull << 40)) {
    set_error("kubecheck: user invariants on a level wider than 2^32 states");
    return -ENOMEM;
  }
  if (n_instr < 1 || n_instr > KC_PRED_MAX_INSTR) {
    set_error("kubecheck: a predicate program has 1 to %d instructions", KC_PRED_MAX_INSTR);
    return -EINVAL;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (W) {
    case 4: launch<4>(states, n, base, d_prog, n_instr, d_out, st); break;
    case 6: launch<6>(states, n, base, d_prog, n_instr, d_out, st); break;
    case 10: launch<10>(states, n, base, d_prog, n_instr, d_out, st); break;
    default:
      set_error("kubecheck: no k_pred for states of %d words", W);
      return -EINVAL;
  }
  KC_HIP_TRY(hipGetLastError());
  return 0;
}

int pred_reset(unsigned long long* d_out, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  KC_HIP_TRY(hipMemsetAsync(d_out, 0xff, 8, st));
  KC_HIP_TRY(hipMemsetAsync(d_out + 1, 0, (PRED_OUT_WORDS - 1) * 8, st));
  return 0;
}

}  // namespace kc

using namespace kc;

extern "C" {

int kc_pred_eval(const kc_model_config* cfg, const uint64_t* program, int n_instr, const uint64_t* tuple) {
  if (!cfg || !program || !tuple) { set_error("kc_pred_eval: NULL"); return -EINVAL; }
  return with_model(cfg->nc, cfg->np, cfg->ns, [&](auto m) {
    using M = decltype(m);
    const PredInstr* code = reinterpret_cast<const PredInstr*>(program);
    const char* why = nullptr;
    if (pred_validate(code, n_instr, M::W, &why) < 0) {
      set_error("kc_pred_eval: bad program: %s", why);
      return -EINVAL;
    }
    typename M::State s;
    if (!M::from_tuple(tuple, s)) {
      set_error("kc_pred_eval: tuple outside the lowered domain");
      return -EINVAL;
    }
    return (int)pred_eval(s.w, PredProgram{code, n_instr});
  });
}

int kc_pred_selftest(int W, const uint64_t* program, int n_instr, const uint64_t* packed_states, uint64_t n_states,
                     uint64_t base, uint64_t* out, uint64_t nout) {
  constexpr uint64_t kMaxStates = 1ull << 22;
  if (!program || !packed_states || !out) { set_error("kc_pred_selftest: NULL"); return -EINVAL; }
  if (!pred_width_ok(W)) { set_error("kc_pred_selftest: W is 4, 6 or 10 (the state widths the models have)"); return -EINVAL; }
  if (n_states < 1 || n_states > kMaxStates) { set_error("kc_pred_selftest: 1 to 2^22 states"); return -EINVAL; }
  if (nout < KC_EMIT_FORE + PRED_OUT_WORDS) {
    set_error("kc_pred_selftest: out holds %d guard words, %d result words, then the caller's aft guards", KC_EMIT_FORE,
              PRED_OUT_WORDS);
    return -EINVAL;
  }
  const PredInstr* code = reinterpret_cast<const PredInstr*>(program);
  const char* why = nullptr;
  if (pred_validate(code, n_instr, W, &why) < 0) {
    set_error("kc_pred_selftest: bad program: %s", why);
    return -EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {   // (the input is valid: -EINVAL needs no GPU)
    (void)hipGetLastError();
    set_error("kc_pred_selftest: no HIP device");
    return -ENODEV;
  }
  OwnedStream st;   // (first: destroyed after every buffer below)
  KC_TRY(st.create(hipStreamNonBlocking));
  selftest::DevBuf d_states, d_prog, d_out;
  KC_TRY(selftest::upload(d_states, packed_states, n_states * W * 8));
  KC_TRY(selftest::upload(d_prog, code, (uint64_t)n_instr * sizeof(PredInstr)));
  KC_TRY(selftest::upload(d_out, out, nout * 8));
  unsigned long long* res = d_out.as<unsigned long long>() + KC_EMIT_FORE;
  KC_TRY(pred_reset(res, st));
  KC_TRY(pred_launch(W, d_states.p, n_states, base, d_prog.as<PredInstr>(), n_instr, res, st));
  KC_HIP_TRY(hipStreamSynchronize(st));
  KC_HIP_TRY(hipMemcpy(out, d_out.p, nout * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
