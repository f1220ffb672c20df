// live_prog.h — k_live_mark_prog<W>: the mark step of the liveness checker for
// a user formula, the program-driven twin of k_live_mark<M>
// (liveness.hip).  liveness.hip (the product path) and the test-only
// live_mark_selftest.hip include it and launch the same kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "live_graph.h"
#include "pred.h"

namespace kc {

namespace {

// every W a model of KC_FOR_EACH_MODEL has is one of these
constexpr bool live_prog_width_ok(int W) { return W == 4 || W == 6 || W == 10; }

// One lane per graph state.  The program holds exactly two predicates, END 0 =
// P and END 1 = Q; pred_eval's bit k says predicate k is FALSE, so stay = ~Q is
// bit 1 and, for form 0 (P ~> Q), trig = P is bit 0 negated; for form 1 (<>Q)
// trig = an Init state.  The program pointer, its length and the form arrive
// in LiveArgs, a kernel argument, and the instruction index is the same in
// every lane: the instruction words come in with scalar loads and the opcode
// branches are uniform, as in k_pred.  A leaf reads its one word straight from
// a.states + i * W; no copy of the state is made.  The counters: one ballot,
// popcount and atomicAdd per wave each (live_wave_count).
template <int W>
__global__ void __launch_bounds__(LIVE_BLOCK) k_live_mark_prog(LiveArgs a, uint32_t n) {
  const uint32_t i = blockIdx.x * LIVE_BLOCK + threadIdx.x;
  bool stay = false, term = false, trig = false;
  if (i < n) {
    const uint32_t f = pred_eval(a.states + (uint64_t)i * W, PredProgram{a.prog, a.prog_n});
    stay = (f >> 1) & 1u;
    trig = a.form == 0 ? !(f & 1u) : a.level[i] == 1u;
    term = live_terminal_of(a, i);
    a.alive[i] = stay;
    a.terminal[i] = term;
    a.trig[i] = trig;
  }
  live_wave_count(stay, &a.ctr->stay);
  live_wave_count(stay && term, &a.ctr->stay_terminal);
  live_wave_count(stay && trig, &a.ctr->trig_stay);
}

// the launch, for the state widths the models have; false for any other W
inline bool live_mark_prog_launch(int W, const LiveArgs& a, uint32_t n, hipStream_t st) {
  const dim3 grid(live_grid(n)), block(LIVE_BLOCK);
  switch (W) {
    case 4: hipLaunchKernelGGL(k_live_mark_prog<4>, grid, block, 0, st, a, n); return true;
    case 6: hipLaunchKernelGGL(k_live_mark_prog<6>, grid, block, 0, st, a, n); return true;
    case 10: hipLaunchKernelGGL(k_live_mark_prog<10>, grid, block, 0, st, a, n); return true;
    default: return false;
  }
}

// A formula's program: valid for states of W words (pred_validate) with exactly
// two predicates.  nullptr, or what is wrong.
inline const char* live_formula_check(int form, const PredInstr* code, int n_instr, int W) {
  if (form != 0 && form != 1) return "form is 0 (P ~> Q) or 1 (<>Q)";
  const char* why = nullptr;
  const int k = pred_validate(code, n_instr, W, &why);
  if (k < 0) return why;
  if (k != 2) return "a formula's program has exactly two predicates: END 0 = P, END 1 = Q";
  return nullptr;
}

}  // namespace

}  // namespace kc
