// pred_kernels.h — k_pred: a predicate program (pred.h) evaluated on every
// state of a resident frontier slice.
#pragma once
#include <hip/hip_runtime.h>

#include "pred.h"

namespace kc {

constexpr int PRED_THREADS = 256;
constexpr int PRED_PER_LANE = 4;      // states per lane: 1,024 per workgroup
constexpr int PRED_TILE = PRED_THREADS * PRED_PER_LANE;

// One lane per state (PRED_PER_LANE strided states per lane).  The program
// pointer and its length are kernel arguments and the instruction index is
// the same in every lane, so the instruction words come in with scalar loads
// and the opcode branches are uniform.  A leaf reads its one word straight
// from the frontier (the word index is uniform too, so the address is
// state base + a scalar offset): no copy of the state is made, and nothing
// is indexed at run time in registers or scratch.
//
// Results (pred.h PRED_OUT_WORDS): each wave adds its evaluated count once,
// its violation count per invariant once (ballot, popcount, lane 0 adds) and
// makes one atomicMin of its smallest (index << 8 | k).
template <int W>
__global__ void __launch_bounds__(PRED_THREADS)
k_pred(const uint64_t* __restrict__ states, uint64_t n, uint64_t base, const PredInstr* __restrict__ prog,
       int n_instr, unsigned long long* __restrict__ out) {
  const PredProgram p{prog, n_instr};
  const uint64_t first = (uint64_t)blockIdx.x * PRED_TILE + threadIdx.x;
  unsigned long long key = ~0ull;            // this lane's smallest
  unsigned int evaluated = 0;                // wave-uniform from here on
  unsigned int cnt[KC_PRED_MAX_INV];
#pragma unroll
  for (int k = 0; k < KC_PRED_MAX_INV; ++k) cnt[k] = 0;
#pragma unroll 1
  for (int r = 0; r < PRED_PER_LANE; ++r) {
    const uint64_t i = first + (uint64_t)r * PRED_THREADS;
    const bool valid = i < n;
    const unsigned long long live = __ballot(valid);
    if (!live) break;                        // (uniform: the wave's indices only grow)
    evaluated += (unsigned)__popcll(live);
    const uint32_t m = valid ? pred_eval(states + i * W, p) : 0u;
    if (!__ballot(m != 0)) continue;         // (uniform)
    if (m) {
      const unsigned long long mine = ((base + i) << 8) | (unsigned)(__ffs((int)m) - 1);
      key = mine < key ? mine : key;
    }
#pragma unroll
    for (int k = 0; k < KC_PRED_MAX_INV; ++k) cnt[k] += (unsigned)__popcll(__ballot((m >> k) & 1u));
  }
  // the wave's smallest key
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long other = __shfl_xor(key, d, 64);
    key = other < key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) {
    if (evaluated) atomicAdd(&out[1], (unsigned long long)evaluated);
    if (key != ~0ull) {
      atomicMin(&out[0], key);
#pragma unroll
      for (int k = 0; k < KC_PRED_MAX_INV; ++k)
        if (cnt[k]) atomicAdd(&out[2 + k], (unsigned long long)cnt[k]);
    }
  }
}

}  // namespace kc
