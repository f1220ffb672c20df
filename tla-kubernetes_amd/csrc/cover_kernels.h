// cover_kernels.h — k_cover: the coverage base counters (cover.h) summed over
// the parents of one BFS level.
#pragma once
#include <hip/hip_runtime.h>

#include "cover.h"

namespace kc {

constexpr int COVER_THREADS = 256;
constexpr int COVER_PER_LANE = 8;     // states per lane: 2,048 per workgroup
constexpr int COVER_TILE = COVER_THREADS * COVER_PER_LANE;
// LDS copies of the vector, one per lane & 31: the lanes of a wave that add to
// the same counter (every lane adds to `states`, cov_api, ...) go to 32
// different banks instead of queueing on one address
constexpr int COVER_STRIPES = 32;
// one state adds less than 2^13 to a counter (|apiState|^2 <= 64^2), so a
// workgroup's 32-bit LDS sums stay below 2^24
static_assert((uint64_t)COVER_TILE * 64 * 64 < (1ull << 32), "k_cover: LDS sums are 32 bits");

// One lane per parent (COVER_PER_LANE strided parents per lane): the state
// comes in with 16-B loads, cover_visit runs on it in registers and adds its
// non-zero terms into its stripe of the workgroup's LDS vector (a state
// touches about a dozen of the counters); the workgroup then adds its non-zero
// sums into the 64-bit totals, at most KC_COVER_N global atomics per 2,048
// states.
template <class M>
__global__ void __launch_bounds__(COVER_THREADS)
k_cover(const typename M::State* __restrict__ cur, uint64_t n, Flags f, unsigned long long* __restrict__ sums) {
  __shared__ unsigned int sh[KC_COVER_N * COVER_STRIPES];
  for (int k = threadIdx.x; k < KC_COVER_N * COVER_STRIPES; k += COVER_THREADS) sh[k] = 0;
  __syncthreads();
  const int stripe = threadIdx.x & (COVER_STRIPES - 1);
  const uint64_t base = (uint64_t)blockIdx.x * COVER_TILE + threadIdx.x;
#pragma unroll 1
  for (int r = 0; r < COVER_PER_LANE; ++r) {
    const uint64_t i = base + (uint64_t)r * COVER_THREADS;
    if (i >= n) break;
    typename M::State s;
    const ulonglong2* v = reinterpret_cast<const ulonglong2*>(cur + i);
#pragma unroll
    for (int k = 0; k < M::W / 2; ++k) {
      const ulonglong2 q = v[k];
      s.w[2 * k] = q.x;
      s.w[2 * k + 1] = q.y;
    }
    cover_visit<M>(s, f, [&](int idx, uint32_t x) {
      if (x) atomicAdd(&sh[idx * COVER_STRIPES + stripe], x);
    });
  }
  __syncthreads();
  for (int k = threadIdx.x; k < KC_COVER_N; k += COVER_THREADS) {
    unsigned int x = 0;
#pragma unroll
    for (int j = 0; j < COVER_STRIPES; ++j) x += sh[k * COVER_STRIPES + ((j + k) & (COVER_STRIPES - 1))];
    if (x) atomicAdd(&sums[k], (unsigned long long)x);
  }
}

}  // namespace kc
