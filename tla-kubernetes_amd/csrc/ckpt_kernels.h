// ckpt_kernels.h — device side of checkpoint / recover:
// the seen-set's fingerprints out of the sparse table as a dense stream
// (k_ckpt_pack), the order-independent section checksum (k_ckpt_sum) and the
// count of restored fingerprints that were not new (k_ckpt_count_bad).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fpset_dev.h"

namespace kc {

constexpr int CKPT_THREADS = 256;
// accumulator words of one pack pass
enum CkptAcc : int { CA_COUNT = 0, CA_SUM = 1, CA_XOR = 2, CA_WORDS = 4 };

// 16-B units [u0, u1) of a ClaimSet -> its non-empty fingerprint words, dense
// in out[0 .. count).  A unit is one {fp, claim} slot, or (COMPACT) the two
// fp words of slots 2u and 2u + 1.  Per trip a workgroup takes CKPT_UNITS x
// 256 consecutive units: every lane issues CKPT_UNITS 16-B loads (each a
// coalesced row of the workgroup) and counts its non-empty words, a shuffle
// scan gives each lane its place in the wave, the four wave totals meet in
// LDS, and ONE atomicAdd on acc[CA_COUNT] reserves the workgroup's output
// range; then dense 8-B stores.  (One atomic per wave and 64 units, the first
// version, ran at the rate of same-address atomics: 35 ns each, 29 GB/s of
// table)  acc[CA_SUM], acc[CA_XOR]: the checksum of
// what was stored, folded once per wave at the end.  The host sizes a window
// (u1 - u0) so that even a full one fits out_cap; the bound is checked all
// the same.
constexpr int CKPT_UNITS = 8;
template <bool COMPACT>
__global__ void __launch_bounds__(CKPT_THREADS)
k_ckpt_pack(const ulonglong2* __restrict__ t, uint64_t nslots, uint64_t u0, uint64_t u1,
            unsigned long long* __restrict__ out, uint64_t out_cap, unsigned long long* __restrict__ acc) {
  static_assert(CKPT_THREADS == 256, "four waves per workgroup");
  __shared__ unsigned int sh_cnt[4];
  __shared__ unsigned long long sh_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr uint64_t PER_WG = (uint64_t)CKPT_THREADS * CKPT_UNITS;
  // every lane of the workgroup runs the same number of trips (barriers inside)
  const uint64_t per_trip = (uint64_t)gridDim.x * PER_WG;
  const uint64_t trips = (u1 - u0 + per_trip - 1) / per_trip;
  unsigned long long s = 0, x = 0;
  for (uint64_t k = 0; k < trips; ++k) {
    const uint64_t base_u = u0 + (k * gridDim.x + blockIdx.x) * PER_WG + threadIdx.x;
    unsigned long long a[CKPT_UNITS], b[CKPT_UNITS];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < CKPT_UNITS; ++j) {
      const uint64_t u = base_u + (uint64_t)j * CKPT_THREADS;
      a[j] = b[j] = 0;
      if (u < u1) {
        const ulonglong2 e = t[u];
        a[j] = e.x;
        if (COMPACT && 2 * u + 1 < nslots) b[j] = e.y;   // (an odd table's last unit holds one slot)
      }
      c += (a[j] != 0ull) + (b[j] != 0ull);
    }
    // the lane's place: an inclusive scan over the wave, then the waves before it
    unsigned incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    if (lane == 63) sh_cnt[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned tot = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
      sh_base = tot ? atomicAdd(&acc[CA_COUNT], (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    uint64_t pos = sh_base + (incl - c);
    for (int w = 0; w < wave; ++w) pos += sh_cnt[w];
#pragma unroll
    for (int j = 0; j < CKPT_UNITS; ++j) {
      if (a[j]) {
        if (pos < out_cap) out[pos] = a[j];
        ++pos;
        s += a[j];
        x ^= a[j];
      }
      if (COMPACT && b[j]) {
        if (pos < out_cap) out[pos] = b[j];
        ++pos;
        s += b[j];
        x ^= b[j];
      }
    }
    __syncthreads();                                     // (sh_cnt and sh_base are rewritten by the next trip)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    x ^= __shfl_down(x, off, 64);
  }
  if (lane == 0 && (s | x)) {
    atomicAdd(&acc[CA_SUM], s);
    atomicXor(&acc[CA_XOR], x);
  }
}

// (sum, xor) of p[0 .. n) added into acc[0], acc[1]; p is 16-B aligned
__global__ void __launch_bounds__(CKPT_THREADS)
k_ckpt_sum(const unsigned long long* __restrict__ p, uint64_t n, unsigned long long* __restrict__ acc) {
  const uint64_t pairs = n / 2, stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
  unsigned long long s = 0, x = 0;
  for (uint64_t i = g; i < pairs; i += stride) {
    const ulonglong2 e = q[i];
    s += e.x + e.y;
    x ^= e.x ^ e.y;
  }
  if (g == 0 && (n & 1)) {
    s += p[n - 1];
    x ^= p[n - 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    x ^= __shfl_down(x, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && (s | x)) {
    atomicAdd(&acc[0], s);
    atomicXor(&acc[1], x);
  }
}

// results of a list insert that are not CL_NEW, added into *bad
__global__ void __launch_bounds__(CKPT_THREADS)
k_ckpt_count_bad(const int* __restrict__ res, uint64_t n, unsigned long long* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long m = __ballot(i < n && res[i] != CL_NEW);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(bad, (unsigned long long)__popcll(m));
}

}  // namespace kc
