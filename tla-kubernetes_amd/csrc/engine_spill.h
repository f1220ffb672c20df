// engine_spill.h — kernels of the engine's seen-set spill mode
// (kc_model_config.seen_hbm_bytes > 0; coldset.h has the cold tier), and the
// tier's host side, SeenSpill, which the sharded stages share (at the end).
//
// The hot tier is the ClaimSet at a fixed size.  Per chunk of parents:
//   k_tile_succ     successors per 256-parent tile, so the host can cut the
//                   level into chunks whose insertions fit the hot table;
//   k_claim / k_settle_rec / k_tile_scan as in the default path: the
//                   chunk's winners w.r.t. the HOT tier (newmask bits);
//   k_spill_queries each winner's cold key and (parent, position), at its
//                   tile offset (same wave-balanced dealing as k_emit);
//   [sort by key; ColdSet::probe]
//   k_spill_apply   winners found in the cold tier lose: newmask bit and tile
//                   count cleared, and the hot slot re-tagged "level 0" so
//                   every later copy (this level's later chunks included)
//                   reads it as old without another cold probe;
//   k_tile_scan, k_emit as usual.
// A flush (k_claimset_keys, sort, ColdSet::add_run, clear) happens between
// chunks.  Chunks of one level are processed in parent order and claims grow
// with the parent index, so a flushed claim of an earlier chunk is always the
// winner over a later chunk's copy, which now finds it in the cold tier.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "coldset.h"
#include "engine_kernels.h"
#include "engine_util.h"
#include "fpset_dev.h"
#include "fpset_host.h"

namespace kc {

constexpr unsigned long long kClaimRetired = ~0ull;   // nclaim of a slot found in the cold tier (claim 0: level 0)

// successors per tile of 256 parents (plan totals, capped like k_claim)
template <class M>
__global__ void __launch_bounds__(256) k_tile_succ(const typename M::State* __restrict__ cur, uint64_t n, Flags f,
                                                   uint32_t* __restrict__ tsum) {
  __shared__ unsigned int sh[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned int c = 0;
  if (i < n) {
    const int t = M::plan(load_state<M>(cur, i), f).total;
    c = (unsigned)(t > M::MAXSUCC ? M::MAXSUCC : t);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tsum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// Every winner w.r.t. the hot tier -> (cold key, loc = parent-in-chunk << 5 | t),
// written at the chunk's exclusive tile offset plus the wave prefix.
template <class M>
__global__ void __launch_bounds__(256) k_spill_queries(const typename M::State* __restrict__ cur, uint64_t n, Flags f,
                                                       const uint32_t* __restrict__ newmask,
                                                       const uint32_t* __restrict__ tile_off,
                                                       uint64_t* __restrict__ qkey, uint32_t* __restrict__ qloc) {
  __shared__ unsigned int sh_wtot[4];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t mask = 0;
  uint64_t counts = 0;
  if (i < n) {
    mask = newmask[i];
    if (mask) counts = M::plan(load_state<M>(cur, i), f).counts;
  }
  const int cnt = __builtin_popcount(mask);
  const int lane = (int)(threadIdx.x & 63);
  int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const int wtot = __shfl(incl, 63, 64);
  const int excl = incl - cnt;
  if (lane == 0) sh_wtot[threadIdx.x >> 6] = (unsigned int)wtot;
  __syncthreads();
  uint32_t obase = tile_off[blockIdx.x];
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) obase += sh_wtot[w];
  const uint64_t wave0 = i - (uint64_t)lane;
  for (int r = 0; r < wtot; r += 64) {
    const int g = r + lane;
    int p = 0;                                       // last lane with excl <= g
#pragma unroll
    for (int b = 32; b > 0; b >>= 1) {
      const int e = __shfl(excl, p + b, 64);
      if (e <= g) p += b;
    }
    int k = g - __shfl(excl, p, 64);
    uint32_t m = (uint32_t)__shfl((int)mask, p, 64);
    const uint64_t pc = __shfl(counts, p, 64);
    if (g >= wtot) continue;
    for (; k > 0; --k) m &= m - 1;
    const int t = __ffs(m) - 1;
    const uint64_t pi = wave0 + (uint64_t)p;
    const typename M::State s = load_state<M>(cur, pi);
    const typename M::Plan pl{pc, 0, -1, -1};
    int slot, j;
    M::locate(pl, t, slot, j);
    typename M::State x;
    M::apply(s, slot, j, f, x);
    const uint64_t o = (uint64_t)obase + (uint64_t)g;
    qkey[o] = cold_key(M::fingerprint(x));
    qloc[o] = (uint32_t)(pi << 5) | (uint32_t)t;
  }
}

// Re-tag fp's hot slot "level 0" (a claim of ~0 reads as old from every
// later level) and as already in the cold tier (flushes skip it).  False if
// fp is not in the table, which the protocol never produces.
__device__ __forceinline__ bool claimset_retire(ClaimEntry* __restrict__ cs, uint64_t nslots, uint64_t fp) {
  uint64_t s = bucket_of(fp, nslots);
  for (uint64_t probe = 0; probe < nslots; ++probe) {
    const unsigned long long f = cs[s].fp;
    if (f == fp) {
      cs[s].nclaim = kClaimRetired;
      return true;
    }
    if (f == 0ull) break;
    s = (s + 1 == nslots) ? 0 : s + 1;
  }
  return false;
}

// Winners found in the cold tier lose (see the file comment).
static __global__ void k_spill_apply(const uint64_t* __restrict__ qkey, const uint32_t* __restrict__ qloc,
                              const uint8_t* __restrict__ found, uint64_t m, uint32_t* __restrict__ newmask,
                              uint32_t* __restrict__ tile_total, ClaimEntry* __restrict__ cs, uint64_t nslots,
                              Counters* __restrict__ C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !found[i]) return;
  const uint32_t loc = qloc[i];
  atomicAnd(&newmask[loc >> 5], ~(1u << (loc & 31)));
  atomicSub(&tile_total[loc >> 13], 1u);              // tile = parent / 256
  if (!claimset_retire(cs, nslots, cold_unkey(qkey[i])))
    atomicAdd(&C->overflow, 1ull);                    // a winner's fp is always in the hot table
}

// Flush: the cold key of every live hot slot (retired slots are already in
// the cold tier) into a dense array; *count = how many.
static __global__ void k_claimset_keys(const ClaimEntry* __restrict__ t, uint64_t nslots, uint64_t* __restrict__ out,
                                uint64_t cap, unsigned long long* __restrict__ count) {
  // (grid-stride; the bound is uniform per wave, so the ballot sees every lane)
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < nslots; i0 += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = i0 + threadIdx.x;
    bool live = false;
    uint64_t fp = 0;
    if (i < nslots) {
      const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(t + i);
      fp = e.x;
      live = fp != 0ull && e.y != kClaimRetired;
    }
    const unsigned long long b = __ballot(live);
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long base = 0;
    if (lane == 0 && b) base = atomicAdd(count, (unsigned long long)__popcll(b));
    base = __shfl(base, 0, 64);
    if (live) {
      const uint64_t k = base + (uint64_t)__popcll(b & ((1ull << lane) - 1));
      if (k < cap) out[k] = cold_key(fp);
    }
  }
}

// ---- The hot/cold seen-set tier's host side, shared by the engine and the
// sharded stages (kc_model_config.seen_hbm_bytes > 0).
// HBM budget B: the hot ClaimSet takes the largest power-of-two table of
// <= B/2 bytes and holds <= 1/2 load (hot_limit); one scratch arena serves
// the flush (the hot keys; the sort borrows the cleared-to-be table) and the
// cold check's queries (keys, locations, found flags, sort space; at most
// q_max at a time); the rest is the cold runs' directories and filters.
// What the two callers do differently is theirs (when to flush, how a level
// or chunk is checked) and comes in as values: Policy.  Loc is the type of a
// query's location (the engine's parent-in-chunk << 5 | t is 32 bits, the
// shard's 64); as a class template the tier brings its sort kernels only
// into the units that use it.
template <class Loc>
struct SeenSpill {
  struct Policy {
    uint64_t flush_cap = 0;     // most keys a flush may find in the hot table
    uint64_t q_max = 0;         // queries per cold check (a multiple of 256)
    const char* who = "";       // message prefix
    std::string dir;            // the disk tier's directory
  };
  struct Queries {
    uint64_t *qk, *qk2;
    Loc *ql, *ql2;
    uint8_t *found, *tmp;
  };

  DeviceArray<uint8_t> arena;                 // (cap = bytes)
  DeviceArray<unsigned long long> d_spctr;    // [0] cold hits, [1] flush count
  PinnedArray<unsigned long long> h_spctr;    // [2] is the caller's (its query count)
  size_t sp_qtmp_bytes = 0;
  ColdSet cold;
  uint64_t hot_limit = 0, q_max = 0;
  uint64_t flushes = 0, queries = 0;
  const char* who = "";

  // slots of the hot table for budget B
  static uint64_t hot_slots(uint64_t B) {
    // the hot table's share of the budget: 1/2 (round 4 A/B: 1/4 leaves room
    // for HBM copies of the newest cold runs but doubles the flushes,
    // 6.0-6.6 s against 4.7-5.3 s on NP=2 at 4 GiB)
    uint64_t ns = 1ull << 12;
    while (ns * 2 * sizeof(ClaimEntry) <= B / 2) ns *= 2;
    return ns;
  }

  // First run: the table, the arena and the cold tier; every run: all empty.
  int setup(const kc_model_config& cfg, DevClaimSet& cs, hipStream_t st, const Policy& pol) {
    if (!cs.t) {
      const uint64_t B = cfg.seen_hbm_bytes;
      const uint64_t ns = hot_slots(B);
      KC_TRY(cs.init(ns, st));
      hot_limit = ns / 2;
      q_max = pol.q_max;
      who = pol.who;
      size_t tmp = 0;
      {
        hipcub::DoubleBuffer<uint64_t> k(nullptr, nullptr);
        hipcub::DoubleBuffer<Loc> v(nullptr, nullptr);
        KC_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, k, v, (int)q_max, 0, 64, st));
      }
      sp_qtmp_bytes = tmp;
      const uint64_t qbytes = q_max * (8 + 8 + 2 * sizeof(Loc) + 1) + tmp + 1024;
      KC_TRY(arena.alloc(std::max<uint64_t>(pol.flush_cap * 8, qbytes)));
      KC_TRY(d_spctr.alloc(8));
      KC_TRY(h_spctr.alloc(8));
      const uint64_t used = ns * sizeof(ClaimEntry) + arena.cap;
      if (used + (1ull << 20) > B) {
        set_error("%s: seen_hbm_bytes %llu too small (hot table + scratch need %llu B)", who,
                  (unsigned long long)B, (unsigned long long)used);
        return -EINVAL;
      }
      ColdSet::Config cc;
      cc.device = cfg.device;
      cc.meta_hbm_bytes = B - used;
      cc.host_bytes = cfg.seen_host_bytes;
      cc.dir = pol.dir;
      if (const uint64_t wk = env_u64("KC_COLD_WINDOW")) cc.window_keys = wk;   // disk-run staging window (keys); tests shrink it
      if (const char* bb = getenv("KC_COLD_BLOOM_BITS")) cc.bloom_bits = atoi(bb);   // filter bits per key (0 = no filters; A/B)
      cc.cache_keys = env_flag("KC_COLD_CACHE", true);   // KC_COLD_CACHE=0: no HBM copies of run keys (A/B)
      KC_TRY(cold.init(cc));
    } else {
      KC_TRY(cs.clear(st));
    }
    cold.clear();
    flushes = queries = 0;
    KC_HIP_TRY(hipMemsetAsync(d_spctr, 0, 64, st));
    return 0;
  }

  // Hot table -> one sorted cold run; the table starts over empty (the
  // caller's count of its entries is the caller's to reset).
  int flush(DevClaimSet& cs, uint64_t cap, hipStream_t st) {
    uint64_t* keys = reinterpret_cast<uint64_t*>(arena.p);
    KC_HIP_TRY(hipMemsetAsync(d_spctr + 1, 0, 8, st));
    hipLaunchKernelGGL(k_claimset_keys, dim3(table_grid(cs.nslots)), dim3(256), 0, st, cs.t, cs.nslots, keys, cap,
                       d_spctr + 1);
    KC_HIP_TRY(hipMemcpyAsync(h_spctr, d_spctr, 16, hipMemcpyDeviceToHost, st));
    KC_HIP_TRY(hipStreamSynchronize(st));
    const uint64_t c = h_spctr[1];
    if (c > cap) {
      set_error("%s: hot seen-set holds %llu > %llu fingerprints", who, (unsigned long long)c,
                (unsigned long long)cap);
      return -EIO;
    }
    if (c) {
      // sort in place, borrowing the hot table (cleared right after) as the
      // alternate buffer and temporary storage
      uint64_t* alt = reinterpret_cast<uint64_t*>(cs.t.p);
      const uint64_t tab = cs.nslots * sizeof(ClaimEntry);
      const uint64_t off = (c * 8 + 255) / 256 * 256;
      hipcub::DoubleBuffer<uint64_t> kb(keys, alt);
      size_t tb = 0;
      KC_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, kb, (int)c, 0, 64, st));
      if (off + tb > tab) {
        set_error("%s: seen-set flush sort needs %llu B > %llu", who, (unsigned long long)(off + tb),
                  (unsigned long long)tab);
        return -ENOMEM;
      }
      KC_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(reinterpret_cast<uint8_t*>(cs.t.p) + off, tb, kb, (int)c, 0, 64, st));
      KC_TRY(cold.add_run(kb.Current(), c, st));
    }
    KC_TRY(cs.clear(st));
    ++flushes;
    return 0;
  }

  // the arena as a cold check uses it
  Queries carve() const {
    Queries q;
    q.qk = reinterpret_cast<uint64_t*>(arena.p);
    q.qk2 = q.qk + q_max;
    q.ql = reinterpret_cast<Loc*>(q.qk2 + q_max);
    q.ql2 = q.ql + q_max;
    q.found = reinterpret_cast<uint8_t*>(q.ql2 + q_max);
    q.tmp = q.found + (q_max + 255) / 256 * 256;
    return q;
  }
};

}  // namespace kc
