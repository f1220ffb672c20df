// shard_kernels.h — the device code of the sharded BFS level (shard.hip
// launches it): the send-buffer pack and gather, the owner-major
// scans and the all-gather row, the received records' claims and settle
// passes, the winners' scans, both emits, the deferred frontier's
// materialisation, the seen-set spill's query kernels, the TLC-order
// renumbering and the undo of a level's generated counts.  A header so that
// the test harness (shard_selftest.hip) instantiates the same text; the
// anonymous namespace gives each translation unit its own copy of the
// kernels that are no templates.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/kubecheck.h"
#include "coldset.h"
#include "engine_kernels.h"
#include "engine_spill.h"
#include "engine_util.h"
#include "kc_common.h"
#include "record.h"

namespace kc {
namespace {

template <class M>
__device__ __forceinline__ uint64_t record_key(const Record<M>* __restrict__ in, uint64_t i) {
  return in[i].w[0];
}


template <class M>
__global__ void __launch_bounds__(256)
k_shard_pack(const typename M::State* __restrict__ cur, uint64_t n, Flags f, uint32_t world,
             uint64_t rank, const uint32_t* __restrict__ off /* [world][n], one exclusive scan */,
             const uint32_t* __restrict__ repmask,
             Record<M>* __restrict__ out, const uint32_t* __restrict__ gpos /* TLC order: G per parent */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t mask = repmask[i];
  if (!mask) return;
  const typename M::State s = load_state<M>(cur, i);
  const typename M::Plan pl = M::plan(s, f);
  const uint64_t fold = M::fp_fold(s);
  uint32_t c[16] = {};
  for (; mask; mask &= mask - 1) {
    const int t = __ffs(mask) - 1;
    int slot, j;
    M::locate(pl, t, slot, j);
    typename M::State x;
    int who;
    M::apply(s, slot, j, f, x, who);
    const uint64_t fp = M::template fingerprint_succ<1>(s, fold, x, who, M::owner_proj(s));
    const uint32_t o = owner_of(fp, world);
    uint32_t r = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
      if (k == o) { r = c[k]; c[k] = r + 1; }
    const uint64_t pos = (uint64_t)off[(uint64_t)o * n + i] + r;   // owner-major scan
    uint64_t w[Record<M>::RW];
    record_pack<M>(x, (rank << 60) | ((gpos ? (uint64_t)gpos[i] : i) << 16) | ((uint64_t)t << 8) |
                          (uint64_t)M::slot_action(s, slot), w);
    ulonglong2* v = reinterpret_cast<ulonglong2*>(out + pos);
#pragma unroll
    for (int k = 0; k < Record<M>::RW / 2; ++k) v[k] = make_ulonglong2(w[2 * k], w[2 * k + 1]);
  }
}

// Records per owner from the owner-major exclusive scan of cnt[world][n]
// (8-bit counts: a parent has at most 32 successors).
// Owner totals (world > 1; 0 at world 1) into tot and straight into pinned
// host memory, with the level head (error key, overflow flags): what the
// host reads after expand, with no copy launches.
// (device-scope loads: the last emit workgroup reads what the others' atomics wrote)
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void head_to_host(const Counters* __restrict__ C, unsigned long long* __restrict__ h) {
  h[0] = ld_agent(&C->err_key);
  h[1] = ld_agent(&C->chunk_base);
  h[2] = ld_agent(&C->overflow);
  h[3] = ld_agent(&C->batch_used);
  h[4] = ld_agent(&C->cand_total);
  h[5] = ld_agent(&C->level_new);
  h[7] = ld_agent(&C->defer_flags);
  h[9] = ld_agent(&C->defer_err);
}
// Level head reset at the start of expand (one launch instead of fills),
// with the candidate overflow list's count and the staging cursor.
__global__ void k_head_reset(Counters* __restrict__ C, unsigned long long* __restrict__ ovf_count,
                             unsigned long long* __restrict__ stage_cur) {
  if (threadIdx.x == 0) {
    C->err_key = ~0ull;
    C->chunk_base = 0;
    C->overflow = 0;
    C->batch_used = 0;
    C->emit_done = 0;
    C->defer_flags = 0;
    C->defer_err = ~0ull;
    *ovf_count = 0;
    *stage_cur = 0;
  }
}
// row != nullptr (ShardBase::expand_dev): the all-gather row too, in device
// memory: totals, status_new, status_err (level 1: an Init-state invariant
// key, 0x12, found by expand takes the status slot, as Group::run does), and
// the failure word.
// (thread o < 16: owner o's total v; thread 0 also the head and the status
// words.  status_err takes the deferred frontier's invariant key, an error
// of the level before, as the materialising emit would have reported it.)
__device__ __forceinline__ void owner_row(uint32_t o, uint64_t v, uint32_t world, uint64_t* __restrict__ tot,
                                          const Counters* __restrict__ C, uint64_t* __restrict__ host_tot,
                                          unsigned long long* __restrict__ host_head, uint64_t* __restrict__ row,
                                          uint64_t status_new, uint64_t status_err, int level1, uint64_t init_err) {
  if (o == 0) {
    head_to_host(C, host_head);
    if (row) {
      uint64_t se = status_err;
      const uint64_t de = C->defer_err;
      if (de < se) se = de;
      // an Init state's invariant violation is level 1's error, whatever
      // level 1's expansion found (an Assert of a lower-index Init state
      // must not hide it)
      if (level1 && init_err != ~0ull) se = init_err;
      row[world] = status_new;
      row[world + 1] = se;
      // failure word: a full table or an over-wide state found by this
      // level's claims, so every rank leaves the loop together (the host
      // overwrites it with its own failure code, if any)
      row[world + 2] = (C->overflow || C->batch_used) ? 1ull : 0ull;
    }
  }
  if (o >= 16) return;
  tot[o] = v;
  host_tot[o] = v;
  if (row && o < world) row[o] = v;
}
__device__ __forceinline__ void owner_totals(const uint32_t* __restrict__ off, const uint8_t* __restrict__ cnt,
                                             uint64_t n, uint32_t world, uint64_t* __restrict__ tot,
                                             const Counters* __restrict__ C, uint64_t* __restrict__ host_tot,
                                             unsigned long long* __restrict__ host_head, uint64_t* __restrict__ row,
                                             uint64_t status_new, uint64_t status_err, int level1,
                                             uint64_t init_err) {
  const uint32_t o = threadIdx.x;
  uint64_t v = 0;
  if (world > 1 && o < world && n > 0) {
    const uint64_t end = (o + 1 < world) ? (uint64_t)off[(uint64_t)(o + 1) * n]
                                         : (uint64_t)off[(uint64_t)world * n - 1] + cnt[(uint64_t)world * n - 1];
    v = end - off[(uint64_t)o * n];
  }
  owner_row(o, v, world, tot, C, host_tot, host_head, row, status_new, status_err, level1, init_err);
}
__global__ void k_owner_totals(const uint32_t* __restrict__ off, const uint8_t* __restrict__ cnt,
                               uint64_t n, uint32_t world, uint64_t* __restrict__ tot,
                               const Counters* __restrict__ C, uint64_t* __restrict__ host_tot,
                               unsigned long long* __restrict__ host_head, uint64_t* __restrict__ row,
                               uint64_t status_new, uint64_t status_err, int level1, uint64_t init_err) {
  owner_totals(off, cnt, n, world, tot, C, host_tot, host_head, row, status_new, status_err, level1, init_err);
}

// Owner-major exclusive scan of the tiles' per-owner record counts (k_claim
// with staging: tcnt[o][tile], world x T cells) -> toff, the send-buffer
// position of each (owner, tile) segment; the owner totals then go to the
// all-gather row and the host as in owner_totals.  One workgroup (the
// engine's k_tile_scan body), instead of a device scan over world x n
// per-parent cells and a totals launch.
__global__ void __launch_bounds__(TSCAN_THREADS)
k_owner_tscan(const uint32_t* __restrict__ tcnt, uint32_t T, uint32_t world, uint32_t* __restrict__ toff,
              uint64_t* __restrict__ tot, const Counters* __restrict__ C, uint64_t* __restrict__ host_tot,
              unsigned long long* __restrict__ host_head, uint64_t* __restrict__ row, uint64_t status_new,
              uint64_t status_err, int level1, uint64_t init_err) {
  __shared__ unsigned int sh_mark[17];
  const uint32_t cells = world * T;
  tile_scan_body(tcnt, cells, toff, 1, ScanMarks{T, world, cells}, sh_mark);
  if (threadIdx.x < 64) {
    const uint32_t o = threadIdx.x;
    const uint64_t v = o < world ? (uint64_t)(sh_mark[o + 1 < world ? o + 1 : world] - sh_mark[o]) : 0ull;
    owner_row(o, world > 1 ? v : 0ull, world, tot, C, host_tot, host_head, row, status_new, status_err, level1,
              init_err);
  }
}
// The same over the owner x chunk sums (round 6, ShardArgs::ocsum): world x
// C cells (C = ceil(T / CSUM_TILES)) instead of world x T; coff[o][chunk] is
// the send-buffer position of the chunk's first record of owner o, and the
// sums are zeroed for the next level.  k_shard_gather adds a tile's offset
// inside its chunk.
__global__ void __launch_bounds__(TSCAN_THREADS)
k_owner_cscan(uint32_t* __restrict__ ocsum, uint32_t C_, uint32_t world, uint32_t* __restrict__ coff,
              uint64_t* __restrict__ tot, const Counters* __restrict__ C, uint64_t* __restrict__ host_tot,
              unsigned long long* __restrict__ host_head, uint64_t* __restrict__ row, uint64_t status_new,
              uint64_t status_err, int level1, uint64_t init_err) {
  __shared__ unsigned int sh_mark[17];
  const uint32_t cells = world * C_;
  tile_scan_body(ocsum, cells, coff, 1, ScanMarks{C_, world, cells}, sh_mark);
  for (uint32_t c = threadIdx.x; c < cells; c += TSCAN_THREADS) ocsum[c] = 0u;
  if (threadIdx.x < 64) {
    const uint32_t o = threadIdx.x;
    const uint64_t v = o < world ? (uint64_t)(sh_mark[o + 1 < world ? o + 1 : world] - sh_mark[o]) : 0ull;
    owner_row(o, world > 1 ? v : 0ull, world, tot, C, host_tot, host_head, row, status_new, status_err, level1,
              init_err);
  }
}
// The staged records into the send buffer (pack without re-expansion): one
// workgroup per tile moves its segment, owner by owner, to toff[o][tile]
// (chunked: coff[o][chunk] + the tile counts of owner o before it in its
// chunk, one wave prefix per owner).
template <class M>
__global__ void __launch_bounds__(256)
k_shard_gather(const Record<M>* __restrict__ stage, const unsigned long long* __restrict__ stoff,
               const uint32_t* __restrict__ tcnt, const uint32_t* __restrict__ toff, uint32_t T, uint32_t world,
               Record<M>* __restrict__ out, int chunked) {
  constexpr int U = Record<M>::RW / 2;     // 16-B units per record
  __shared__ uint32_t sh_n[16], sh_src[16], sh_dst[16];
  const uint32_t tile = blockIdx.x;
  const unsigned long long b = stoff[tile];      // (loaded with the counts: one round trip less)
  if (!chunked) {
    if (threadIdx.x == 0) {
      uint32_t acc = 0;
      for (uint32_t o = 0; o < world; ++o) {
        const uint32_t c = tcnt[(uint64_t)o * T + tile];
        sh_n[o] = c;
        sh_src[o] = acc;
        sh_dst[o] = toff[(uint64_t)o * T + tile];
        acc += c;
      }
    }
  } else if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x, c0 = tile / CSUM_TILES * CSUM_TILES, j = tile - c0;
    const uint32_t nC = (T + CSUM_TILES - 1) / CSUM_TILES;
    uint32_t v[16], base[16];
#pragma unroll
    for (uint32_t o = 0; o < 16; ++o) {          // (world <= 15) every owner's counts and chunk base at once
      v[o] = o < world && c0 + lane < T ? tcnt[(uint64_t)o * T + c0 + lane] : 0u;
      base[o] = o < world ? toff[(uint64_t)o * nC + tile / CSUM_TILES] : 0u;
    }
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t o = 0; o < 16; ++o) {
      if (o >= world) break;
      uint32_t x = v[o];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, off, 64);
        if (lane >= (uint32_t)off) x += y;
      }
      if (lane == j) {
        sh_n[o] = v[o];
        sh_src[o] = acc;
        sh_dst[o] = base[o] + x - v[o];
      }
      acc += (uint32_t)__shfl((int)v[o], (int)j, 64);
    }
  }
  __syncthreads();
  if (b == ~0ull) return;
  const ulonglong2* src = reinterpret_cast<const ulonglong2*>(stage + b);
  ulonglong2* dst = reinterpret_cast<ulonglong2*>(out);
  for (uint32_t o = 0; o < world; ++o) {
    const uint32_t units = sh_n[o] * U;
    const ulonglong2* s = src + (uint64_t)sh_src[o] * U;
    ulonglong2* d = dst + (uint64_t)sh_dst[o] * U;
    for (uint32_t u = threadIdx.x; u < units; u += blockDim.x) d[u] = s[u];
  }
}

// 8-bit per-owner counts widened for the owner-major scan
struct Widen8 {
  __host__ __device__ __forceinline__ uint32_t operator()(uint8_t v) const { return v; }
};

// Record flags: 0 = out, 1 = candidate, 2 = inserted its fp, 3 = displacer.
enum : unsigned int { RF_OUT = 0, RF_CAND = 1, RF_INSERTER = 2, RF_DISPLACER = 3 };

template <class M>
__global__ void __launch_bounds__(256)
k_rec_claim(const Record<M>* __restrict__ in, uint64_t n, ClaimEntry* __restrict__ cs,
            uint64_t nslots, uint32_t level, unsigned long long* __restrict__ rfp,
            unsigned int* __restrict__ flag, Counters* __restrict__ C, int tlc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long probes = 0;
  if (i < n) {
    typename M::State x;
    uint64_t key;
    load_record<M>(in, i, x, key);
    const uint64_t fp = M::template fingerprint<1>(x);
    rfp[i] = fp;
    const int r = claimset_claim_store(cs, nslots, fp, make_claim(level, record_ckey(key, tlc)), level);
    if (r == CL_FULL) atomicAdd(&C->overflow, 1ull);
    flag[i] = r == CL_NEW ? RF_INSERTER : (r == CL_CUR ? RF_CAND : RF_OUT);
    probes = 1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) probes += __shfl_down(probes, off, 64);
  if ((threadIdx.x & 63) == 0 && probes) atomicAdd(&stripe(C).probes, probes);
}

// First-claim mode (cfg.first_claim; ShardT::first_): a received record is
// new iff its CAS inserts the fingerprint — no claim word, no candidates, no
// settle passes (a copy this rank's own k_claim inserted at expand, or an
// earlier record's, makes it old).  isnew[i] directly, and each block's
// winners into rtot[blk] (the record half of k_win_scan's input).
// (Two records per lane, their loads, probes and CASes issued together,
// measured slower at R = 8: Σ over the ranks 23.3 -> 26.5 ms, r06z — half
// the workgroups on the small levels.)
template <class M>
__global__ void __launch_bounds__(256)
k_rec_claim_first(const Record<M>* __restrict__ in, uint64_t n, ClaimEntry* __restrict__ cs, uint64_t nslots,
                  uint32_t* __restrict__ isnew, uint32_t* __restrict__ rtot, Counters* __restrict__ C,
                  int compact) {
  __shared__ unsigned int sh_rw[4];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t w = 0;
  if (i < n) {
    typename M::State x;
    uint64_t key;
    load_record<M>(in, i, x, key);
    const uint64_t fp = M::template fingerprint<1>(x);
    unsigned long long* const w8 = reinterpret_cast<unsigned long long*>(cs);
    const uint64_t b = compact ? fpslots_home(fp, nslots) : bucket_of(fp, nslots);
    const int r = compact ? fpslots_insert_pair(w8, nslots, fp, b, fpslots_first(w8, b))
                          : claimset_insert_from(cs, nslots, fp, b, cs[b].fp);
    if (r == CL_FULL) atomicAdd(&C->overflow, 1ull);
    w = r == CL_NEW ? 1u : 0u;
    isnew[i] = w;
  }
  const unsigned long long bw = __ballot(w != 0);
  const unsigned long long bp = __ballot(i < n);
  if ((threadIdx.x & 63) == 0) {
    sh_rw[threadIdx.x >> 6] = (unsigned)__popcll(bw);
    if (bp) atomicAdd(&stripe(C).probes, (unsigned long long)__popcll(bp));
  }
  __syncthreads();
  if (threadIdx.x == 0) rtot[blockIdx.x] = sh_rw[0] + sh_rw[1] + sh_rw[2] + sh_rw[3];
}

// PASS 0: candidates fold their claims (a displaced local claim loses its
// newmask bit, the displacer is flagged); PASS 1: inserters and displacers
// win iff the stored claim is still theirs.
// PASS 1 with rtot: the block's winners (the record half of k_win_scan's input).
template <class M, int PASS>
__device__ __forceinline__ void rec_settle(uint64_t blk, const Record<M>* __restrict__ in, uint64_t n,
                                           ClaimEntry* __restrict__ cs, uint64_t nslots, uint32_t level,
                                           const ClaimKeys& rank, const unsigned long long* __restrict__ rfp,
                                           unsigned int* __restrict__ flag, uint32_t* __restrict__ newmask,
                                           uint64_t nlocal, uint32_t* __restrict__ isnew, Counters* __restrict__ C,
                                           uint32_t* __restrict__ rtot) {
  const uint64_t i = blk * 256 + threadIdx.x;
  if (PASS == 0) {
    if (i >= n) return;
    const unsigned int fl = flag[i];
    if (fl != RF_CAND) return;
    const uint64_t claim = make_claim(level, record_ckey(record_key<M>(in, i), rank.gpos != nullptr));
    const unsigned long long prev = claimset_store_claim(cs, nslots, rfp[i], claim);
    if (prev < ~claim) settle_displace(prev, level, rank, 0, nlocal, newmask, C, &flag[i], RF_DISPLACER);
  } else {
    uint32_t w = 0;
    if (i < n) {
      const unsigned int fl = flag[i];
      if (fl >= RF_INSERTER) {
        const uint64_t claim = make_claim(level, record_ckey(record_key<M>(in, i), rank.gpos != nullptr));
        w = ~claimset_get(cs, nslots, rfp[i]) == claim ? 1u : 0u;
      }
      isnew[i] = w;
    }
    if (rtot) {
      __shared__ unsigned int sh_rw[4];
      const unsigned long long b = __ballot(w != 0);
      if ((threadIdx.x & 63) == 0) sh_rw[threadIdx.x >> 6] = (unsigned)__popcll(b);
      __syncthreads();
      if (threadIdx.x == 0) rtot[blk] = sh_rw[0] + sh_rw[1] + sh_rw[2] + sh_rw[3];
    }
  }
}
// One settle pass over this rank's own claim tiles (blocks [0, tiles)), the
// received records (the next rblocks) and the tiles' candidate overflow list
// (the blocks after those), in one launch: the passes of the three commute
// (atomicMax claims; a displaced candidate has no bit; with no per-tile
// counts here, overflow winners set their bits like tile winners).  Pass A
// also resets the level's error key for the emits.
// wtot != nullptr (PASS 1, the tile-count path): the own tiles' new-state
// counts go to wtot[0, tiles) and the record blocks' winners to
// wtot[tiles, tiles + rblocks) — k_win_scan's input — and the launch has no
// overflow-list blocks: their pass B adds to the tile counts afterwards
// (k_settle_ovf<1>), as the engine's does, so no winner is counted twice.
template <class M, int PASS>
__global__ void __launch_bounds__(256)
k_settle_both(uint32_t tiles, uint32_t rblocks, uint64_t n_local, ClaimEntry* __restrict__ cs, uint64_t nslots,
              uint32_t level, ClaimKeys rank, const unsigned int* __restrict__ rcount,
              const unsigned long long* __restrict__ rec_fp, unsigned int* __restrict__ rec_lk,
              uint32_t* __restrict__ newmask, const Record<M>* __restrict__ in, uint64_t n,
              const unsigned long long* __restrict__ rfp, unsigned int* __restrict__ flag,
              uint32_t* __restrict__ isnew, Counters* __restrict__ C, CandOvf ovf, uint32_t* __restrict__ wtot) {
  static_assert(CLAIM_TILE == 256, "one block size for both halves");
  if (PASS == 0 && blockIdx.x == 0 && threadIdx.x == 0) C->err_key = ~0ull;   // (nothing before the emits sets it)
  const uint32_t tb = tiles;
  if (blockIdx.x < tb) {
    settle_tile<PASS>(blockIdx.x, n_local, 0, cs, nslots, level, rcount, rec_fp, rec_lk, newmask, C, rank,
                      PASS == 1 ? wtot : nullptr);
  } else if (blockIdx.x < tb + rblocks) {
    rec_settle<M, PASS>(blockIdx.x - tb, in, n, cs, nslots, level, rank, rfp, flag, newmask, n_local, isnew, C,
                        PASS == 1 && wtot ? wtot + tiles : nullptr);
  } else {
    settle_ovf_blocks<PASS>(blockIdx.x - tb - rblocks, gridDim.x - tb - rblocks, ovf, n_local, 0, cs, nslots,
                            level, newmask, C, rank, nullptr);
  }
}
// Positions of the level's new states (the tile-count path): one scan over
// [own tiles' counts | record blocks' winners] -> woff; chunk_base = this
// rank's own new states (the records' emit base), level_new = all.
__global__ void __launch_bounds__(TSCAN_THREADS)
// (it also resets the level's error key for the emits — expand's Assert /
// deadlock keys were read from its own head copy; in the deterministic mode
// settle pass A did this already, first-claim mode runs no settle pass)
k_win_scan(const uint32_t* __restrict__ wtot, uint32_t tiles, uint32_t rblocks, uint32_t* __restrict__ woff,
           Counters* __restrict__ C) {
  __shared__ unsigned int sh_mark[4];
  const uint32_t cells = tiles + rblocks;
  tile_scan_body(wtot, cells, woff, 1, ScanMarks{cells, 2, tiles}, sh_mark);
  if (threadIdx.x == 0) {
    C->chunk_base = sh_mark[2];
    C->level_new = sh_mark[1];
    C->err_key = ~0ull;
  }
}
constexpr unsigned SHARD_OVF_BLOCKS = 256;
// A small level (<= FUSE_OVF_SCAN_MAX own parents): the overflow list's
// pass B and k_win_scan in one workgroup (engine_kernels.h k_ovf_tile_scan)
__global__ void __launch_bounds__(TSCAN_THREADS)
k_ovf_win_scan(CandOvf ovf, uint64_t n_local, ClaimEntry* __restrict__ cs, uint64_t nslots, uint32_t level,
               uint32_t* __restrict__ newmask, Counters* __restrict__ C, ClaimKeys rank, uint32_t* __restrict__ wtot,
               uint32_t tiles, uint32_t rblocks, uint32_t* __restrict__ woff) {
  settle_ovf_blocks<1>(0, 1, ovf, n_local, 0, cs, nslots, level, newmask, C, rank, wtot);
  __syncthreads();
  __shared__ unsigned int sh_mark[4];
  const uint32_t cells = tiles + rblocks;
  tile_scan_body(wtot, cells, woff, 1, ScanMarks{cells, 2, tiles}, sh_mark);
  if (threadIdx.x == 0) {
    C->chunk_base = sh_mark[2];
    C->level_new = sh_mark[1];
  }
}

// Narrow levels: both exclusive scans (own winners' popcounts, records'
// isnew flags) and k_shard_base's totals in one workgroup, instead of two
// device scans and a launch.
constexpr uint64_t SHARD_SMALL_SCAN = 16384;
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += y;
  }
  if (lane == 63) lds[wv] = x;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t k = 0; k < nw; ++k) {
    const uint32_t t = lds[k];
    if (k < wv) before += t;
    total += t;
  }
  __syncthreads();
  return before + x - v;
}
// Narrow levels at world > 1: the owner-major exclusive scan of the count
// matrix and k_owner_totals in one workgroup (instead of a device scan's two
// launches and the totals launch).
constexpr uint64_t OWNER_SMALL_SCAN = 16384;
__global__ void __launch_bounds__(1024)
k_owner_scan_small(const uint8_t* __restrict__ cnt, uint32_t* __restrict__ off, uint64_t n, uint32_t world,
                   uint64_t* __restrict__ tot, const Counters* __restrict__ C, uint64_t* __restrict__ host_tot,
                   unsigned long long* __restrict__ host_head, uint64_t* __restrict__ row, uint64_t status_new,
                   uint64_t status_err, int level1, uint64_t init_err) {
  __shared__ uint32_t lds[16];
  const uint64_t cells = n * world;
  uint32_t carry = 0, total = 0;
  for (uint64_t b = 0; b < cells; b += blockDim.x) {
    const uint64_t i = b + threadIdx.x;
    const uint32_t v = i < cells ? (uint32_t)cnt[i] : 0u;
    const uint32_t e = block_exclusive_scan(v, lds, total);
    if (i < cells) off[i] = carry + e;
    carry += total;
  }
  __syncthreads();       // (the scan's global writes, for the totals' reads below)
  if (threadIdx.x < 64)
    owner_totals(off, cnt, n, world, tot, C, host_tot, host_head, row, status_new, status_err, level1, init_err);
}
__global__ void __launch_bounds__(1024)
k_shard_scan_small(const uint32_t* __restrict__ newmask, uint64_t nlocal, uint32_t* __restrict__ offsets,
                   const uint32_t* __restrict__ isnew, uint64_t nrec, uint32_t* __restrict__ ioff,
                   Counters* __restrict__ C) {
  __shared__ uint32_t lds[16];
  uint32_t carry = 0, tot = 0;
  for (uint64_t b = 0; b < nlocal; b += blockDim.x) {
    const uint64_t i = b + threadIdx.x;
    const uint32_t v = i < nlocal ? NewCount()(newmask[i]) : 0u;
    const uint32_t e = block_exclusive_scan(v, lds, tot);
    if (i < nlocal) offsets[i] = carry + e;
    carry += tot;
  }
  const uint32_t lt = carry;
  carry = 0;
  for (uint64_t b = 0; b < nrec; b += blockDim.x) {
    const uint64_t i = b + threadIdx.x;
    const uint32_t v = i < nrec ? isnew[i] : 0u;
    const uint32_t e = block_exclusive_scan(v, lds, tot);
    if (i < nrec) ioff[i] = carry + e;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    C->chunk_base = lt;
    C->level_new = (uint64_t)lt + carry;
  }
}

// chunk_base = this rank's own new states (the records' emit base);
// level_new = all new states of the level
__global__ void k_shard_base(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ newmask,
                             uint64_t nlocal, const uint32_t* __restrict__ ioff,
                             const uint32_t* __restrict__ isnew, uint64_t nrec, Counters* __restrict__ C) {
  if (threadIdx.x != 0) return;
  const uint64_t lt = nlocal ? (uint64_t)offsets[nlocal - 1] + NewCount()(newmask[nlocal - 1]) : 0;
  const uint64_t rt = nrec ? (uint64_t)ioff[nrec - 1] + isnew[nrec - 1] : 0;
  C->chunk_base = lt;
  C->level_new = lt + rt;
}

// The winners among the received records, after the local ones (one
// workgroup's share).
// (boff != nullptr, the tile-count path: the block's first position, the
// rest from the block's own isnew flags; else per-record offsets ioff after
// the own states, chunk_base)
__device__ __forceinline__ uint64_t rec_block_pos(uint64_t blk, uint64_t i, uint64_t n,
                                                  const uint32_t* __restrict__ isnew,
                                                  const uint32_t* __restrict__ ioff,
                                                  const uint32_t* __restrict__ boff, const Counters* __restrict__ C,
                                                  bool* won) {
  const bool w = i < n && isnew[i];
  *won = w;
  if (!boff) return w ? C->chunk_base + ioff[i] : 0ull;
  __shared__ unsigned int sh_rw[4];
  const unsigned long long b = __ballot(w);
  const unsigned lane = threadIdx.x & 63;
  if (lane == 0) sh_rw[threadIdx.x >> 6] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned before = 0;
  for (unsigned k = 0; k < (threadIdx.x >> 6); ++k) before += sh_rw[k];
  return (uint64_t)boff[blk] + before + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}
template <class M>
__device__ __forceinline__ void emit_rec_block(uint64_t blk, const Record<M>* __restrict__ in, uint64_t n,
                                               const uint32_t* __restrict__ isnew, const uint32_t* __restrict__ ioff,
                                               const uint32_t* __restrict__ boff,
                                               Flags f, typename M::State* __restrict__ next,
                                               unsigned long long* __restrict__ pkeys, uint64_t next_gidx,
                                               Counters* __restrict__ C) {
  __shared__ unsigned int sh_act[A_COUNT];
  __shared__ unsigned long long sh_cand;
  if (threadIdx.x < A_COUNT) sh_act[threadIdx.x] = 0;
  if (threadIdx.x == 0) sh_cand = 0;
  __syncthreads();
  const uint64_t i = blk * blockDim.x + threadIdx.x;
  unsigned long long cand = 0;
  bool won;
  const uint64_t o = rec_block_pos(blk, i, n, isnew, ioff, boff, C, &won);
  if (won) {
    typename M::State x;
    uint64_t key;
    load_record<M>(in, i, x, key);
    store_state<M>(next, o, x);
    pkeys[next_gidx + o] = key;
    if (M::check(x, f.inv_mask) >= 0) atomicMin(&C->err_key, (key & ~0xffull) | E_INVARIANT);
    // (a record's action byte indexes LDS: a zeroed record of a failed rank
    // reads 0; anything out of range would be a corrupt record, counted nowhere)
    if ((key & 0xff) < (uint64_t)A_COUNT) atomicAdd(&sh_act[key & 0xff], 1u);
    cand = (unsigned long long)M::plan(x, f).total;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cand += __shfl_down(cand, off, 64);
  if ((threadIdx.x & 63) == 0 && cand) atomicAdd(&sh_cand, cand);
  __syncthreads();
  if (threadIdx.x < A_COUNT && sh_act[threadIdx.x])
    atomicAdd(&stripe(C).act_dist[threadIdx.x], (unsigned long long)sh_act[threadIdx.x]);
  if (threadIdx.x == 0 && sh_cand) atomicAdd(&stripe(C).next_cand, sh_cand);
}
// cand_total = sum of the next_cand stripes (one lane per stripe), then the
// level head straight into pinned host memory
__device__ __forceinline__ void level_tail(Counters* __restrict__ C, unsigned long long* __restrict__ host_head) {
  static_assert(CTR_STRIPES == 64, "one lane per stripe");
  unsigned long long v = ld_agent(&C->s[threadIdx.x].next_cand);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (threadIdx.x == 0) {
    C->cand_total = v;
    __threadfence();
    head_to_host(C, host_head);
  }
}
__global__ void __launch_bounds__(64) k_shard_cand(Counters* __restrict__ C,
                                                   unsigned long long* __restrict__ host_head) {
  level_tail(C, host_head);
}
// Both emits in one launch: blocks [0, lblocks) this rank's own winners
// (the engine's wave-balanced emit body, engine_kernels.h emit_body, with
// parent keys), the rest the records'.  Narrow levels (tail != 0): the last
// workgroup to finish runs k_shard_cand's tail; a wide level's grid would
// queue that many device-scope atomics and fences on one counter
// (measured: NP=2 sharded 172 -> 680 ms), so it takes the separate launch.
// woff != nullptr: the tile-count path (k_win_scan's offsets: own tiles,
// then record blocks); else per-parent offsets and per-record ioff.
template <class M>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_shard_emit(const typename M::State* __restrict__ cur, uint64_t n_local, uint32_t lblocks, Flags f, uint64_t rank,
             const uint32_t* __restrict__ newmask, const uint32_t* __restrict__ offsets,
             const Record<M>* __restrict__ in, uint64_t n, const uint32_t* __restrict__ isnew,
             const uint32_t* __restrict__ ioff, typename M::State* __restrict__ next,
             unsigned long long* __restrict__ pkeys, uint64_t next_gidx, Counters* __restrict__ C,
             unsigned long long* __restrict__ host_head, int tail, const uint32_t* __restrict__ woff) {
  __shared__ bool sh_last;
  if (blockIdx.x < lblocks)
    emit_body<M, 0, true>(cur, n_local, 0, f, newmask, offsets, next, 0, 0, next_gidx, pkeys, nullptr, 1, C, woff,
                          rank);
  else
    emit_rec_block<M>(blockIdx.x - lblocks, in, n, isnew, ioff, woff ? woff + lblocks : nullptr, f, next, pkeys,
                      next_gidx, C);
  if (!tail) return;
  // every thread's atomics (error key, stripes) before this workgroup counts as done
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) sh_last = atomicAdd(&C->emit_done, 1ull) == gridDim.x - 1;
  __syncthreads();
  if (!sh_last || threadIdx.x >= 64) return;
  __threadfence();
  if (threadIdx.x == 0) C->emit_done = 0;
  level_tail(C, host_head);
}
constexpr unsigned SHARD_TAIL_BLOCKS = 64;    // emit grids up to this size run the level tail themselves

// The deferred frontier's emit (round 5; the engine's k_emit_links on the
// sharded path): per new state only its link and its parent key (TLC's
// trace file) — own winners at their tile offsets in (parent, position)
// order (link parent << 8 | position), then the received records' winners
// in receive order (link bit 63 | record index: the next level's k_claim
// reads the state from this level's receive buffer).  No state is built,
// stored, checked or planned here: the next level's k_claim rebuilds each
// state as it expands it (shard_rebuild).  Entries at or past `cap` are not
// written and set DF_CAPACITY; the host grows the buffers and runs the
// launch again (it writes nothing else).
template <class M>
__global__ void __launch_bounds__(256)
k_shard_emit_links(uint64_t n_local, uint32_t lblocks, uint64_t rank, const uint32_t* __restrict__ gpos,
                   const uint32_t* __restrict__ newmask,
                   const Record<M>* __restrict__ in, uint64_t n, const uint32_t* __restrict__ isnew,
                   const uint32_t* __restrict__ woff, unsigned long long* __restrict__ link,
                   unsigned long long* __restrict__ pkeys, uint64_t next_gidx, uint64_t cap,
                   Counters* __restrict__ C, unsigned long long* __restrict__ host_head, int tail) {
  __shared__ unsigned int sh_wtot[4];
  __shared__ bool sh_last;
  bool over = false;
  if (blockIdx.x < lblocks) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t tbase = woff[blockIdx.x];         // (loaded with the masks: one round trip less)
    const uint32_t mask = i < n_local ? newmask[i] : 0u;
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
    uint64_t obase = tbase;
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
      if (g >= wtot) continue;
      for (; k > 0; --k) m &= m - 1;
      const uint64_t t = (uint64_t)(__ffs(m) - 1);
      const uint64_t pidx = wave0 + (uint64_t)p;
      const uint64_t o = obase + (uint64_t)g;
      if (o >= cap) {
        over = true;
        continue;
      }
      link[o] = (pidx << 8) | t;
      pkeys[next_gidx + o] = (rank << 60) | ((gpos ? (uint64_t)gpos[pidx] : pidx) << 16) | (t << 8);
    }
  } else {
    const uint64_t blk = blockIdx.x - lblocks;
    const uint64_t i = blk * blockDim.x + threadIdx.x;
    bool won;
    const uint64_t o = rec_block_pos(blk, i, n, isnew, nullptr, woff + lblocks, C, &won);
    if (won) {
      if (o >= cap) {
        over = true;
      } else {
        link[o] = (1ull << 63) | i;
        pkeys[next_gidx + o] = in[i].w[0];
      }
    }
  }
  if (over) atomicOr(&C->defer_flags, DF_CAPACITY);
  if (!tail) return;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) sh_last = atomicAdd(&C->emit_done, 1ull) == gridDim.x - 1;
  __syncthreads();
  if (!sh_last || threadIdx.x >= 64) return;
  __threadfence();
  if (threadIdx.x == 0) C->emit_done = 0;
  level_tail(C, host_head);
}

// A deferred frontier materialised outside k_claim (before a narrow batch,
// at a max_levels stop): the same rebuild, plus the level's successor count.
template <class M, bool TLC>
__global__ void __launch_bounds__(256) k_shard_materialize(DeferArgs df, uint64_t n, Flags f, uint64_t rank,
                                                           Counters* __restrict__ C) {
  __shared__ unsigned int sh_actd[A_COUNT];
  if (threadIdx.x < A_COUNT) sh_actd[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long cand = 0;
  if (i < n) {
    const typename M::State s = shard_rebuild<M, 1, TLC>(df, i, f, rank, sh_actd, C);
    cand = (unsigned long long)M::plan(s, f).total;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cand += __shfl_down(cand, off, 64);
  if ((threadIdx.x & 63) == 0 && cand) atomicAdd(&stripe(C).next_cand, cand);
  __syncthreads();
  if (threadIdx.x < A_COUNT && sh_actd[threadIdx.x])
    atomicAdd(&stripe(C).act_dist[threadIdx.x], (unsigned long long)sh_actd[threadIdx.x]);
}

// ---- seen-set spill (cfg.seen_hbm_bytes > 0), per rank: the engine's hot
// ClaimSet + cold runs (coldset.h, engine_spill.h) over this rank's share of
// the fingerprints.  After a level's settle passes and scans, its winners
// w.r.t. the hot table are checked against the cold tier in windows of
// emit positions [w0, w1): cold key + location (own successor: parent << 5 |
// position; received record: bit 63 | record index).
template <class M>
__global__ void __launch_bounds__(256)
k_shard_spill_queries(const typename M::State* __restrict__ cur, uint64_t n_local, uint32_t lblocks, Flags f,
                      const uint32_t* __restrict__ newmask, const uint32_t* __restrict__ offsets, uint64_t n,
                      const unsigned long long* __restrict__ rfp, const uint32_t* __restrict__ isnew,
                      const uint32_t* __restrict__ ioff, const Counters* __restrict__ C, uint64_t w0, uint64_t w1,
                      uint64_t* __restrict__ qkey, uint64_t* __restrict__ qloc) {
  if (blockIdx.x < lblocks) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_local) return;
    uint32_t mask = newmask[i];
    if (!mask) return;
    const uint64_t o = offsets[i];
    if (o >= w1 || o + (uint64_t)__builtin_popcount(mask) <= w0) return;
    const typename M::State s = load_state<M>(cur, i);
    const typename M::Plan pl = M::plan(s, f);
    const uint64_t fold = M::fp_fold(s);
    const uint32_t proj = M::owner_proj(s);
    for (uint64_t pos = o; mask; mask &= mask - 1, ++pos) {
      if (pos < w0 || pos >= w1) continue;
      const int t = __ffs(mask) - 1;
      int slot, j;
      M::locate(pl, t, slot, j);
      typename M::State x;
      int who;
      M::apply(s, slot, j, f, x, who);
      // (the fingerprint k_claim claimed: owner bits included, as at every world)
      qkey[pos - w0] = cold_key(M::template fingerprint_succ<1>(s, fold, x, who, proj));
      qloc[pos - w0] = (i << 5) | (uint64_t)t;
    }
    return;
  }
  const uint64_t r = (uint64_t)(blockIdx.x - lblocks) * blockDim.x + threadIdx.x;
  if (r >= n || !isnew[r]) return;
  const uint64_t pos = C->chunk_base + ioff[r];
  if (pos < w0 || pos >= w1) return;
  qkey[pos - w0] = cold_key(rfp[r]);
  qloc[pos - w0] = (1ull << 63) | r;
}
// Winners found in the cold tier lose: their newmask bit or isnew flag is
// cleared and their hot slot retired (engine_spill.h claimset_retire).
__global__ void k_shard_spill_apply(const uint64_t* __restrict__ qkey, const uint64_t* __restrict__ qloc,
                                    const uint8_t* __restrict__ found, uint64_t m, uint32_t* __restrict__ newmask,
                                    uint32_t* __restrict__ isnew, ClaimEntry* __restrict__ cs, uint64_t nslots,
                                    Counters* __restrict__ C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !found[i]) return;
  const uint64_t loc = qloc[i];
  if (loc >> 63)
    isnew[loc & ~(1ull << 63)] = 0u;
  else
    atomicAnd(&newmask[loc >> 5], ~(1u << (loc & 31)));
  if (!claimset_retire(cs, nslots, cold_unkey(qkey[i]))) atomicAdd(&C->overflow, 1ull);
}

// ---- TLC order (ShardBase::tlc_*; cfg.tlc_order, world > 1).  Per level of
// global width W, after every rank's insert: k_tlc_mask sets, for each new
// state this rank won, its position bit in its parent's word (parent keys
// carry the parent's G); the words are summed over the ranks (bits of one
// parent are disjoint: every successor has one owner); then G of a new state
// = the winners of the parents before its parent (one scan over the W
// popcounts) + its parent's winners before it (k_tlc_pos), and its local
// index = the rank's G values before it (a bitmap over the next level's G
// and one scan of its word popcounts: k_tlc_perm).  The bitmap and its scan
// stay as the next level's G -> local index map (ClaimKeys::mine).
__global__ void __launch_bounds__(256) k_tlc_mask(const unsigned long long* __restrict__ pk, uint64_t nn,
                                                  uint32_t* __restrict__ wmask, uint64_t W,
                                                  Counters* __restrict__ C) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  const uint64_t key = pk[i];
  const uint64_t g = (key >> 16) & 0xffffffffull;
  const uint32_t t = (uint32_t)((key >> 8) & 0xff);
  if (g >= W || t >= 32) {
    atomicAdd(&C->overflow, 1ull);                // a parent key outside the level: fail loudly
    return;
  }
  atomicOr(&wmask[g], 1u << t);
}
__global__ void __launch_bounds__(256) k_tlc_pos(const unsigned long long* __restrict__ pk, uint64_t nn,
                                                 const uint32_t* __restrict__ wmask,
                                                 const uint32_t* __restrict__ wbase, uint32_t* __restrict__ gnew,
                                                 uint32_t* __restrict__ bits) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  const uint64_t key = pk[i];
  const uint64_t g = (key >> 16) & 0xffffffffull;
  const uint32_t t = (uint32_t)((key >> 8) & 31);
  const uint32_t gn = wbase[g] + (uint32_t)__builtin_popcount(wmask[g] & ((1u << t) - 1u));
  gnew[i] = gn;
  atomicOr(&bits[gn >> 5], 1u << (gn & 31));
}
__global__ void __launch_bounds__(256) k_tlc_perm(uint64_t nn, const uint32_t* __restrict__ gnew,
                                                  const uint32_t* __restrict__ bits,
                                                  const uint32_t* __restrict__ brank,
                                                  const unsigned long long* __restrict__ link_in,
                                                  const unsigned long long* __restrict__ pk_in,
                                                  unsigned long long* __restrict__ link_out,
                                                  unsigned long long* __restrict__ pk_out,
                                                  uint32_t* __restrict__ gpos_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nn) return;
  const uint32_t gn = gnew[i];
  const uint64_t j = (uint64_t)brank[gn >> 5] + (uint64_t)__builtin_popcount(bits[gn >> 5] & ((1u << (gn & 31)) - 1u));
  link_out[j] = link_in[i];
  pk_out[j] = pk_in[i];
  gpos_out[j] = gn;
}

// drop_last_expand: take a level's per-action generated counts back out
// (what k_claim added: each parent's plan slot counts, by action), from the
// level's states and the plans k_claim kept
template <class M>
__global__ void __launch_bounds__(256) k_undo_gen(const typename M::State* __restrict__ st,
                                                  const unsigned long long* __restrict__ counts, uint64_t n,
                                                  Counters* __restrict__ C) {
  __shared__ unsigned int sh[A_COUNT];
  if (threadIdx.x < A_COUNT) sh[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const typename M::State s = load_state<M>(st, i);
    const unsigned long long c = counts[i];
#pragma unroll
    for (int slot = 0; slot < M::NSLOT; ++slot) {
      const unsigned v = (unsigned)((c >> (6 * slot)) & 63);
      if (v) atomicAdd(&sh[M::slot_action(s, slot)], v);
    }
  }
  __syncthreads();
  if (threadIdx.x < A_COUNT && sh[threadIdx.x])
    atomicAdd(&stripe(C).act_gen[threadIdx.x], 0ull - (unsigned long long)sh[threadIdx.x]);   // (mod 2^64)
}

}  // namespace
}  // namespace kc
