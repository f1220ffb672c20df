// shard_selftest.hip — test-only device harness for the sharded level's
// kernels (shard_kernels.h): kc_shard_selftest runs them on inputs of the
// suite's making, with the grids and block sizes ShardT (shard.hip) launches
// them with, for Model<1,1,1> and Model<1,2,1>.
// tests/test_gpu_shard_kernels.py compares the results with
// tests/shard_model.py.
//
//   kind 0  the owner scans: k_owner_tscan, k_owner_cscan, k_owner_scan_small,
//           or hipcub's exclusive sum through Widen8 + k_owner_totals
//   kind 1  k_shard_gather<M>, chunked or not
//   kind 2  k_tlc_mask, the other ranks' words, then tlc_order's sequence:
//           the NewCount scan, k_tlc_pos, the bitmap scan, k_tlc_perm
//   kind 3  k_shard_pack<M>, with or without gpos
//   kind 4  k_shard_materialize<M, false / true>
//   kind 5  k_undo_gen<M>
//   kind 6  the deterministic insert: k_head_reset, the sharded k_claim<M, 0,
//           true, 1> (or its TLC-order variant; claim_selftest_launch.h, shared
//           with claim_selftest.hip), k_rec_claim, k_settle_both<M, 0>,
//           k_settle_both<M, 1>, then k_ovf_win_scan, or k_settle_ovf<1> +
//           k_win_scan, or k_shard_scan_small, or hipcub's scans +
//           k_shard_base; then k_shard_emit or k_shard_emit_links, with
//           k_shard_cand when the emit does not run the level tail
//   kind 7  the first-claim insert: k_claim FIRST (16-B slots or the compact
//           table), k_rec_claim_first, k_win_scan, either emit
//
// Not driven: k_shard_spill_queries / k_shard_spill_apply, shard_narrow.h,
// shard_driver.hip's kernels, record staging inside k_claim (claim_selftest.hip
// kind 3 drives it), a full seen-set (CL_FULL).
//
// Data travels as u64 words, one per element whatever the kernel's element
// type.  Every output section is uploaded as the caller filled it and copied
// back whole: KC_EMIT_FORE guard elements, the kernel's array, the caller's
// aft guards.  The harness checks, on the host and before any launch,
// everything a kernel's indices depend on (so a machine without a GPU answers
// -EINVAL to bad input and -ENODEV only to good input).  Nothing of the
// product path calls this file.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/kubecheck.h"
#include "claim_launch.h"
#include "claim_selftest_launch.h"
#include "engine_kernels.h"
#include "engine_util.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "record.h"
#include "selftest_util.h"
#include "shard_kernels.h"

namespace kc {
namespace {

using selftest::DevBuf;
using selftest::upload;

constexpr uint64_t FORE = KC_EMIT_FORE;
constexpr uint64_t kMaxCells = 1ull << 22, kMaxAft = 1ull << 10;
constexpr uint32_t PAD_CELL = 0xA5A5A5A5u;   // what the scans' pad cells hold

int bad(const char* what) {
  set_error("kc_shard_selftest: %s", what);
  return -EINVAL;
}

// One output section: `len` elements of T on the device, filled from the
// caller's u64 words and copied back into them.
template <class T>
struct Section {
  DevBuf d;
  uint64_t len = 0;
  T* ptr() const { return d.as<T>() + FORE; }
  int up(const uint64_t* src, uint64_t n) {
    len = n;
    std::vector<T> h(n);
    for (uint64_t i = 0; i < n; ++i) h[i] = (T)src[i];
    return upload(d, h.data(), n * sizeof(T));
  }
  int down(uint64_t* dst) const {
    std::vector<T> h(len);
    KC_HIP_TRY(hipMemcpy(h.data(), d.p, len * sizeof(T), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < len; ++i) dst[i] = (uint64_t)h[i];
    return 0;
  }
};
// The same in pinned host memory (what the product's kernels write the owner
// totals and the level head into).
struct PinnedSection {
  PinnedArray<uint64_t> h;
  uint64_t len = 0;
  uint64_t* ptr() const { return h.p + FORE; }
  int up(const uint64_t* src, uint64_t n) {
    len = n;
    KC_TRY(h.alloc(n));
    memcpy(h.p, src, n * 8);
    return 0;
  }
  void down(uint64_t* dst) const { memcpy(dst, h.p, len * 8); }
};

int need_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_shard_selftest: no HIP device");
    return -ENODEV;
  }
  return 0;
}

int sync_launch() {
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  return 0;
}

// out = nsec sections of FORE + need[k] + aft words; at[k] = where section k starts
bool layout(const uint64_t* need, int nsec, uint64_t aft, uint64_t nout, uint64_t* at) {
  at[0] = 0;
  for (int k = 0; k < nsec; ++k) at[k + 1] = at[k] + FORE + need[k] + aft;
  return nout == at[nsec];
}

// hipcub's exclusive sum as ShardT spells it (size query, scratch, the scan)
template <class In>
int exclusive_sum(In in, uint32_t* out, uint64_t n, DevBuf& tmp) {
  size_t tmp_bytes = 0;
  KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, out, (int)n, nullptr));
  KC_TRY(tmp.alloc(tmp_bytes + 16));
  KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, in, out, (int)n, nullptr));
  return 0;
}

// ---------------------------------------------------------------- owner scans
// kind 0.  par = [mode, world, T, status_new, status_err, level1, init_err,
// want_row, aft]; mode 0 k_owner_tscan, 1 k_owner_cscan (T cells per owner,
// u32), 2 k_owner_scan_small, 3 hipcub + k_owner_totals (T = n parents, u8
// cells).  a = the world * T cells, owner-major; b = the first ten words of
// Counters.  out = off, tot[16], host_tot[16] and host_head[10] (pinned),
// row[world + 3].  res = the cells after the launch.
int run_owner_scan(const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb,
                   uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  if (!par || npar != 9 || !b || nb != 10 || !out) return bad("owner scan: 9 scalars, 10 head words, out");
  const uint64_t mode = par[0], world = par[1], T = par[2], aft = par[8];
  if (mode > 3 || world < 1 || world > 15 || par[5] > 1 || par[7] > 1 || aft > kMaxAft)
    return bad("owner scan: mode 0-3, world 1 to 15, level1 and want_row 0 or 1");
  const bool tiles = mode < 2;
  if (T > kMaxCells || (tiles && T == 0)) return bad("owner scan: 1 to 2^22 cells per owner (modes 2, 3: from 0)");
  const uint64_t cells = world * T;
  if (cells > (mode == 2 ? OWNER_SMALL_SCAN : kMaxCells))
    return bad("owner scan: world * T up to 2^22 (mode 2: up to OWNER_SMALL_SCAN)");
  if (na != cells || nres != cells || (cells && (!a || !res))) return bad("owner scan: a and res of world * T cells");
  uint64_t sum = 0;
  for (uint64_t i = 0; i < cells; ++i) {
    if (a[i] >> (tiles ? 32 : 8)) return bad("owner scan: a cell over its width (32 bits; modes 2, 3: 8)");
    sum += a[i];
  }
  if (sum >> 32) return bad("owner scan: the total does not fit 32 bits");
  const uint64_t G = (cells + 3) / 4;
  const uint64_t need[5] = {tiles ? std::max(4 * G, cells + 1) : cells, 16, 16, 10, world + 3};
  uint64_t at[6];
  if (!layout(need, 5, aft, nout, at)) return bad("owner scan: out of 5 sections: off, tot, host_tot, host_head, row");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  auto len = [&](int k) { return FORE + need[k] + aft; };
  DevBuf in, ctr, tmp;
  Section<uint32_t> off;
  Section<uint64_t> tot, row;
  PinnedSection host_tot, host_head;
  if (tiles) {
    std::vector<uint32_t> h(4 * G, PAD_CELL);
    for (uint64_t i = 0; i < cells; ++i) h[i] = (uint32_t)a[i];
    KC_TRY(upload(in, h.data(), h.size() * 4));
  } else {
    std::vector<uint8_t> h(cells);
    for (uint64_t i = 0; i < cells; ++i) h[i] = (uint8_t)a[i];
    KC_TRY(upload(in, h.data(), cells));
  }
  KC_TRY(off.up(out + at[0], len(0)));
  KC_TRY(tot.up(out + at[1], len(1)));
  KC_TRY(host_tot.up(out + at[2], len(2)));
  KC_TRY(host_head.up(out + at[3], len(3)));
  KC_TRY(row.up(out + at[4], len(4)));
  KC_TRY(ctr.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(ctr.p, 0, sizeof(Counters)));
  KC_HIP_TRY(hipMemcpy(ctr.p, b, 10 * 8, hipMemcpyHostToDevice));
  uint64_t* const d_row = par[7] ? row.ptr() : nullptr;
  unsigned long long* const head = reinterpret_cast<unsigned long long*>(host_head.ptr());
  const uint64_t status_new = par[3], status_err = par[4], init_err = par[6];
  const int level1 = (int)par[5];
  if (mode == 0) {
    // ShardT::expand_dev, the staged level
    hipLaunchKernelGGL(k_owner_tscan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, in.as<const uint32_t>(), (uint32_t)T,
                       (uint32_t)world, off.ptr(), tot.ptr(), ctr.as<const Counters>(), host_tot.ptr(), head, d_row,
                       status_new, status_err, level1, init_err);
  } else if (mode == 1) {
    // ShardT::expand_dev, the staged level with chunk sums
    hipLaunchKernelGGL(k_owner_cscan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, in.as<uint32_t>(), (uint32_t)T,
                       (uint32_t)world, off.ptr(), tot.ptr(), ctr.as<const Counters>(), host_tot.ptr(), head, d_row,
                       status_new, status_err, level1, init_err);
  } else if (mode == 2) {
    // ShardT::expand_dev, cells <= OWNER_SMALL_SCAN
    hipLaunchKernelGGL(k_owner_scan_small, dim3(1), dim3(1024), 0, nullptr, in.as<const uint8_t>(), off.ptr(), T,
                       (uint32_t)world, tot.ptr(), ctr.as<const Counters>(), host_tot.ptr(), head, d_row, status_new,
                       status_err, level1, init_err);
  } else {
    // ShardT::expand_dev / ShardT::pack, the device scan (nothing to scan at world 1)
    if (world > 1 && cells) {
      const hipcub::TransformInputIterator<uint32_t, Widen8, const uint8_t*> cnt32(in.as<const uint8_t>(), Widen8());
      KC_TRY(exclusive_sum(cnt32, off.ptr(), cells, tmp));
    }
    hipLaunchKernelGGL(k_owner_totals, dim3(1), dim3(64), 0, nullptr, off.ptr(), in.as<const uint8_t>(), T,
                       (uint32_t)world, tot.ptr(), ctr.as<const Counters>(), host_tot.ptr(), head, d_row, status_new,
                       status_err, level1, init_err);
  }
  KC_TRY(sync_launch());
  KC_TRY(off.down(out + at[0]));
  KC_TRY(tot.down(out + at[1]));
  host_tot.down(out + at[2]);
  host_head.down(out + at[3]);
  KC_TRY(row.down(out + at[4]));
  if (tiles) {
    std::vector<uint32_t> h(cells);
    KC_HIP_TRY(hipMemcpy(h.data(), in.p, cells * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < cells; ++i) res[i] = h[i];
  } else if (cells) {
    std::vector<uint8_t> h(cells);
    KC_HIP_TRY(hipMemcpy(h.data(), in.p, cells, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < cells; ++i) res[i] = h[i];
  }
  return 0;
}

// --------------------------------------------------------------------- gather
// kind 1.  par = [world, T, chunked, nstage, aft]; a = the staging buffer,
// nstage records of raw words; b = stoff[T] (~0: the tile staged nothing),
// tcnt[world][T], then toff[world][T] (chunked 0) or coff[world][ceil(T /
// CSUM_TILES)] (chunked 1), which must be the owner-major exclusive sums of
// tcnt, or of its chunk sums.  A staged tile's segment lies inside the staging
// buffer.  out = the send buffer: exactly the sum of tcnt records.
template <class M>
int run_gather(const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb,
               uint64_t* out, uint64_t nout) {
  constexpr uint64_t RW = Record<M>::RW;
  static_assert(FORE % 2 == 0, "the send buffer behind the guards is 16-B aligned");
  if (!par || npar != 5 || !b || !out) return bad("gather: 5 scalars, b and out");
  const uint64_t world = par[0], T = par[1], chunked = par[2], nstage = par[3], aft = par[4];
  if (world < 1 || world > 15 || T == 0 || T > (1ull << 16) || chunked > 1 || nstage > kMaxCells || aft > kMaxAft)
    return bad("gather: world 1 to 15, 1 to 2^16 tiles, chunked 0 or 1, up to 2^22 staged records");
  if (na != nstage * RW || (na && !a)) return bad("gather: a holds nstage records");
  const uint64_t nC = (T + CSUM_TILES - 1) / CSUM_TILES, cells = world * T, ncell = chunked ? world * nC : cells;
  if (nb != T + cells + ncell) return bad("gather: b holds stoff[T], tcnt[world][T] and the offsets");
  const uint64_t *stoff = b, *tcnt = b + T, *offs = b + T + cells;
  uint64_t run = 0;
  for (uint64_t o = 0; o < world; ++o)
    for (uint64_t t = 0; t < T; ++t) {
      if (!chunked ? offs[o * T + t] != run : (t % CSUM_TILES == 0 && offs[o * nC + t / CSUM_TILES] != run))
        return bad("gather: the offsets are not the owner-major exclusive sums of tcnt");
      if (tcnt[o * T + t] > kMaxCells) return bad("gather: a tile count over 2^22");
      run += tcnt[o * T + t];
      if (run > kMaxCells) return bad("gather: more than 2^22 records");
    }
  for (uint64_t t = 0; t < T; ++t) {
    if (stoff[t] == ~0ull) continue;
    uint64_t seg = 0;
    for (uint64_t o = 0; o < world; ++o) seg += tcnt[o * T + t];
    if (stoff[t] > nstage || seg > nstage - stoff[t]) return bad("gather: a tile's segment outside the staging buffer");
  }
  uint64_t at[2];
  const uint64_t need[1] = {run * RW};
  if (!layout(need, 1, aft, nout, at)) return bad("gather: out of fore guards + the records' words + aft guards");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf stage, so, tc, to;
  Section<uint64_t> send;
  KC_TRY(upload(stage, a, na * 8));
  KC_TRY(upload(so, stoff, T * 8));
  std::vector<uint32_t> h(cells + ncell);
  for (uint64_t i = 0; i < cells + ncell; ++i) h[i] = (uint32_t)tcnt[i];
  KC_TRY(upload(tc, h.data(), cells * 4));
  KC_TRY(upload(to, h.data() + cells, ncell * 4));
  KC_TRY(send.up(out, nout));
  // ShardT::pack, the staged level
  hipLaunchKernelGGL(k_shard_gather<M>, dim3((unsigned)T), dim3(256), 0, nullptr, stage.as<const Record<M>>(),
                     so.as<const unsigned long long>(), tc.as<const uint32_t>(), to.as<const uint32_t>(), (uint32_t)T,
                     (uint32_t)world, reinterpret_cast<Record<M>*>(send.ptr()), (int)chunked);
  KC_TRY(sync_launch());
  return send.down(out);
}

// ------------------------------------------------------------------ TLC order
// kind 2.  par = [nn, W, aft]; a = pkeys[nn] (parent G << 16 | position << 8 |
// action), then link[nn]; b = other[W], the other ranks' position words, OR-ed
// into this rank's after k_tlc_mask (the all-reduce's stand-in).  out = wmask[W],
// wbase[W], gnew[nn], bits[W + 1], brank[W + 1], link_out[nn], pk_out[nn],
// gpos_out[nn].  res = [Counters::overflow].  A key with G >= W or position >=
// 32 is counted by k_tlc_mask; ShardT::tlc_order's kernels would index with it,
// so the harness then stops after k_tlc_mask.
int run_tlc(const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb,
            uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  if (!par || npar != 3 || !b || !out || !res || nres != 1) return bad("tlc: 3 scalars, b, out, res of 1 word");
  const uint64_t nn = par[0], W = par[1], aft = par[2], words = W + 1;
  if (nn > (1ull << 20) || W == 0 || W > (1ull << 20) || aft > kMaxAft)
    return bad("tlc: up to 2^20 new states, a level of 1 to 2^20 states");
  if (na != 2 * nn || (nn && !a) || nb != W) return bad("tlc: a holds pkeys[nn] and link[nn], b other[W]");
  bool outside = false;
  for (uint64_t i = 0; i < nn; ++i)
    if (((a[i] >> 16) & 0xffffffffull) >= W || ((a[i] >> 8) & 0xff) >= 32) outside = true;
  for (uint64_t g = 0; g < W; ++g)
    if (b[g] >> 32) return bad("tlc: a position word over 32 bits");
  const uint64_t need[8] = {W, W, nn, words, words, nn, nn, nn};
  uint64_t at[9];
  if (!layout(need, 8, aft, nout, at)) return bad("tlc: out of 8 sections");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  auto len = [&](int k) { return FORE + need[k] + aft; };
  DevBuf pk, lk, ctr, tmp, tmp2;
  Section<uint32_t> wmask, wbase, gnew, bits, brank, gpos;
  Section<unsigned long long> link_out, pk_out;
  KC_TRY(upload(pk, a, nn * 8));
  KC_TRY(upload(lk, a + nn, nn * 8));
  KC_TRY(wmask.up(out + at[0], len(0)));
  KC_TRY(wbase.up(out + at[1], len(1)));
  KC_TRY(gnew.up(out + at[2], len(2)));
  KC_TRY(bits.up(out + at[3], len(3)));
  KC_TRY(brank.up(out + at[4], len(4)));
  KC_TRY(link_out.up(out + at[5], len(5)));
  KC_TRY(pk_out.up(out + at[6], len(6)));
  KC_TRY(gpos.up(out + at[7], len(7)));
  KC_TRY(ctr.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(ctr.p, 0, sizeof(Counters)));
  // ShardT::tlc_masks
  KC_HIP_TRY(hipMemsetAsync(wmask.ptr(), 0, W * 4, nullptr));
  if (nn)
    hipLaunchKernelGGL(k_tlc_mask, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, nullptr,
                       pk.as<const unsigned long long>(), nn, wmask.ptr(), W, ctr.as<Counters>());
  KC_TRY(sync_launch());
  if (!outside) {
    // (the other ranks' words: the caller's all-reduce between the two calls)
    std::vector<uint32_t> h(W);
    KC_HIP_TRY(hipMemcpy(h.data(), wmask.ptr(), W * 4, hipMemcpyDeviceToHost));
    for (uint64_t g = 0; g < W; ++g) h[g] |= (uint32_t)b[g];
    KC_HIP_TRY(hipMemcpy(wmask.ptr(), h.data(), W * 4, hipMemcpyHostToDevice));
    // ShardT::tlc_order
    KC_HIP_TRY(hipMemsetAsync(bits.ptr(), 0, words * 4, nullptr));
    const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> wc(wmask.ptr(), NewCount());
    KC_TRY(exclusive_sum(wc, wbase.ptr(), W, tmp));
    const unsigned g = (unsigned)((nn + 255) / 256);
    if (nn)
      hipLaunchKernelGGL(k_tlc_pos, dim3(g), dim3(256), 0, nullptr, pk.as<const unsigned long long>(), nn, wmask.ptr(),
                         wbase.ptr(), gnew.ptr(), bits.ptr());
    const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> bc(bits.ptr(), NewCount());
    KC_TRY(exclusive_sum(bc, brank.ptr(), words, tmp2));
    if (nn)
      hipLaunchKernelGGL(k_tlc_perm, dim3(g), dim3(256), 0, nullptr, nn, gnew.ptr(), bits.ptr(), brank.ptr(),
                         lk.as<const unsigned long long>(), pk.as<const unsigned long long>(), link_out.ptr(),
                         pk_out.ptr(), gpos.ptr());
    KC_TRY(sync_launch());
  }
  KC_TRY(wmask.down(out + at[0]));
  KC_TRY(wbase.down(out + at[1]));
  KC_TRY(gnew.down(out + at[2]));
  KC_TRY(bits.down(out + at[3]));
  KC_TRY(brank.down(out + at[4]));
  KC_TRY(link_out.down(out + at[5]));
  KC_TRY(pk_out.down(out + at[6]));
  KC_TRY(gpos.down(out + at[7]));
  std::vector<Counters> hc(1);
  KC_HIP_TRY(hipMemcpy(hc.data(), ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
  res[0] = hc[0].overflow;
  return 0;
}

// ----------------------------------------------------------------------- states
template <class M>
typename M::State state_of(const uint64_t* w) {
  typename M::State s;
  for (int k = 0; k < M::W; ++k) s.w[k] = w[k];
  return s;
}
// a state of the lowered domain: it survives the round trip through its tuple
template <class M>
bool in_domain(const typename M::State& s) {
  typename M::State r;
  uint64_t tup[M::TUPLE_WORDS];
  M::to_tuple(s, tup);
  bool same = M::from_tuple(tup, r);
  for (int k = 0; same && k < M::W; ++k) same = r.w[k] == s.w[k];
  return same;
}
inline uint32_t host_owner(uint64_t fp, uint64_t world) {      // owner_of, on the host
  return (uint32_t)(((unsigned __int128)(fp << 1) * world) >> 64);
}
// Records given as state words + key -> their wire form (record_pack, host side)
template <class M>
int pack_records(const uint64_t* src, uint64_t n, std::vector<uint64_t>& raw) {
  constexpr uint64_t RW = Record<M>::RW;
  raw.assign(std::max<uint64_t>(n, 1) * RW, 0);
  for (uint64_t r = 0; r < n; ++r) {
    const typename M::State x = state_of<M>(src + r * (M::W + 1));
    if (!in_domain<M>(x)) return bad("a record's state is not a packed state of the model");
    uint64_t w[RW];
    record_pack<M>(x, src[r * (M::W + 1) + M::W], w);
    for (uint64_t k = 0; k < RW; ++k) raw[r * RW + k] = w[k];
  }
  return 0;
}

// ----------------------------------------------------------------------- pack
// kind 3.  par = [n, world, rank, with_gpos, aft]; a = n packed parents raising
// no Assert; b = repmask[n] (bits below each parent's successor count), then
// gpos[n] when with_gpos.  The harness counts the marked successors per owner
// and parent with the kernel's own host code and gives the kernel their
// owner-major exclusive sums.  out = the send buffer, exactly the marked
// successors' records, then the same records unpacked on the host (state
// words, then the key).  res = the records per owner [world].
template <class M>
int run_pack(const Flags& f, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b,
             uint64_t nb, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  constexpr uint64_t RW = Record<M>::RW;
  if (!par || npar != 5 || !a || !b || !out || !res) return bad("pack: 5 scalars, a, b, out and res");
  const uint64_t n = par[0], world = par[1], rank = par[2], gp = par[3], aft = par[4];
  if (n == 0 || n > (1ull << 17) || world < 1 || world > 15 || rank >= world || gp > 1 || aft > kMaxAft)
    return bad("pack: 1 to 2^17 parents, world 1 to 15, rank below it, with_gpos 0 or 1");
  if (na != n * M::W || nb != (gp ? 2 * n : n) || nres != world)
    return bad("pack: a of n states, b of repmask[n] (and gpos[n]), res of world words");
  std::vector<int> tot;
  if (const char* why = selftest::check_states<M>(a, n, f, tot)) return bad(why);
  std::vector<uint32_t> cnt(world * n, 0), off(world * n);
  for (uint64_t i = 0; i < n; ++i) {
    if (b[i] >> tot[i]) return bad("pack: a repmask bit at or past the parent's successor count");
    if (gp && b[n + i] >> 32) return bad("pack: a G over 32 bits");
    const typename M::State s = state_of<M>(a + i * M::W);
    const typename M::Plan pl = M::plan(s, f);
    const uint64_t fold = M::fp_fold(s);
    for (uint32_t mask = (uint32_t)b[i]; mask; mask &= mask - 1) {
      int slot, j, who;
      M::locate(pl, __builtin_ctz(mask), slot, j);
      typename M::State x;
      M::apply(s, slot, j, f, x, who);
      ++cnt[host_owner(M::template fingerprint_succ<1>(s, fold, x, who, M::owner_proj(s)), world) * n + i];
    }
  }
  uint64_t run = 0;
  for (uint64_t o = 0; o < world; ++o) {
    res[o] = run;
    for (uint64_t i = 0; i < n; ++i) {
      off[o * n + i] = (uint32_t)run;
      run += cnt[o * n + i];
    }
    res[o] = run - res[o];
  }
  uint64_t at[3];
  const uint64_t need[2] = {run * RW, run * (M::W + 1)};
  if (!layout(need, 2, aft, nout, at)) return bad("pack: out of the marked successors' records, raw and unpacked");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf cur, rm, of, gpos;
  Section<uint64_t> send;
  KC_TRY(upload(cur, a, na * 8));
  std::vector<uint32_t> h(2 * n);
  for (uint64_t i = 0; i < nb; ++i) h[i] = (uint32_t)b[i];
  KC_TRY(upload(rm, h.data(), n * 4));
  KC_TRY(upload(gpos, h.data() + n, gp ? n * 4 : 0));
  KC_TRY(upload(of, off.data(), off.size() * 4));
  KC_TRY(send.up(out, at[1]));
  // ShardT::pack, a level that staged nothing
  hipLaunchKernelGGL(k_shard_pack<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     cur.as<const typename M::State>(), n, f, (uint32_t)world, rank, of.as<const uint32_t>(),
                     rm.as<const uint32_t>(), reinterpret_cast<Record<M>*>(send.ptr()),
                     gp ? gpos.as<const uint32_t>() : (const uint32_t*)nullptr);
  KC_TRY(sync_launch());
  KC_TRY(send.down(out));
  // the same records unpacked on the host: state words, then the key
  for (uint64_t r = 0; r < run; ++r) {
    uint64_t w[RW];
    for (uint64_t k = 0; k < RW; ++k) w[k] = out[FORE + r * RW + k];
    typename M::State x;
    uint64_t key;
    record_unpack<M>(w, x, key);
    uint64_t* o = out + at[1] + FORE + r * (M::W + 1);
    for (int k = 0; k < M::W; ++k) o[k] = x.w[k];
    o[M::W] = key;
  }
  return 0;
}

// ------------------------------------------------------------------ materialise
// kind 4.  par = [n, nprev, nrec, rank, tlc, prev_counts, aft]; a = nprev
// packed states of the previous frontier raising no Assert, then (tlc 1)
// prev_gpos[nprev]; b = link[n] (parent << 8 | position inside the previous
// frontier and below the parent's successor count, or bit 63 | record index
// below nrec), then the previous level's receive buffer: nrec records as state
// words + key (the harness packs them).  out = n states.  res = [defer_err,
// next_cand, act_dist[A_COUNT]].
template <class M>
int run_shard_materialize(const Flags& f, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na,
                          const uint64_t* b, uint64_t nb, uint64_t* out, uint64_t nout, uint64_t* res,
                          uint64_t nres) {
  constexpr uint64_t W = M::W;
  if (!par || npar != 7 || !a || !b || !out || !res) return bad("materialize: 7 scalars, a, b, out and res");
  const uint64_t n = par[0], nprev = par[1], nrec = par[2], rank = par[3], tlc = par[4], aft = par[6];
  if (n == 0 || n > (1ull << 20) || nprev == 0 || nprev > (1ull << 17) || nrec > (1ull << 20) || rank > 14 ||
      tlc > 1 || par[5] > 1 || aft > kMaxAft)
    return bad("materialize: 1 to 2^20 states, 1 to 2^17 previous states, up to 2^20 records, rank 0 to 14");
  if (na != nprev * W + (tlc ? nprev : 0) || nb != n + nrec * (W + 1) || nres != 2 + (uint64_t)A_COUNT)
    return bad("materialize: a of nprev states (and prev_gpos), b of n links and nrec records, res of 2 + A_COUNT");
  std::vector<int> tot;
  if (const char* why = selftest::check_states<M>(a, nprev, f, tot)) return bad(why);
  for (uint64_t i = 0; tlc && i < nprev; ++i)
    if (a[nprev * W + i] >> 32) return bad("materialize: a G over 32 bits");
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t lk = b[i];
    if (lk >> 63) {
      if ((lk & ~(1ull << 63)) >= nrec) return bad("materialize: a record link outside the receive buffer");
    } else if ((lk >> 8) >= nprev || (lk & 0xff) >= (uint64_t)tot[lk >> 8]) {
      return bad("materialize: a link outside the previous frontier or past its parent's successor count");
    }
  }
  std::vector<uint64_t> raw;
  KC_TRY(pack_records<M>(b + n, nrec, raw));
  std::vector<unsigned long long> counts(nprev);
  for (uint64_t i = 0; i < nprev; ++i) counts[i] = M::plan(state_of<M>(a + i * W), f).counts;
  uint64_t at[2];
  const uint64_t need[1] = {n * W};
  if (!layout(need, 1, aft, nout, at)) return bad("materialize: out of fore guards + n states + aft guards");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf prev, lk, rec, pc, gpos, ctr;
  Section<uint64_t> o;
  KC_TRY(upload(prev, a, nprev * W * 8));
  KC_TRY(upload(lk, b, n * 8));
  KC_TRY(upload(rec, raw.data(), raw.size() * 8));
  KC_TRY(upload(pc, counts.data(), nprev * 8));
  std::vector<uint32_t> g(nprev, 0);
  for (uint64_t i = 0; tlc && i < nprev; ++i) g[i] = (uint32_t)a[nprev * W + i];
  KC_TRY(upload(gpos, g.data(), nprev * 4));
  KC_TRY(o.up(out, nout));
  KC_TRY(ctr.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(ctr.p, 0, sizeof(Counters)));
  const unsigned long long none = ~0ull;
  KC_HIP_TRY(hipMemcpy(ctr.p, &none, 8, hipMemcpyHostToDevice));                                  // err_key
  // ShardT::materialize
  DeferArgs df;
  df.prev = prev.p;
  df.link = lk.as<const unsigned long long>();
  df.prev_rec = rec.p;
  df.out = o.ptr();
  if (par[5]) df.prev_counts = pc.as<const unsigned long long>();
  if (tlc) df.prev_gpos = gpos.as<const uint32_t>();
  KC_HIP_TRY(hipMemsetAsync(&ctr.as<Counters>()->defer_err, 0xff, 8, nullptr));
  if (tlc)
    hipLaunchKernelGGL((k_shard_materialize<M, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, df, n,
                       f, rank, ctr.as<Counters>());
  else
    hipLaunchKernelGGL((k_shard_materialize<M, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, df,
                       n, f, rank, ctr.as<Counters>());
  KC_TRY(sync_launch());
  KC_TRY(o.down(out));
  std::vector<Counters> hc(1);
  KC_HIP_TRY(hipMemcpy(hc.data(), ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
  res[0] = hc[0].defer_err;
  res[1] = hc[0].next_cand();
  for (int k = 0; k < A_COUNT; ++k) res[2 + k] = hc[0].act_dist(k);
  return 0;
}

// ------------------------------------------------------------------------ undo
// kind 5.  par = [n]; a = n packed states (an Assert parent is legal); b =
// act_gen[A_COUNT] before.  The plans are those k_claim keeps (Plan::counts of
// each state).  res = act_gen[A_COUNT] after k_undo_gen, mod 2^64.
template <class M>
int run_undo(const Flags& f, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b,
             uint64_t nb, uint64_t* res, uint64_t nres) {
  if (!par || npar != 1 || !a || !b || !res) return bad("undo: 1 scalar, a, b and res");
  const uint64_t n = par[0];
  if (n == 0 || n > (1ull << 17) || na != n * M::W || nb != (uint64_t)A_COUNT || nres != (uint64_t)A_COUNT)
    return bad("undo: 1 to 2^17 states, act_gen of A_COUNT words in and out");
  std::vector<unsigned long long> counts(n);
  for (uint64_t i = 0; i < n; ++i) {
    const typename M::State s = state_of<M>(a + i * M::W);
    if (!in_domain<M>(s)) return bad("undo: a state is not a packed state of the model");
    counts[i] = M::plan(s, f).counts;
  }
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf st, pc, ctr;
  KC_TRY(upload(st, a, na * 8));
  KC_TRY(upload(pc, counts.data(), n * 8));
  std::vector<Counters> hc(1);
  memset(hc.data(), 0, sizeof(Counters));
  for (int k = 0; k < A_COUNT; ++k) hc[0].s[0].act_gen[k] = b[k];
  KC_TRY(upload(ctr, hc.data(), sizeof(Counters)));
  // ShardT::drop_last_expand
  hipLaunchKernelGGL(k_undo_gen<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     st.as<const typename M::State>(), pc.as<const unsigned long long>(), n, ctr.as<Counters>());
  KC_TRY(sync_launch());
  KC_HIP_TRY(hipMemcpy(hc.data(), ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
  for (int k = 0; k < A_COUNT; ++k) res[k] = hc[0].act_gen(k);
  return 0;
}

// ---------------------------------------------------------------------- insert
// kinds 6 (deterministic) and 7 (first-claim): one rank's half of a level after
// the exchange, as ShardT::expand_dev / insert / insert_emit launch it.
// par = [n_local, nrec, level (the successors'), nslots, world, rank, path,
//   tlc, emit, cap, tail, unfused, next_gidx, aft, cap2, W]
//   path   kind 6: 0 = tile counts (k_settle_both<1> with wtot, then
//          k_ovf_win_scan, or with unfused 1 k_settle_ovf<1> + k_win_scan),
//          1 = k_settle_both<1> without wtot + k_shard_scan_small, 2 = the same
//          with hipcub's scans + k_shard_base.  kind 7: 0 = 16-B slots, 1 =
//          the compact table (nslots even).
//   tlc    1 = TLC-order claim keys (kind 6, path 0, emit 1): a then ends with
//          gpos[n_local], strictly increasing and below W, the level's width;
//          the harness builds gbits / grank from it as ShardT::init does
//   emit   0 = k_shard_emit, 1 = k_shard_emit_links with `cap` (path 0 only);
//          cap2 != 0: when the first launch sets DF_CAPACITY, defer_flags is
//          cleared and the launch repeated with cap2, as insert_emit does
//   tail   1 = the emit's last workgroup runs the level tail, 0 = k_shard_cand
// a = n_local packed parents (n_local may be 0); b = nrec records as state
//   words + key, senders below world and not this rank (TLC: parent G below
//   W); table = the image, in and out, nslots >= stored + the parents'
//   successors + nrec + 1 (TLC: a same-level claim's G below 32 (W / 32 + 1)).
// out = newmask[n_local], rfp[nrec], flag[nrec], isnew[nrec], wtot and woff
//   [own tiles + record blocks + 8] (else empty), offsets[n_local] and
//   ioff[nrec] (kind 6 path 1, 2; else empty), next[bound states] (emit 0),
//   link[bound] (emit 1), pkeys[next_gidx + bound + 1]; bound = the parents'
//   successors + nrec.
// res = [err_key, overflow, probes, chunk_base, level_new, cand_total,
//   defer_flags, defer_flags after the first emit launch, act_dist[A_COUNT],
//   the host head's 10 words (pinned memory; 0xA5.. before)].
constexpr int INS_NPAR = 16, INS_NSEC = 11, INS_NRES = 8 + A_COUNT + 10;
template <class M>
int run_insert(bool first, const kc_model_config& cfg, const uint64_t* par, uint64_t npar, const uint64_t* a,
               uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* table, uint64_t ntable, uint64_t* out,
               uint64_t nout, uint64_t* res, uint64_t nres) {
  using State = typename M::State;
  constexpr uint64_t W = M::W;
  const Flags f = flags_of(cfg);
  if (!par || npar != (uint64_t)INS_NPAR || !out || !res || nres != (uint64_t)INS_NRES || !table)
    return bad("insert: 16 scalars, the table, out, res of 8 + A_COUNT + 10 words");
  const uint64_t n = par[0], nrec = par[1], level = par[2], nslots = par[3], world = par[4], rank = par[5];
  const uint64_t path = par[6], tlc = par[7], links = par[8], cap = par[9], tail = par[10], unfused = par[11];
  const uint64_t next_gidx = par[12], aft = par[13], cap2 = par[14], LW = par[15];
  const bool c8 = first && path == 1, tc = first || path == 0;
  if (n > (1ull << 17) || nrec > (1ull << 17) || n + nrec == 0 || level == 0 || level >= (1u << 20) || world < 2 ||
      world > 15 || rank >= world || tlc > 1 || links > 1 || tail > 1 || unfused > 1 || next_gidx > (1ull << 20) ||
      aft > kMaxAft || path > (first ? 1u : 2u))
    return bad("insert: up to 2^17 parents and records (not both 0), level 1 to 2^20 - 1, world 2 to 15, rank below "
               "it");
  if ((links && !tc) || (tlc && (first || !links)) || (unfused && (first || path)) || (first && tlc))
    return bad("insert: links need the tile counts, TLC order needs links and kind 6, unfused is path 0's");
  if (nslots < 2 || nslots > (1ull << 24) || ntable != (c8 ? nslots : 2 * nslots) || (c8 && (nslots & 1)))
    return bad("insert: a table of 2 to 2^24 slots (even for the compact table), 2 words a slot (compact: 1)");
  if (na != n * W + (tlc ? n : 0) || (na && !a) || nb != nrec * (W + 1) || (nb && !b))
    return bad("insert: a of n_local states (TLC: and gpos), b of nrec records");
  const uint64_t words = LW / 32 + 1;
  if (tlc && (LW == 0 || LW > (1ull << 24))) return bad("insert: TLC order needs the level's width, 1 to 2^24");
  uint64_t succ = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const State s = state_of<M>(a + i * W);
    if (!in_domain<M>(s)) return bad("insert: a parent is not a packed state of the model");
    succ += (uint64_t)std::min<int>(M::plan(s, f).total, M::MAXSUCC);
    if (tlc && (a[n * W + i] >= LW || (i && a[n * W + i] <= a[n * W + i - 1])))
      return bad("insert: gpos strictly increasing and below W");
  }
  std::vector<uint64_t> raw;
  KC_TRY(pack_records<M>(b, nrec, raw));
  for (uint64_t r = 0; r < nrec; ++r) {
    const uint64_t key = b[r * (W + 1) + W];
    if ((key >> 60) >= world || (key >> 60) == rank)
      return bad("insert: a record's sender is another rank below world");
    if (tlc && ((key >> 16) & 0xffffffffull) >= LW) return bad("insert: a record's parent G at or past W");
  }
  uint64_t used = 0;
  for (uint64_t i = 0; i < nslots; ++i) {
    const uint64_t fp = c8 ? table[i] : table[2 * i];
    if (fp) ++used;
    else if (!c8 && table[2 * i + 1]) return bad("insert: a claim word in an empty slot of the table image");
    if (fp && !c8 && tlc) {
      const uint64_t claim = ~table[2 * i + 1];
      if ((claim >> CLAIM_KEY_BITS) == level && ((claim & ((1ull << CLAIM_KEY_BITS) - 1)) >> 12) >= 32 * words)
        return bad("insert: a same-level claim's G outside the level's bitmap");
    }
  }
  if (used + succ + nrec + 1 > nslots) return bad("insert: nslots too small: stored + successors + records + 1");
  const uint64_t tiles = (n + CLAIM_TILE - 1) / CLAIM_TILE, rgrid = (nrec + 255) / 256;
  const unsigned lt = n ? (unsigned)tiles : 0u, rb = nrec ? (unsigned)rgrid : 0u;
  const uint64_t bound = succ + nrec, cells = (uint64_t)lt + rb;
  const uint64_t need[INS_NSEC] = {n, nrec, nrec, nrec, tc ? cells + 8 : 0, tc ? cells + 8 : 0, tc ? 0 : n,
                                   tc ? 0 : nrec, links ? 0 : bound * W, links ? bound : 0, next_gidx + bound + 1};
  uint64_t at[INS_NSEC + 1];
  if (!layout(need, INS_NSEC, aft, nout, at)) return bad("insert: out of 11 sections");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  auto len = [&](int k) { return FORE + need[k] + aft; };
  Section<uint32_t> newmask, isnew, wtot, woff, offsets, ioff;
  Section<unsigned long long> rfp, link, pkeys;
  Section<unsigned int> flag;
  Section<uint64_t> next;
  KC_TRY(newmask.up(out + at[0], len(0)));
  KC_TRY(rfp.up(out + at[1], len(1)));
  KC_TRY(flag.up(out + at[2], len(2)));
  KC_TRY(isnew.up(out + at[3], len(3)));
  KC_TRY(wtot.up(out + at[4], len(4)));
  KC_TRY(woff.up(out + at[5], len(5)));
  KC_TRY(offsets.up(out + at[6], len(6)));
  KC_TRY(ioff.up(out + at[7], len(7)));
  KC_TRY(next.up(out + at[8], len(8)));
  KC_TRY(link.up(out + at[9], len(9)));
  KC_TRY(pkeys.up(out + at[10], len(10)));
  DevClaimSet cs;
  cs.compact = c8;
  cs.nslots = nslots;
  KC_TRY(cs.t.alloc(cs.units(nslots)));
  KC_HIP_TRY(hipMemcpy(cs.t.p, table, ntable * 8, hipMemcpyHostToDevice));
  DevBuf cur, in, ctr, rcount, rec_fp, rec_lk, ovf_cnt, ovf_fp, ovf_lk, ovf_tile, stage_cur, repmask, cnt, gpos, gbits,
      grank, tmp, tmp2;
  PinnedArray<unsigned long long> head;
  KC_TRY(head.alloc(10));
  for (int k = 0; k < 10; ++k) head.p[k] = 0xA5A5A5A5A5A5A5A5ull;
  KC_TRY(upload(cur, a, n * W * 8));
  KC_TRY(upload(in, raw.data(), raw.size() * 8));
  KC_TRY(ctr.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(ctr.p, 0, sizeof(Counters)));
  const uint64_t ocap = std::max<uint64_t>(succ, 1), t1 = std::max<uint64_t>(tiles, 1);
  KC_TRY(rcount.alloc(t1 * 4));
  KC_HIP_TRY(hipMemset(rcount.p, 0, t1 * 4));
  KC_TRY(rec_fp.alloc(t1 * CLAIM_RCAP * 8));
  KC_TRY(rec_lk.alloc(t1 * CLAIM_RCAP * 4));
  KC_TRY(ovf_cnt.alloc(8));
  KC_TRY(stage_cur.alloc(8));
  KC_TRY(ovf_fp.alloc(ocap * 8));
  KC_TRY(ovf_lk.alloc(ocap * 4));
  KC_TRY(ovf_tile.alloc(ocap * 4));
  KC_TRY(repmask.alloc(std::max<uint64_t>(n, 1) * 4));
  KC_TRY(cnt.alloc(std::max<uint64_t>(n, 1) * world));
  const CandOvf ovf{ovf_cnt.as<unsigned long long>(), ovf_fp.as<unsigned long long>(), ovf_lk.as<unsigned int>(),
                    ovf_tile.as<unsigned int>(), ocap};
  ClaimKeys ck((uint32_t)rank);
  if (tlc) {
    // the level's G -> local index map, as ShardT::init builds level 1's
    std::vector<uint32_t> g(std::max<uint64_t>(n, 1), 0), bits(words, 0), brank(words, 0);
    for (uint64_t i = 0; i < n; ++i) {
      g[i] = (uint32_t)a[n * W + i];
      bits[g[i] >> 5] |= 1u << (g[i] & 31);
    }
    for (uint64_t w = 1; w < words; ++w) brank[w] = brank[w - 1] + (uint32_t)__builtin_popcount(bits[w - 1]);
    KC_TRY(upload(gpos, g.data(), g.size() * 4));
    KC_TRY(upload(gbits, bits.data(), words * 4));
    KC_TRY(upload(grank, brank.data(), words * 4));
    ck.gpos = gpos.as<const uint32_t>();
    ck.gbits = gbits.as<const uint32_t>();
    ck.grank = grank.as<const uint32_t>();
  }
  Counters* const C = ctr.as<Counters>();
  const Record<M>* const rin = in.as<const Record<M>>();
  const uint32_t lv = (uint32_t)level;
  const ClaimBufs bufs{nullptr, rcount.as<unsigned int>(), rec_fp.as<unsigned long long>(), rec_lk.as<unsigned int>(),
                       newmask.ptr(), C};
  // ShardT::expand_dev
  hipLaunchKernelGGL(k_head_reset, dim3(1), dim3(64), 0, nullptr, C, ovf_cnt.as<unsigned long long>(),
                     stage_cur.as<unsigned long long>());
  if (n) {
    ShardArgs sa;
    sa.world = (uint32_t)world;
    sa.rank = (uint32_t)rank;
    sa.repmask = repmask.as<uint32_t>();
    sa.cnt = cnt.as<uint8_t>();
    sa.ovf = ovf;
    if (tlc) sa.gpos = ck.gpos;
    if (first) sa.ttot = wtot.ptr();
    const State* dcur = cur.as<const State>();
    if (first && c8)
      selftest::launch_shard_claim<M, false, true, true>((unsigned)tiles, dcur, n, f, 0, cs, lv, bufs, sa);
    else if (first)
      selftest::launch_shard_claim<M, false, true, false>((unsigned)tiles, dcur, n, f, 0, cs, lv, bufs, sa);
    else if (tlc)
      selftest::launch_shard_claim<M, true>((unsigned)tiles, dcur, n, f, 0, cs, lv, bufs, sa);
    else
      selftest::launch_shard_claim<M>((unsigned)tiles, dcur, n, f, 0, cs, lv, bufs, sa);
  }
  KC_HIP_TRY(hipGetLastError());
  // ShardT::insert
  if (first) {
    if (nrec)
      hipLaunchKernelGGL(k_rec_claim_first<M>, dim3((unsigned)rgrid), dim3(256), 0, nullptr, rin, nrec, cs.t.p,
                         cs.nslots, isnew.ptr(), wtot.ptr() + lt, C, cs.compact ? 1 : 0);
    hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, wtot.ptr(), lt, rb, woff.ptr(), C);
  } else {
    if (nrec)
      hipLaunchKernelGGL(k_rec_claim<M>, dim3((unsigned)rgrid), dim3(256), 0, nullptr, rin, nrec, cs.t.p, cs.nslots, lv,
                         rfp.ptr(), flag.ptr(), C, (int)tlc);
    const unsigned ob = n ? SHARD_OVF_BLOCKS : 0u;
    auto settle = [&](int pass, unsigned ob_blocks, uint32_t* wt) {
      const unsigned g = std::max(lt + rb + ob_blocks, 1u);
      if (pass == 0)
        hipLaunchKernelGGL((k_settle_both<M, 0>), dim3(g), dim3(256), 0, nullptr, lt, rb, n, cs.t.p, cs.nslots, lv, ck,
                           bufs.rcount, bufs.rec_fp, bufs.rec_lk, bufs.newmask, rin, nrec, rfp.ptr(), flag.ptr(),
                           isnew.ptr(), C, ovf, wt);
      else
        hipLaunchKernelGGL((k_settle_both<M, 1>), dim3(g), dim3(256), 0, nullptr, lt, rb, n, cs.t.p, cs.nslots, lv, ck,
                           bufs.rcount, bufs.rec_fp, bufs.rec_lk, bufs.newmask, rin, nrec, rfp.ptr(), flag.ptr(),
                           isnew.ptr(), C, ovf, wt);
    };
    settle(0, ob, (uint32_t*)nullptr);
    if (tc) {
      if (lt + rb) settle(1, 0, wtot.ptr());
      if (n && n <= FUSE_OVF_SCAN_MAX && !unfused) {
        hipLaunchKernelGGL(k_ovf_win_scan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, ovf, n, cs.t.p, cs.nslots, lv,
                           bufs.newmask, C, ck, wtot.ptr(), lt, rb, woff.ptr());
      } else {
        if (n)
          hipLaunchKernelGGL(k_settle_ovf<1>, dim3(SHARD_OVF_BLOCKS), dim3(256), 0, nullptr, ovf, n, (uint64_t)0,
                             cs.t.p, cs.nslots, lv, bufs.newmask, C, ck, wtot.ptr());
        hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, wtot.ptr(), lt, rb, woff.ptr(), C);
      }
    } else {
      settle(1, ob, (uint32_t*)nullptr);
      // ShardT::scan_winners
      if (path == 1) {
        hipLaunchKernelGGL(k_shard_scan_small, dim3(1), dim3(1024), 0, nullptr, bufs.newmask, n, offsets.ptr(),
                           isnew.ptr(), nrec, ioff.ptr(), C);
      } else {
        if (n) {
          const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> newcnt(bufs.newmask, NewCount());
          KC_TRY(exclusive_sum(newcnt, offsets.ptr(), n, tmp));
        }
        if (nrec) KC_TRY(exclusive_sum(isnew.ptr(), ioff.ptr(), nrec, tmp2));
        hipLaunchKernelGGL(k_shard_base, dim3(1), dim3(64), 0, nullptr, offsets.ptr(), bufs.newmask, n, ioff.ptr(),
                           isnew.ptr(), nrec, C);
      }
    }
  }
  KC_HIP_TRY(hipGetLastError());
  // ShardT::insert_emit
  const unsigned lb = (unsigned)((n + 255) / 256), eg = std::max(lb + (nrec ? (unsigned)rgrid : 0u), 1u);
  State* const nx = reinterpret_cast<State*>(next.ptr());
  auto emit = [&](uint64_t c) {
    if (links)
      hipLaunchKernelGGL(k_shard_emit_links<M>, dim3(eg), dim3(256), 0, nullptr, n, lb, rank,
                         tlc ? ck.gpos : (const uint32_t*)nullptr, bufs.newmask, rin, nrec, isnew.ptr(), woff.ptr(),
                         link.ptr(), pkeys.ptr(), next_gidx, c, C, head.p, (int)tail);
    else
      hipLaunchKernelGGL(k_shard_emit<M>, dim3(eg), dim3(256), 0, nullptr, cur.as<const State>(), n, lb, f, rank,
                         bufs.newmask, offsets.ptr(), rin, nrec, isnew.ptr(), ioff.ptr(), nx, pkeys.ptr(), next_gidx,
                         C, head.p, (int)tail, tc ? woff.ptr() : (const uint32_t*)nullptr);
    if (!tail) hipLaunchKernelGGL(k_shard_cand, dim3(1), dim3(64), 0, nullptr, C, head.p);
  };
  // (a cap past the sections' room would let a wrong position out of them)
  emit(links ? std::min(cap, bound) : 0);
  KC_TRY(sync_launch());
  std::vector<Counters> hc(1);
  KC_HIP_TRY(hipMemcpy(hc.data(), ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
  res[7] = hc[0].defer_flags;
  if (links && cap2 && (head.p[7] & DF_CAPACITY)) {
    KC_HIP_TRY(hipMemsetAsync(&C->defer_flags, 0, 8, nullptr));
    emit(std::min(cap2, bound));
    KC_TRY(sync_launch());
    KC_HIP_TRY(hipMemcpy(hc.data(), ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
  }
  KC_TRY(newmask.down(out + at[0]));
  KC_TRY(rfp.down(out + at[1]));
  KC_TRY(flag.down(out + at[2]));
  KC_TRY(isnew.down(out + at[3]));
  KC_TRY(wtot.down(out + at[4]));
  KC_TRY(woff.down(out + at[5]));
  KC_TRY(offsets.down(out + at[6]));
  KC_TRY(ioff.down(out + at[7]));
  KC_TRY(next.down(out + at[8]));
  KC_TRY(link.down(out + at[9]));
  KC_TRY(pkeys.down(out + at[10]));
  KC_HIP_TRY(hipMemcpy(table, cs.t.p, ntable * 8, hipMemcpyDeviceToHost));
  const Counters& h = hc[0];
  res[0] = h.err_key;
  res[1] = h.overflow;
  res[2] = h.probes();
  res[3] = h.chunk_base;
  res[4] = h.level_new;
  res[5] = h.cand_total;
  res[6] = h.defer_flags;
  for (int k = 0; k < A_COUNT; ++k) res[8 + k] = h.act_dist(k);
  for (int k = 0; k < 10; ++k) res[8 + A_COUNT + k] = head.p[k];
  return 0;
}

template <class M>
int run_model(int kind, const kc_model_config& cfg, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na,
              const uint64_t* b, uint64_t nb, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  const Flags f = flags_of(cfg);
  switch (kind) {
    case 1:
      return run_gather<M>(par, npar, a, na, b, nb, out, nout);
    case 3:
      return run_pack<M>(f, par, npar, a, na, b, nb, out, nout, res, nres);
    case 4:
      return run_shard_materialize<M>(f, par, npar, a, na, b, nb, out, nout, res, nres);
    default:
      return run_undo<M>(f, par, npar, a, na, b, nb, res, nres);
  }
}

}  // namespace
}  // namespace kc

extern "C" int kc_shard_selftest(int kind, const kc_model_config* cfg, const uint64_t* par, uint64_t npar,
                                 const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* table,
                                 uint64_t ntable, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  using namespace kc;
  if (kind < 0 || kind > 7) return bad("kind 0-7");
  if (kind < 6 && (table || ntable)) return bad("a table belongs to kinds 6 and 7");
  if (kind == 0) return run_owner_scan(par, npar, a, na, b, nb, out, nout, res, nres);
  if (kind == 2) return run_tlc(par, npar, a, na, b, nb, out, nout, res, nres);
  if (!cfg || cfg->nc != 1 || cfg->ns != 1 || (cfg->np != 1 && cfg->np != 2))
    return bad("a model config with nc = ns = 1 and np 1 or 2");
  if (kind >= 6) {
    const bool first = kind == 7;
    return cfg->np == 1
               ? run_insert<Model<1, 1, 1>>(first, *cfg, par, npar, a, na, b, nb, table, ntable, out, nout, res, nres)
               : run_insert<Model<1, 2, 1>>(first, *cfg, par, npar, a, na, b, nb, table, ntable, out, nout, res, nres);
  }
  return cfg->np == 1 ? run_model<Model<1, 1, 1>>(kind, *cfg, par, npar, a, na, b, nb, out, nout, res, nres)
                      : run_model<Model<1, 2, 1>>(kind, *cfg, par, npar, a, na, b, nb, out, nout, res, nres);
}
