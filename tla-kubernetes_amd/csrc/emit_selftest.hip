// emit_selftest.hip — test-only device harness for the kernels that turn a
// wide level's newmask words into the next frontier (engine_kernels.h):
// kc_emit_selftest runs one of k_tile_scan / k_chunk_scan, tile_scan_body with
// ScanMarks, k_emit_links, k_emit<M>, k_materialize<M>, k_parent_chain and
// spread_tile on inputs of the suite's making, with the engine's grids and
// block sizes, for Model<1,1,1> and Model<1,2,1>.  tests/test_gpu_scan_emit.py
// compares the results with tests/emit_model.py and the host Spec.
//
// Outputs travel as u64 words, one per element whatever the kernel's element
// type.  Every output section is uploaded as the caller filled it and copied
// back whole: KC_EMIT_FORE guard elements, then the kernel's array (the
// kernel's pointer is section + KC_EMIT_FORE elements), then the caller's aft
// guards.  The harness checks, on the host and before any launch, everything
// a kernel's indices depend on (so a machine without a GPU answers -EINVAL to
// bad input and -ENODEV only to good input), and sizes every section for the
// worst case the input allows (see each kind), so no input reaches a kernel
// with a buffer it could overrun.  Nothing of the product path calls this
// file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/kubecheck.h"
#include "engine_kernels.h"
#include "engine_util.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "selftest_util.h"

namespace kc {
namespace {

using selftest::DevBuf;
using selftest::upload;

constexpr uint64_t FORE = KC_EMIT_FORE;
constexpr uint64_t kEmitTestMax = 1ull << 24;   // elements of a section
constexpr uint32_t MARK_GUARD = 0xA5A5A5A5u;

int bad(const char* what) {
  set_error("kc_emit_selftest: %s", what);
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

template <class T>
int upload_as(DevBuf& d, const uint64_t* src, uint64_t n, uint64_t pad = 0, T padv = T()) {
  std::vector<T> h(n + pad, padv);
  for (uint64_t i = 0; i < n; ++i) h[i] = (T)src[i];
  return upload(d, h.data(), (n + pad) * sizeof(T));
}

int need_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_emit_selftest: no HIP device");
    return -ENODEV;
  }
  return 0;
}

int sync_launch() {
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  return 0;
}

// Counters with err_key = ~0 (none) and the chunk's base.
int make_counters(DevBuf& c, uint64_t chunk_base) {
  KC_TRY(c.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(c.p, 0, sizeof(Counters)));
  unsigned long long head[2] = {~0ull, chunk_base};
  KC_HIP_TRY(hipMemcpy(c.p, head, sizeof(head), hipMemcpyHostToDevice));
  return 0;
}
int read_counters(const DevBuf& c, Counters& h) {
  KC_HIP_TRY(hipMemcpy(&h, c.p, sizeof(Counters), hipMemcpyDeviceToHost));
  return 0;
}

// ---------------------------------------------------------------- scan, marks
__global__ void __launch_bounds__(TSCAN_THREADS)
k_scan_marks(const uint32_t* __restrict__ tot, uint32_t T, uint32_t* __restrict__ off, int reg_ok, ScanMarks mk,
             uint32_t* __restrict__ marks_out) {
  __shared__ unsigned int sh_mark[17];
  if (threadIdx.x < 17) sh_mark[threadIdx.x] = MARK_GUARD;
  __syncthreads();
  tile_scan_body(tot, T, off, reg_ok, mk, sh_mark);
  if (threadIdx.x < 17) marks_out[threadIdx.x] = sh_mark[threadIdx.x];
}

// kinds 0 and 1.  par = [T, reg_ok, chunk] or [T, reg_ok, stride, nmark,
// extra]; a = the 4 * ceil(T / 4) cells the scan loads (the pad cells are the
// caller's garbage; the first T sum below 2^32); out = off, at least
// max(4 * ceil(T / 4), T + 1) cells behind the fore guards.  kind 0: res = the
// na input cells after the launch (k_chunk_scan zeroes the first T).  kind 1:
// res = sh_mark[0 .. 16], which starts as 0xA5A5A5A5.
int run_scan(bool marks, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, uint64_t* out,
             uint64_t nout, uint64_t* res, uint64_t nres) {
  if (!par || npar != (marks ? 5u : 3u) || !a || !out || !res) return bad("scan: par, a, out and res");
  const uint64_t T = par[0];
  if (T == 0 || T > (1ull << 22) || par[1] > 1) return bad("scan: 1 to 2^22 cells, reg_ok 0 or 1");
  const uint64_t G = (T + 3) / 4;
  if (na != 4 * G) return bad("scan: a holds 4 * ceil(T / 4) cells");
  uint64_t sum = 0;
  for (uint64_t i = 0; i < na; ++i) {
    if (a[i] >> 32) return bad("scan: a cell over 32 bits");
    if (i < T) sum += a[i];
  }
  if (sum >> 32) return bad("scan: the total does not fit 32 bits");
  if (nout > kEmitTestMax || nout < FORE + std::max(4 * G, T + 1)) return bad("scan: off is too small");
  ScanMarks mk;
  if (marks) {
    if (par[2] >> 32 || par[3] > 16 || par[4] >> 32 || nres != 17) return bad("marks: nmark <= 16, res of 17 words");
    mk = ScanMarks{(uint32_t)par[2], (uint32_t)par[3], (uint32_t)par[4]};
  } else if (par[2] > 1 || nres != na) {
    return bad("scan: chunk 0 or 1, res of na words");
  }
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf tot;
  Section<uint32_t> off, mo;
  KC_TRY(upload_as<uint32_t>(tot, a, na));
  KC_TRY(off.up(out, nout));
  if (marks) {
    const uint64_t zero[17 + FORE] = {};
    KC_TRY(mo.up(zero, 17 + FORE));
    hipLaunchKernelGGL(k_scan_marks, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, tot.as<const uint32_t>(), (uint32_t)T,
                       off.ptr(), (int)par[1], mk, mo.ptr());
  } else if (par[2]) {
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, tot.as<uint32_t>(), (uint32_t)T,
                       off.ptr(), (int)par[1]);
  } else {
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(TSCAN_THREADS), 0, nullptr, tot.as<const uint32_t>(), (uint32_t)T,
                       off.ptr(), (int)par[1]);
  }
  KC_TRY(sync_launch());
  KC_TRY(off.down(out));
  if (marks) {
    uint64_t m[17 + FORE];
    KC_TRY(mo.down(m));
    for (int i = 0; i < 17; ++i) res[i] = m[FORE + i];
  } else {
    std::vector<uint32_t> h(na);
    KC_HIP_TRY(hipMemcpy(h.data(), tot.p, na * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < na; ++i) res[i] = h[i];
  }
  return 0;
}

// ------------------------------------------------------------------ link emit
// The masks' tile counts and their exclusive sums.
struct TileSums {
  std::vector<uint32_t> ttot, toff;   // [T], [T + 1]
  uint64_t total = 0;
};
int tile_sums(const uint64_t* mask, uint64_t n, TileSums& ts) {
  const uint64_t T = (n + 255) / 256;
  ts.ttot.assign(T, 0);
  ts.toff.assign(T + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (mask[i] >> 32) return bad("a newmask word over 32 bits");
    ts.ttot[i / 256] += (uint32_t)__builtin_popcountll(mask[i]);
  }
  for (uint64_t t = 0; t < T; ++t) {
    ts.toff[t] = (uint32_t)ts.total;
    ts.total += ts.ttot[t];
  }
  if (ts.total >> 32) return bad("more than 2^32 new states");
  ts.toff[T] = (uint32_t)ts.total;
  return 0;
}

// kind 2.  par = [n, base, level_gidx, next_gidx, cap, chunk_base, mode,
// want_link, want_trace, seclen]; a = newmask[n]; b = the offsets, which the
// harness recomputes: mode 0 tile_off[T + 1] (k_tile_scan's output), mode 1
// coff[C + 1] (k_chunk_scan's, C = ceil(T / 64)) then ttot[T].  out = link,
// parent, ord: three sections of seclen elements, each at least fore guards +
// next_gidx + chunk_base + total + 1 (every entry and one more, whatever cap
// says).  res = [defer_flags, outdeg[16]].  ttot is rounded up as the engine
// rounds it (T + 4 cells; the pad cells hold 0xA5A5A5A5).
int run_emit_links(const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb,
                   uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  if (!par || npar != 10 || !a || !b || !out || !res) return bad("emit_links: par, a, b, out and res");
  const uint64_t n = par[0], base = par[1], level_gidx = par[2], next_gidx = par[3], cap = par[4], cb = par[5];
  const uint64_t mode = par[6], seclen = par[9];
  if (n == 0 || n > (1ull << 20) || na != n || mode > 1 || par[7] > 1 || par[8] > 1)
    return bad("emit_links: 1 to 2^20 parents, one newmask word each, mode and switches 0 or 1");
  if (base >> 47 || level_gidx >> 47 || next_gidx > (1ull << 20) || cb > (1ull << 20))
    return bad("emit_links: base, level_gidx below 2^47; next_gidx, chunk_base up to 2^20");
  TileSums ts;
  KC_TRY(tile_sums(a, n, ts));
  const uint64_t T = ts.ttot.size(), C = (T + CSUM_TILES - 1) / CSUM_TILES;
  std::vector<uint32_t> offs;
  if (mode == 0) {
    if (nb != T + 1) return bad("emit_links: tile_off holds T + 1 cells");
    offs = ts.toff;
  } else {
    if (nb != C + 1 + T) return bad("emit_links: coff holds C + 1 cells, then ttot T");
    for (uint64_t c = 0; c <= C; ++c) offs.push_back(ts.toff[std::min(c * CSUM_TILES, T)]);
    for (uint64_t t = 0; t < T; ++t)
      if (b[C + 1 + t] != ts.ttot[t]) return bad("emit_links: ttot is not the tiles' new-state count");
  }
  for (uint64_t k = 0; k < offs.size(); ++k)
    if (b[k] != offs[k]) return bad("emit_links: the offsets are not the exclusive sums of the masks");
  if (seclen > kEmitTestMax || nout != 3 * seclen || seclen < FORE + next_gidx + cb + ts.total + 1 || nres != 17)
    return bad("emit_links: three sections of fore + next_gidx + chunk_base + total + 1 elements at least");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf nm, to, tt, ctr;
  Section<unsigned long long> link, parent;
  Section<uint8_t> ord;
  KC_TRY(upload_as<uint32_t>(nm, a, n));
  KC_TRY(upload(to, offs.data(), offs.size() * 4));
  KC_TRY(upload_as<uint32_t>(tt, b + (mode ? C + 1 : 0), mode ? T : 0, 4, MARK_GUARD));
  KC_TRY(link.up(out, seclen));
  KC_TRY(parent.up(out + seclen, seclen));
  KC_TRY(ord.up(out + 2 * seclen, seclen));
  KC_TRY(make_counters(ctr, cb));
  hipLaunchKernelGGL(k_emit_links, dim3((unsigned)((T + EMIT_TPB - 1) / EMIT_TPB)), dim3(256), 0, nullptr, n, base,
                     nm.as<const uint32_t>(), to.as<const uint32_t>(), level_gidx, next_gidx,
                     par[8] ? parent.ptr() : nullptr, par[8] ? ord.ptr() : nullptr, par[7] ? link.ptr() : nullptr, cap,
                     ctr.as<Counters>(), mode ? tt.as<const uint32_t>() : (const uint32_t*)nullptr);
  KC_TRY(sync_launch());
  KC_TRY(link.down(out));
  KC_TRY(parent.down(out + seclen));
  KC_TRY(ord.down(out + 2 * seclen));
  Counters h;
  KC_TRY(read_counters(ctr, h));
  res[0] = h.defer_flags;
  for (int k = 0; k < OUTDEG_BINS; ++k) res[1 + k] = h.outdeg(k);
  return 0;
}

// ------------------------------------------------------------------------ emit
template <class M>
int check_parents(const uint64_t* packed, uint64_t n, const Flags& f, std::vector<int>& tot) {
  const char* why = selftest::check_states<M>(packed, n, f, tot);
  return why ? bad(why) : 0;
}

// kind 3.  par = [n, base, next_base, chunk_base, level_gidx, next_gidx,
// keep_trace, mode, seclen_next, seclen_trace]; a = n packed parents of the
// model under cfg; b = newmask[n], bits below each parent's successor count.
// mode 0: tile offsets (the harness's own exclusive sums of the masks), mode 1:
// per-parent offsets.  out = next (seclen_next states: fore guard states +
// chunk_base - next_base + total at least), then parent and ord (seclen_trace
// elements: fore + next_gidx + chunk_base + total at least).  res = [err_key,
// next_cand, act_dist[A_COUNT], outdeg[16]].
template <class M>
int run_emit(const Flags& f, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b,
             uint64_t nb, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  if (!par || npar != 10 || !a || !b || !out || !res) return bad("emit: par, a, b, out and res");
  const uint64_t n = par[0], base = par[1], next_base = par[2], cb = par[3], level_gidx = par[4], next_gidx = par[5];
  const uint64_t mode = par[7], sn = par[8], st = par[9];
  if (n == 0 || n > (1ull << 20) || na != n * M::W || nb != n || par[6] > 1 || mode > 1)
    return bad("emit: 1 to 2^20 parents, one newmask word each, keep_trace and mode 0 or 1");
  if (base >> 40 || level_gidx >> 47 || next_gidx > (1ull << 20) || cb > (1ull << 20) || next_base > cb)
    return bad("emit: base below 2^40, level_gidx below 2^47; next_gidx, chunk_base up to 2^20; next_base <= "
               "chunk_base");
  std::vector<int> tot;
  KC_TRY(check_parents<M>(a, n, f, tot));
  TileSums ts;
  KC_TRY(tile_sums(b, n, ts));
  std::vector<uint32_t> poff(n);
  uint64_t run = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (b[i] >> tot[i]) return bad("emit: a newmask bit at or past the parent's successor count");
    poff[i] = (uint32_t)run;
    run += (uint64_t)__builtin_popcountll(b[i]);
  }
  if (sn > kEmitTestMax / M::W || st > kEmitTestMax || nout != sn * M::W + 2 * st ||
      sn < FORE + cb - next_base + ts.total || st < FORE + next_gidx + cb + ts.total ||
      nres != 2 + (uint64_t)A_COUNT + OUTDEG_BINS)
    return bad("emit: next of fore + chunk_base - next_base + total states, parent and ord of fore + next_gidx + "
               "chunk_base + total elements at least");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf cur, nm, po, to, ctr;
  Section<uint64_t> next;
  Section<unsigned long long> parent;
  Section<uint8_t> ord;
  KC_TRY(upload(cur, a, na * 8));
  KC_TRY(upload_as<uint32_t>(nm, b, n));
  KC_TRY(upload(po, poff.data(), n * 4));
  KC_TRY(upload(to, ts.toff.data(), ts.toff.size() * 4));
  KC_TRY(next.up(out, sn * M::W));
  KC_TRY(parent.up(out + sn * M::W, st));
  KC_TRY(ord.up(out + sn * M::W + st, st));
  KC_TRY(make_counters(ctr, cb));
  typename M::State* nx = reinterpret_cast<typename M::State*>(next.d.as<uint64_t>()) + FORE;
  hipLaunchKernelGGL((k_emit<M, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     cur.as<const typename M::State>(), n, base, f, nm.as<const uint32_t>(), po.as<const uint32_t>(),
                     nx, next_base, level_gidx, next_gidx, parent.ptr(), ord.ptr(), (int)par[6], ctr.as<Counters>(),
                     mode ? (const uint32_t*)nullptr : to.as<const uint32_t>());
  KC_TRY(sync_launch());
  KC_TRY(next.down(out));
  KC_TRY(parent.down(out + sn * M::W));
  KC_TRY(ord.down(out + sn * M::W + st));
  Counters h;
  KC_TRY(read_counters(ctr, h));
  res[0] = h.err_key;
  res[1] = h.next_cand();
  for (int k = 0; k < A_COUNT; ++k) res[2 + k] = h.act_dist(k);
  for (int k = 0; k < OUTDEG_BINS; ++k) res[2 + A_COUNT + k] = h.outdeg(k);
  return 0;
}

// ----------------------------------------------------------------- materialise
// kind 4.  par = [n, nprev, mode, gidx0, prev_gidx0, prev_counts]; a = nprev
// packed states of the previous frontier; b = mode 0: link[n] (parent index <<
// 8 | position), mode 1: parent[n] then ord[n] (global parent indices; the
// kernel reads them at gidx0 + i, behind gidx0 cells of ~0 / 0xff).  Every
// parent index is below nprev and every position below that parent's successor
// count.  prev_counts 1: the rebuild takes the plans from an array (M::plan of
// each previous state), 0: it plans them itself.  out = n states behind fore
// guard states.  res = [defer_flags, defer_inv_n, next_cand, act_dist[A_COUNT]].
template <class M>
int run_materialize(const Flags& f, const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na,
                    const uint64_t* b, uint64_t nb, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  if (!par || npar != 6 || !a || !b || !out || !res) return bad("materialize: par, a, b, out and res");
  const uint64_t n = par[0], nprev = par[1], mode = par[2], gidx0 = par[3], prev_gidx0 = par[4];
  if (n == 0 || n > (1ull << 20) || nprev == 0 || nprev > (1ull << 20) || na != nprev * M::W || mode > 1 ||
      par[5] > 1 || nb != (mode ? 2 * n : n) || gidx0 > (1ull << 20) || prev_gidx0 >> 47)
    return bad("materialize: 1 to 2^20 states and previous states, mode and prev_counts 0 or 1, gidx0 up to 2^20");
  std::vector<int> tot;
  KC_TRY(check_parents<M>(a, nprev, f, tot));
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t pp, t;
    if (mode == 0) {
      pp = b[i] >> 8;
      t = b[i] & 0xff;
    } else {
      if (b[i] < prev_gidx0) return bad("materialize: a parent below prev_gidx0");
      pp = b[i] - prev_gidx0;
      t = b[n + i];
    }
    if (pp >= nprev) return bad("materialize: a parent index outside the previous frontier");
    if (t >= (uint64_t)tot[pp]) return bad("materialize: a position at or past the parent's successor count");
  }
  if (nout > kEmitTestMax || nout % M::W || nout / M::W < FORE + n || nres != 3 + (uint64_t)A_COUNT)
    return bad("materialize: out of fore + n states at least");
  std::vector<unsigned long long> counts(nprev);
  for (uint64_t i = 0; i < nprev; ++i) {
    typename M::State s;
    for (int k = 0; k < M::W; ++k) s.w[k] = a[i * M::W + k];
    counts[i] = M::plan(s, f).counts;
  }
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf prev, lk, pa, od, pc, ctr;
  Section<uint64_t> o;
  KC_TRY(upload(prev, a, na * 8));
  if (mode == 0) {
    KC_TRY(upload(lk, b, n * 8));
  } else {
    std::vector<unsigned long long> hp(gidx0 + n, ~0ull);
    std::vector<uint8_t> ho(gidx0 + n, 0xff);
    for (uint64_t i = 0; i < n; ++i) {
      hp[gidx0 + i] = b[i];
      ho[gidx0 + i] = (uint8_t)b[n + i];
    }
    KC_TRY(upload(pa, hp.data(), hp.size() * 8));
    KC_TRY(upload(od, ho.data(), ho.size()));
  }
  KC_TRY(upload(pc, counts.data(), nprev * 8));
  KC_TRY(o.up(out, nout));
  KC_TRY(make_counters(ctr, 0));
  DeferArgs df;
  df.prev = prev.p;
  if (mode == 0) {
    df.link = lk.as<const unsigned long long>();
  } else {
    df.parent = pa.as<const unsigned long long>();
    df.ord = od.as<const uint8_t>();
    df.gidx0 = gidx0;
    df.prev_gidx0 = prev_gidx0;
  }
  df.out = reinterpret_cast<typename M::State*>(o.d.as<uint64_t>()) + FORE;
  if (par[5]) df.prev_counts = pc.as<const unsigned long long>();
  hipLaunchKernelGGL(k_materialize<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, df, n, f,
                     ctr.as<Counters>());
  KC_TRY(sync_launch());
  KC_TRY(o.down(out));
  Counters h;
  KC_TRY(read_counters(ctr, h));
  res[0] = h.defer_flags;
  res[1] = h.defer_inv_n;
  res[2] = h.next_cand();
  for (int k = 0; k < A_COUNT; ++k) res[3 + k] = h.act_dist(k);
  return 0;
}

// ---------------------------------------------------------------- parent chain
// kind 5.  par = [g, cap]; a = parent[na] (each below na, or ~0), b = ord[na]
// (bytes), g < na.  out = pinned host memory, as in the engine: fore guards,
// the length word, then cap chain words at least; uploaded as given.
int run_parent_chain(const uint64_t* par, uint64_t npar, const uint64_t* a, uint64_t na, const uint64_t* b,
                     uint64_t nb, uint64_t* out, uint64_t nout) {
  if (!par || npar != 2 || !a || !b || !out) return bad("parent_chain: par, a, b and out");
  const uint64_t g = par[0], cap = par[1];
  if (na == 0 || na > (1ull << 20) || nb != na || g >= na || cap > (1ull << 16) || nout > (1ull << 20) ||
      nout < FORE + 1 + cap)
    return bad("parent_chain: 1 to 2^20 states, g among them, cap up to 2^16, out of fore + 1 + cap words at least");
  for (uint64_t i = 0; i < na; ++i)
    if ((a[i] >= na && a[i] != ~0ull) || b[i] > 0xff) return bad("parent_chain: a parent outside the states");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  DevBuf pa, od;
  PinnedArray<uint64_t> h;
  KC_TRY(upload(pa, a, na * 8));
  KC_TRY(upload_as<uint8_t>(od, b, na));
  KC_TRY(h.alloc(nout));
  memcpy(h.p, out, nout * 8);
  hipLaunchKernelGGL(k_parent_chain, dim3(1), dim3(64), 0, nullptr, pa.as<const unsigned long long>(),
                     od.as<const uint8_t>(), g, h.p + FORE + 1, (uint32_t)cap, h.p + FORE);
  KC_TRY(sync_launch());
  memcpy(out, h.p, nout * 8);
  return 0;
}

// ---------------------------------------------------------------------- spread
__global__ void k_spread(uint32_t G, uint32_t S, uint32_t* __restrict__ out) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < G) out[b] = spread_tile(b, G, S);
}

// kind 6.  par = [G, S]; out[b] = spread_tile(b, G, S) for b < G, behind the
// fore guards.
int run_spread(const uint64_t* par, uint64_t npar, uint64_t* out, uint64_t nout) {
  if (!par || npar != 2 || !out) return bad("spread: par and out");
  if (par[0] == 0 || par[0] > (1ull << 20) || par[1] >> 32 || nout > kEmitTestMax || nout < FORE + par[0])
    return bad("spread: 1 to 2^20 workgroups, out of fore + G words at least");
  KC_TRY(need_device());   // (the input is valid: -EINVAL needs no GPU)
  Section<uint32_t> o;
  KC_TRY(o.up(out, nout));
  hipLaunchKernelGGL(k_spread, dim3((unsigned)((par[0] + 255) / 256)), dim3(256), 0, nullptr, (uint32_t)par[0],
                     (uint32_t)par[1], o.ptr());
  KC_TRY(sync_launch());
  return o.down(out);
}

}  // namespace
}  // namespace kc

extern "C" int kc_emit_selftest(int kind, const kc_model_config* cfg, const uint64_t* par, uint64_t npar,
                                const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* out,
                                uint64_t nout, uint64_t* res, uint64_t nres) {
  using namespace kc;
  if (kind < 0 || kind > 6) return bad("kind 0-6");
  const bool model = kind == 3 || kind == 4;
  if (model && (!cfg || cfg->nc != 1 || cfg->ns != 1 || (cfg->np != 1 && cfg->np != 2)))
    return bad("a model config with nc = ns = 1 and np 1 or 2");
  switch (kind) {
    case 0:
    case 1:
      return run_scan(kind == 1, par, npar, a, na, out, nout, res, nres);
    case 2:
      return run_emit_links(par, npar, a, na, b, nb, out, nout, res, nres);
    case 3:
      return cfg->np == 1 ? run_emit<Model<1, 1, 1>>(flags_of(*cfg), par, npar, a, na, b, nb, out, nout, res, nres)
                          : run_emit<Model<1, 2, 1>>(flags_of(*cfg), par, npar, a, na, b, nb, out, nout, res, nres);
    case 4:
      return cfg->np == 1
                 ? run_materialize<Model<1, 1, 1>>(flags_of(*cfg), par, npar, a, na, b, nb, out, nout, res, nres)
                 : run_materialize<Model<1, 2, 1>>(flags_of(*cfg), par, npar, a, na, b, nb, out, nout, res, nres);
    case 5:
      return run_parent_chain(par, npar, a, na, b, nb, out, nout);
    default:
      return run_spread(par, npar, out, nout);
  }
}
