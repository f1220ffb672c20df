// spill_selftest.hip — test-only device harness for the kernels that join
// the seen-set's two tiers (engine_spill.h): kc_spill_selftest runs one of
// k_claimset_keys, k_spill_queries<M>, k_spill_apply (with claimset_retire)
// and k_tile_succ<M> on inputs of the suite's making, launched as the engine
// launches them, for Model<1,1,1> and Model<1,2,1>.  tests/
// test_gpu_spill_kernels.py compares the results with the host Spec and
// tests/cold_model.py.  The harness checks, on the host and before any
// launch, everything a kernel's indices depend on (see each kind), so no
// input reaches a kernel with a buffer it could overrun.  Nothing of the
// product path calls this file.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/kubecheck.h"
#include "engine_spill.h"
#include "engine_util.h"
#include "fpset_host.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "selftest_util.h"

namespace kc {
namespace {

using selftest::DevBuf;
using selftest::upload;

constexpr uint64_t kSpillTestMax = 1ull << 20;    // slots, parents, queries

int bad(const char* what) {
  set_error("kc_spill_selftest: %s", what);
  return -EINVAL;
}

Flags test_flags() {
  kc_model_config c;
  kc_model_config_default(&c);
  return flags_of(c);
}

// (selftest_util.h check_states under the default flags)
template <class M>
int check_states(const uint64_t* packed, uint64_t n, std::vector<int>& tot) {
  const char* why = selftest::check_states<M>(packed, n, test_flags(), tot);
  return why ? bad(why) : 0;
}

// kind 0.  a = table image (2 words per slot), na = slots; out = nout >= cap
// words, uploaded as given (the guard pattern) and copied back; res[0] = count.
int run_claimset_keys(const uint64_t* a, uint64_t na, uint64_t cap, uint64_t* out, uint64_t nout, uint64_t* res) {
  // (up to 2^25 slots: past 2^24 the grid of table_grid strides)
  if (!a || !out || !res || na < 2 || na > (1ull << 25) || cap > nout || nout == 0 || nout > 2 * kSpillTestMax)
    return bad("claimset_keys: 2 to 2^25 slots, cap <= nout, 1 to 2^21 output words");
  DevBuf t, o, c;
  KC_TRY(upload(t, a, na * 16));
  KC_TRY(upload(o, out, nout * 8));
  KC_TRY(c.alloc(8));
  KC_HIP_TRY(hipMemset(c.p, 0, 8));
  hipLaunchKernelGGL(k_claimset_keys, dim3(table_grid(na)), dim3(256), 0, nullptr, t.as<const ClaimEntry>(), na,
                     o.as<uint64_t>(), cap, c.as<unsigned long long>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(out, o.p, nout * 8, hipMemcpyDeviceToHost));
  KC_HIP_TRY(hipMemcpy(res, c.p, 8, hipMemcpyDeviceToHost));
  return 0;
}

// kind 1.  a = na packed parents; b[i] = newmask of parent i (bits below its
// successor count only); c = exclusive winner sums per 256-parent tile (the
// harness recomputes them and refuses anything else); out = qkey, res = qloc,
// nout words each (>= the winners), uploaded as given and copied back.
template <class M>
int run_spill_queries(const uint64_t* a, uint64_t na, const uint64_t* b, const uint64_t* c, uint64_t nc, uint64_t* out,
                      uint64_t nout, uint64_t* res) {
  const uint64_t tiles = (na + 255) / 256;
  if (!a || !b || !c || !out || !res || na == 0 || na > kSpillTestMax || nc != tiles || nout == 0 ||
      nout > 32 * kSpillTestMax)
    return bad("spill_queries: 1 to 2^20 parents, one tile offset per 256 parents");
  std::vector<int> tot;
  KC_TRY(check_states<M>(a, na, tot));
  std::vector<uint32_t> mask(na), toff(tiles), loc(nout);
  uint64_t sum = 0;
  for (uint64_t i = 0; i < na; ++i) {
    if (i % 256 == 0) {
      if (c[i / 256] != sum) return bad("spill_queries: tile_off is not the exclusive sum of the tiles' winners");
      toff[i / 256] = (uint32_t)sum;
    }
    if (b[i] >> tot[i]) return bad("spill_queries: a newmask bit at or past the parent's successor count");
    mask[i] = (uint32_t)b[i];
    sum += (uint64_t)__builtin_popcountll(b[i]);
  }
  if (sum > nout) return bad("spill_queries: more winners than output words");
  for (uint64_t i = 0; i < nout; ++i) loc[i] = (uint32_t)res[i];
  DevBuf cur, nm, to, qk, ql;
  KC_TRY(upload(cur, a, na * M::W * 8));
  KC_TRY(upload(nm, mask.data(), na * 4));
  KC_TRY(upload(to, toff.data(), tiles * 4));
  KC_TRY(upload(qk, out, nout * 8));
  KC_TRY(upload(ql, loc.data(), nout * 4));
  hipLaunchKernelGGL(k_spill_queries<M>, dim3((unsigned)tiles), dim3(256), 0, nullptr,
                     cur.as<const typename M::State>(), na, test_flags(), nm.as<const uint32_t>(),
                     to.as<const uint32_t>(), qk.as<uint64_t>(), ql.as<uint32_t>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(out, qk.p, nout * 8, hipMemcpyDeviceToHost));
  KC_HIP_TRY(hipMemcpy(loc.data(), ql.p, nout * 4, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < nout; ++i) res[i] = loc[i];
  return 0;
}

// kind 2.  a = table image in, na = slots; b = m x {qkey, qloc, found}
// (3 words per query; qloc >> 5 < cap); c = nc parents' newmask words; cap =
// parents.  out = the table image (2 na words); res = [overflow, newmask x nc,
// tile_total x tiles].  tile_total starts at each tile's popcount of newmask,
// and every found query's newmask bit is set on entry, so no count wraps.
int run_spill_apply(const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t m, const uint64_t* c, uint64_t nc,
                    uint64_t* out, uint64_t nout, uint64_t* res) {
  const uint64_t tiles = (nc + 255) / 256;
  if (!a || !b || !c || !out || !res || na < 2 || na > kSpillTestMax || m == 0 || m > kSpillTestMax || nc == 0 ||
      nc > kSpillTestMax || nout != 2 * na)
    return bad("spill_apply: 2 to 2^20 slots, 1 to 2^20 queries and parents, nout = 2 x slots");
  std::vector<uint64_t> qk(m);
  std::vector<uint32_t> ql(m), nm(nc), tt(tiles, 0);
  std::vector<uint8_t> fd(m);
  for (uint64_t i = 0; i < nc; ++i) {
    if (c[i] >> 32) return bad("spill_apply: a newmask word over 32 bits");
    nm[i] = (uint32_t)c[i];
    tt[i / 256] += (uint32_t)__builtin_popcount(nm[i]);
  }
  std::vector<uint32_t> left = nm;
  for (uint64_t i = 0; i < m; ++i) {
    qk[i] = b[3 * i];
    const uint64_t loc = b[3 * i + 1];
    if (loc >> 32 || (loc >> 5) >= nc || b[3 * i + 2] > 1) return bad("spill_apply: qloc outside the parents");
    ql[i] = (uint32_t)loc;
    fd[i] = (uint8_t)b[3 * i + 2];
    if (fd[i]) {
      if (!((left[loc >> 5] >> (loc & 31)) & 1)) return bad("spill_apply: a found query whose newmask bit is clear");
      left[loc >> 5] &= ~(1u << (loc & 31));
    }
  }
  DevBuf t, dk, dl, df, dn, dt, ctr;
  KC_TRY(upload(t, a, na * 16));
  KC_TRY(upload(dk, qk.data(), m * 8));
  KC_TRY(upload(dl, ql.data(), m * 4));
  KC_TRY(upload(df, fd.data(), m));
  KC_TRY(upload(dn, nm.data(), nc * 4));
  KC_TRY(upload(dt, tt.data(), tiles * 4));
  KC_TRY(ctr.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(ctr.p, 0, sizeof(Counters)));
  hipLaunchKernelGGL(k_spill_apply, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, dk.as<const uint64_t>(),
                     dl.as<const uint32_t>(), df.as<const uint8_t>(), m, dn.as<uint32_t>(), dt.as<uint32_t>(),
                     t.as<ClaimEntry>(), na, ctr.as<Counters>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(out, t.p, na * 16, hipMemcpyDeviceToHost));
  KC_HIP_TRY(hipMemcpy(nm.data(), dn.p, nc * 4, hipMemcpyDeviceToHost));
  KC_HIP_TRY(hipMemcpy(tt.data(), dt.p, tiles * 4, hipMemcpyDeviceToHost));
  unsigned long long ovf = 0;
  KC_HIP_TRY(hipMemcpy(&ovf, reinterpret_cast<char*>(ctr.p) + offsetof(Counters, overflow), 8, hipMemcpyDeviceToHost));
  res[0] = ovf;
  for (uint64_t i = 0; i < nc; ++i) res[1 + i] = nm[i];
  for (uint64_t i = 0; i < tiles; ++i) res[1 + nc + i] = tt[i];
  return 0;
}

// kind 3.  a = na packed parents; res[t] = successors of tile t.
template <class M>
int run_tile_succ(const uint64_t* a, uint64_t na, uint64_t* res) {
  if (!a || !res || na == 0 || na > kSpillTestMax) return bad("tile_succ: 1 to 2^20 parents");
  std::vector<int> tot;
  KC_TRY(check_states<M>(a, na, tot));
  const uint64_t tiles = (na + 255) / 256;
  std::vector<uint32_t> ts(tiles);
  DevBuf cur, d;
  KC_TRY(upload(cur, a, na * M::W * 8));
  KC_TRY(d.alloc(tiles * 4));
  KC_HIP_TRY(hipMemset(d.p, 0xff, tiles * 4));
  hipLaunchKernelGGL(k_tile_succ<M>, dim3((unsigned)tiles), dim3(256), 0, nullptr, cur.as<const typename M::State>(),
                     na, test_flags(), d.as<uint32_t>());
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(ts.data(), d.p, tiles * 4, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < tiles; ++i) res[i] = ts[i];
  return 0;
}

}  // namespace
}  // namespace kc

extern "C" int kc_spill_selftest(int kind, int np, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb,
                                 const uint64_t* c, uint64_t nc, uint64_t cap, uint64_t* out, uint64_t nout,
                                 uint64_t* res) {
  using namespace kc;
  if (kind < 0 || kind > 3 || (np != 1 && np != 2)) return bad("kind 0-3, np 1 or 2");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_spill_selftest: no HIP device");
    return -ENODEV;
  }
  switch (kind) {
    case 0:
      return run_claimset_keys(a, na, cap, out, nout, res);
    case 1:
      if (nb != na) return bad("spill_queries: one newmask word per parent");
      return np == 1 ? run_spill_queries<Model<1, 1, 1>>(a, na, b, c, nc, out, nout, res)
                     : run_spill_queries<Model<1, 2, 1>>(a, na, b, c, nc, out, nout, res);
    case 2:
      if (cap != nc) return bad("spill_apply: cap = parents");
      return run_spill_apply(a, na, b, nb, c, nc, out, nout, res);
    default:
      return np == 1 ? run_tile_succ<Model<1, 1, 1>>(a, na, res) : run_tile_succ<Model<1, 2, 1>>(a, na, res);
  }
}
