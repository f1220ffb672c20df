// claim_selftest.hip — test-only device harness for k_claim and the settle
// passes (engine_kernels.h): kc_claim_selftest runs one launch set over a
// frontier and a seen-set image of the suite's making, with the product's own
// launch spelling (launch_claim of claim_launch.h; the three settle launches
// as the engine's launch_settle issues them), for Model<1,1,1>, Model<1,2,1>
// and Model<1,3,1> (and Model<1,1,0> in kind 0: the deadlocked states).
// tests/test_gpu_claim.py compares the results with tests/claim_model.py.
//
//   kind 0  k_claim<M>, then k_settle_rec<0>, k_settle_rec<1>, k_settle_ovf<1>
//   kind 1  k_claim<M, 0, false, 0, false, true, false> (first-claim, 16-B slots)
//   kind 2  k_claim<M, 0, false, 0, false, true, true>  (first-claim, compact table)
//   kind 3  k_claim<M, 0, true, 1> with shard.hip's dynamic LDS and record
//           staging on, then the same three settle launches under the rank's
//           ClaimKeys (the rank's own tiles and overflow list; the received
//           records' passes of k_settle_both are not driven)
//
// Not driven: TLC order (TLC = true, gpos), the sharded deferred rebuild
// (shard_rebuild), ocsum, the narrow kernels, and the ABL / KC_DIAG builds.
//
// Data travels as u64 words, one per element whatever the kernel's element
// type.  Every output section is uploaded as the caller filled it and copied
// back whole: KC_EMIT_FORE guard elements, the kernel's array, the caller's
// aft guards.  The harness checks, on the host and before any launch,
// everything a kernel's indices depend on (so a machine without a GPU answers
// -EINVAL to bad input and -ENODEV only to good input), and sizes every buffer
// for the worst case the input allows: a candidate segment per tile, an
// overflow list of the frontier's successor count, a table with a free slot
// left after every successor is new.  Nothing of the product path calls this
// file.
#include <hip/hip_runtime.h>

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

namespace kc {
namespace {

using selftest::DevBuf;
using selftest::upload;

constexpr uint64_t FORE = KC_EMIT_FORE;
constexpr uint64_t kMaxParents = 1ull << 17, kMaxBase = 1ull << 20, kMaxSlots = 1ull << 24;
constexpr uint64_t kMaxStage = 1ull << 22, kMaxAft = 1ull << 10;
constexpr int NPAR = 12, NSEC = 12, NRES = 10 + 2 * A_COUNT;
enum ParFlag : uint64_t { PF_DEFER = 1, PF_PREV_COUNTS = 2, PF_CSUM = 4 };

int bad(const char* what) {
  set_error("kc_claim_selftest: %s", what);
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

template <class M>
typename M::State state_of(const uint64_t* w) {
  typename M::State s;
  for (int k = 0; k < M::W; ++k) s.w[k] = w[k];
  return s;
}

// The packed states are states of the lowered domain; tot[i] = the successors
// k_claim expands (an Assert parent's: those before the failing action).
template <class M>
int check_parents(const uint64_t* packed, uint64_t n, const Flags& f, uint64_t& succ) {
  for (uint64_t i = 0; i < n; ++i) {
    const typename M::State s = state_of<M>(packed + i * M::W);
    typename M::State r;
    uint64_t tup[M::TUPLE_WORDS];
    M::to_tuple(s, tup);
    bool same = M::from_tuple(tup, r);
    for (int k = 0; same && k < M::W; ++k) same = r.w[k] == s.w[k];
    if (!same) return bad("a parent is not a packed state of the model");
    succ += (uint64_t)std::min<int>(M::plan(s, f).total, M::MAXSUCC);
  }
  return 0;
}

template <class M>
int run(int kind, const kc_model_config& cfg, const uint64_t* par, const uint64_t* a, uint64_t na, const uint64_t* b,
        uint64_t nb, uint64_t* table, uint64_t ntable, uint64_t* out, uint64_t nout, uint64_t* res) {
  using State = typename M::State;
  constexpr uint64_t W = M::W, RW = Record<M>::RW;
  const Flags f = flags_of(cfg);
  const uint64_t n = par[0], base = par[1], level = par[2], spread = par[4], nslots = par[5], world = par[6];
  const uint64_t rank = par[7], pf = par[8], nprev = par[9], stage_cap = par[10], aft = par[11];
  const bool sh = kind == 3, first = kind == 1 || kind == 2, c8 = kind == 2, dfr = (pf & PF_DEFER) != 0;
  if (n == 0 || n > kMaxParents || base > kMaxBase || level == 0 || level >= (1u << 20) || par[3] > 1 ||
      spread >> 32 || pf > 7 || aft > kMaxAft)
    return bad("1 to 2^17 parents, base up to 2^20, level 1 to 2^20 - 1, check_deadlock 0 or 1, flags 0-7");
  if (nslots < 2 || nslots > kMaxSlots || ntable != (c8 ? nslots : 2 * nslots) || (c8 && (nslots & 1)))
    return bad("a table of 2 to 2^24 slots (even for the compact table), its image of 2 words a slot (compact: 1)");
  if (sh ? (world < 2 || world > 8 || rank >= world || base != 0 || dfr || stage_cap > kMaxStage)
         : (world != 1 || rank != 0 || stage_cap != 0))
    return bad("sharded: world 2 to 8, rank below world, base 0, no deferred frontier; else world 1, rank 0");
  if ((pf & PF_CSUM) && !first) return bad("chunk sums belong to the first-claim kinds");
  if ((pf & PF_PREV_COUNTS) && !dfr) return bad("prev_counts belongs to the deferred frontier");
  // the parents: given, or rebuilt here from the previous frontier's links
  std::vector<uint64_t> parents;
  std::vector<unsigned long long> link, pcounts;
  if (dfr) {
    if (na != 0 || nprev == 0 || nprev > kMaxParents || nb != nprev * W + n || !b)
      return bad("deferred: no parents, 1 to 2^17 previous states, then one link per parent");
    std::vector<int> ptot;
    if (const char* why = selftest::check_states<M>(b, nprev, f, ptot)) return bad(why);
    parents.resize(n * W);
    link.assign(base + n, ~0ull);
    pcounts.resize(nprev);
    for (uint64_t i = 0; i < nprev; ++i) pcounts[i] = M::plan(state_of<M>(b + i * W), f).counts;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t lk = b[nprev * W + i], pp = lk >> 8, t = lk & 0xff;
      if (pp >= nprev) return bad("a link's parent index outside the previous frontier");
      if (t >= (uint64_t)ptot[pp]) return bad("a link's position at or past the parent's successor count");
      const State gp = state_of<M>(b + pp * W);
      int slot, j;
      M::locate(M::plan(gp, f), (int)t, slot, j);
      State x;
      M::apply(gp, slot, j, f, x);
      for (uint64_t k = 0; k < W; ++k) parents[i * W + k] = x.w[k];
      link[base + i] = lk;
    }
    a = parents.data();
  } else if (!a || na != n * W || nb != 0 || nprev != 0) {
    return bad("n packed parents, and nothing of a previous frontier");
  }
  uint64_t succ = 0;
  KC_TRY(check_parents<M>(a, n, f, succ));
  // the table: a free slot is left when every successor is new, so no probe
  // loop runs round a full table
  if (!table) return bad("the table image");
  uint64_t used = 0;
  for (uint64_t i = 0; i < nslots; ++i) {
    const uint64_t fp = c8 ? table[i] : table[2 * i];
    if (fp) ++used;
    else if (!c8 && table[2 * i + 1]) return bad("a claim word in an empty slot of the table image");
  }
  if (used + succ + 1 > nslots) return bad("nslots too small: stored + every successor new + 1 free slot");
  // the output sections
  const uint64_t tiles = (n + CLAIM_TILE - 1) / CLAIM_TILE, C = (tiles + CSUM_TILES - 1) / CSUM_TILES;
  const uint64_t need[NSEC] = {n, tiles, tiles, (pf & PF_CSUM) ? C : 0, dfr ? (base + n) * W : 0, dfr ? base + n : 0,
                               sh ? n : 0, sh ? world * n : 0, sh ? world * tiles : 0, sh ? tiles : 0,
                               sh ? stage_cap * RW : 0, sh ? stage_cap * (W + 1) : 0};
  uint64_t at[NSEC + 1] = {0};
  for (int k = 0; k < NSEC; ++k) at[k + 1] = at[k] + FORE + need[k] + aft;
  if (!out || nout != at[NSEC] || !res) return bad("out: 12 sections of fore guards + the kind's elements + aft guards");
  // the device
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("kc_claim_selftest: no HIP device");
    return -ENODEV;   // (the input is valid: -EINVAL needs no GPU)
  }
  auto len = [&](int k) { return FORE + need[k] + aft; };
  Section<uint32_t> newmask, rcount, ttot, csum, repmask, tcnt;
  Section<uint64_t> dfout, stage;
  Section<unsigned long long> counts_out, stoff;
  Section<uint8_t> cnt;
  KC_TRY(newmask.up(out + at[0], len(0)));
  KC_TRY(rcount.up(out + at[1], len(1)));
  KC_TRY(ttot.up(out + at[2], len(2)));
  KC_TRY(csum.up(out + at[3], len(3)));
  KC_TRY(dfout.up(out + at[4], len(4)));
  KC_TRY(counts_out.up(out + at[5], len(5)));
  KC_TRY(repmask.up(out + at[6], len(6)));
  KC_TRY(cnt.up(out + at[7], len(7)));
  KC_TRY(tcnt.up(out + at[8], len(8)));
  KC_TRY(stoff.up(out + at[9], len(9)));
  KC_TRY(stage.up(out + at[10], len(10)));
  DevClaimSet cs;
  cs.compact = c8;
  cs.nslots = nslots;
  KC_TRY(cs.t.alloc(cs.units(nslots)));
  KC_HIP_TRY(hipMemcpy(cs.t.p, table, ntable * 8, hipMemcpyHostToDevice));
  DevBuf cur, prev, lk, pc, ctr, rec_fp, rec_lk, ovf_cnt, ovf_fp, ovf_lk, ovf_tile, stage_cur;
  if (dfr) {
    KC_TRY(upload(prev, b, nprev * W * 8));
    KC_TRY(upload(lk, link.data(), link.size() * 8));
    KC_TRY(upload(pc, pcounts.data(), nprev * 8));
  } else {
    KC_TRY(upload(cur, a, n * W * 8));
  }
  KC_TRY(ctr.alloc(sizeof(Counters)));
  KC_HIP_TRY(hipMemset(ctr.p, 0, sizeof(Counters)));
  const unsigned long long none = ~0ull;
  KC_HIP_TRY(hipMemcpy(ctr.p, &none, 8, hipMemcpyHostToDevice));   // err_key
  const uint64_t ocap = std::max<uint64_t>(succ, 1);
  KC_TRY(rec_fp.alloc(tiles * CLAIM_RCAP * 8));
  KC_TRY(rec_lk.alloc(tiles * CLAIM_RCAP * 4));
  KC_TRY(ovf_cnt.alloc(8));
  KC_TRY(stage_cur.alloc(8));
  KC_HIP_TRY(hipMemset(ovf_cnt.p, 0, 8));
  KC_HIP_TRY(hipMemset(stage_cur.p, 0, 8));
  KC_TRY(ovf_fp.alloc(ocap * 8));
  KC_TRY(ovf_lk.alloc(ocap * 4));
  KC_TRY(ovf_tile.alloc(ocap * 4));
  ShardArgs sa;
  sa.spread = (uint32_t)spread;
  sa.ovf = CandOvf{ovf_cnt.as<unsigned long long>(), ovf_fp.as<unsigned long long>(), ovf_lk.as<unsigned int>(),
                   ovf_tile.as<unsigned int>(), ocap};
  if (first) sa.ttot = ttot.ptr();
  if (pf & PF_CSUM) sa.csum = csum.ptr();
  if (sh) {
    sa.world = (uint32_t)world;
    sa.rank = (uint32_t)rank;
    sa.repmask = repmask.ptr();
    sa.cnt = cnt.ptr();
    sa.stage = stage.ptr();
    sa.stage_cur = stage_cur.as<unsigned long long>();
    sa.stage_cap = stage_cap;
    sa.tcnt = tcnt.ptr();
    sa.stoff = stoff.ptr();
  }
  DeferArgs df;
  State* dout = reinterpret_cast<State*>(dfout.ptr());
  if (dfr) {
    df.prev = prev.p;
    df.link = lk.as<const unsigned long long>();
    df.out = dout;
    if (pf & PF_PREV_COUNTS) df.prev_counts = pc.as<const unsigned long long>();
    df.counts_out = counts_out.ptr();
  }
  // (a deferred level's parents are rebuilt into the frontier buffer: the
  // engine passes cur_ + start with df.out = cur_)
  const State* dcur = dfr ? dout + base : cur.as<const State>();
  const ClaimBufs bufs{nullptr, rcount.ptr(), rec_fp.as<unsigned long long>(), rec_lk.as<unsigned int>(),
                       newmask.ptr(), ctr.as<Counters>()};
  const unsigned T = (unsigned)tiles;
  const uint32_t lv = (uint32_t)level;
  const int dl = (int)par[3];
  if (kind == 0)
    launch_claim<M>(nullptr, T, 0, dcur, n, base, f, dl, cs, lv, bufs, sa, df);
  else if (kind == 1)
    launch_claim<M, 0, false, 0, false, true, false>(nullptr, T, 0, dcur, n, base, f, dl, cs, lv, bufs, sa, df);
  else if (kind == 2)
    launch_claim<M, 0, false, 0, false, true, true>(nullptr, T, 0, dcur, n, base, f, dl, cs, lv, bufs, sa, df);
  else   // (base 0, no deferred frontier: checked above)
    selftest::launch_shard_claim<M>(T, dcur, n, f, dl, cs, lv, bufs, sa);
  KC_HIP_TRY(hipGetLastError());
  if (!first) {
    // the engine's launch_settle (engine.hip), under the rank's claim keys
    const ClaimKeys keys((uint32_t)rank);
    hipLaunchKernelGGL(k_settle_rec<0>, dim3(T + SETTLE_OVF_BLOCKS), dim3(CLAIM_TILE), 0, nullptr, n, base, cs.t.p,
                       cs.nslots, lv, bufs.rcount, bufs.rec_fp, bufs.rec_lk, bufs.newmask, bufs.ctr, keys,
                       (uint32_t*)nullptr, T, sa.ovf);
    hipLaunchKernelGGL(k_settle_rec<1>, dim3(T), dim3(CLAIM_TILE), 0, nullptr, n, base, cs.t.p, cs.nslots, lv,
                       bufs.rcount, bufs.rec_fp, bufs.rec_lk, bufs.newmask, bufs.ctr, keys, ttot.ptr());
    hipLaunchKernelGGL(k_settle_ovf<1>, dim3(SETTLE_OVF_GRID), dim3(256), 0, nullptr, sa.ovf, n, base, cs.t.p,
                       cs.nslots, lv, bufs.newmask, bufs.ctr, keys, ttot.ptr());
  }
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_TRY(newmask.down(out + at[0]));
  KC_TRY(rcount.down(out + at[1]));
  KC_TRY(ttot.down(out + at[2]));
  KC_TRY(csum.down(out + at[3]));
  KC_TRY(dfout.down(out + at[4]));
  KC_TRY(counts_out.down(out + at[5]));
  KC_TRY(repmask.down(out + at[6]));
  KC_TRY(cnt.down(out + at[7]));
  KC_TRY(tcnt.down(out + at[8]));
  KC_TRY(stoff.down(out + at[9]));
  KC_TRY(stage.down(out + at[10]));
  // the staged records unpacked: W state words, then the key
  for (uint64_t r = 0; sh && r < stage_cap; ++r) {
    uint64_t w[RW];
    for (uint64_t k = 0; k < RW; ++k) w[k] = out[at[10] + FORE + r * RW + k];
    State x;
    uint64_t key;
    record_unpack<M>(w, x, key);
    uint64_t* o = out + at[11] + FORE + r * (W + 1);
    for (uint64_t k = 0; k < W; ++k) o[k] = x.w[k];
    o[W] = key;
  }
  KC_HIP_TRY(hipMemcpy(table, cs.t.p, ntable * 8, hipMemcpyDeviceToHost));
  std::vector<Counters> hc(1);
  KC_HIP_TRY(hipMemcpy(hc.data(), ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
  const Counters& h = hc[0];
  res[0] = h.err_key;
  res[1] = h.overflow;
  res[2] = h.probes();
  res[3] = h.settles();
  res[4] = h.cand_ovf();
  res[5] = h.next_cand();
  res[6] = h.defer_flags;
  res[7] = h.defer_inv_n;
  KC_HIP_TRY(hipMemcpy(&res[8], ovf_cnt.p, 8, hipMemcpyDeviceToHost));
  KC_HIP_TRY(hipMemcpy(&res[9], stage_cur.p, 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < A_COUNT; ++k) {
    res[10 + k] = h.act_gen(k);
    res[10 + A_COUNT + k] = h.act_dist(k);
  }
  return 0;
}

}  // namespace
}  // namespace kc

extern "C" int kc_claim_selftest(int kind, const kc_model_config* cfg, const uint64_t* par, uint64_t npar,
                                 const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* table,
                                 uint64_t ntable, uint64_t* out, uint64_t nout, uint64_t* res, uint64_t nres) {
  using namespace kc;
  if (kind < 0 || kind > 3) return bad("kind 0-3");
  if (!cfg || !par || npar != (uint64_t)NPAR || nres != (uint64_t)NRES) return bad("cfg, 12 scalars, res of 54 words");
  const bool ns0 = kind == 0 && cfg->np == 1 && cfg->ns == 0;
  if (cfg->nc != 1 || cfg->np < 1 || cfg->np > 3 || (cfg->ns != 1 && !ns0))
    return bad("a model config with nc = ns = 1 and np 1 to 3 (kind 0: also nc = np = 1, ns = 0)");
  if (ns0) return run<Model<1, 1, 0>>(kind, *cfg, par, a, na, b, nb, table, ntable, out, nout, res);
  switch (cfg->np) {
    case 1:
      return run<Model<1, 1, 1>>(kind, *cfg, par, a, na, b, nb, table, ntable, out, nout, res);
    case 2:
      return run<Model<1, 2, 1>>(kind, *cfg, par, a, na, b, nb, table, ntable, out, nout, res);
    default:
      return run<Model<1, 3, 1>>(kind, *cfg, par, a, na, b, nb, table, ntable, out, nout, res);
  }
}
