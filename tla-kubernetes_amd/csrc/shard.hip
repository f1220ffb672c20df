// shard.hip — fingerprint-owner-sharded BFS stages for one GPU of R (one
// process per GPU; kubecheck/distributed.py drives the levels and does the
// exchange with RCCL all-to-all through torch.distributed).
//
// owner(fp) = floor(fp * R / 2^63) (fps are uniform in [1, 2^63)), the top
// bits of the fingerprint as in TLC's MultiFPSet [ext-TLC].  Per level:
//   expand : the engine's k_claim in shard mode (engine_kernels.h): LDS tile
//            dedup, then every tile representative this rank owns claims its
//            fp in the local ClaimSet shard (STORE-claim + newmask protocol);
//            the others are marked and counted per owner -> one exclusive
//            scan over the owner-major count matrix
//   pack   : k_shard_pack writes one record per remote representative
//            {state words, key} into the caller's send buffer, grouped by
//            owner, each group in (parent, t) order
//   (all-to-all by the caller)
//   insert : received records claim their fp in the same ClaimSet
//            (k_rec_claim, same protocol), then settle pass A (local and
//            record candidates fold their claims; a displaced local claim
//            loses its newmask bit), pass B (local displacers, record
//            inserters and displacers re-read their claim), two scans, and
//            the emit of the winners — this rank's own successors first (in
//            parent order), then the records' (in receive order) — with parent
//            keys (TLC trace file), invariant checks and counters.
// With R = 1 nothing is sent and the level is the single-GPU engine's.
// Keys: rank << 60 | parent index << 16 | successor position << 8 | low byte
// (action id in records and parent keys, ErrKind in error keys); the
// ClaimSet claim orders them by (rank, parent, position), so the same minimum
// is taken everywhere and the result does not depend on arrival order.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kubecheck.h"
#include "claim_launch.h"
#include "coldset.h"
#include "engine_kernels.h"
#include "engine_spill.h"
#include "engine_util.h"
#include "fpset_host.h"
#include "kc_common.h"
#include "record.h"
#include "shard.h"
#include "shard_narrow.h"
#include "shard_kernels.h"   // the level's kernels (also instantiated by shard_selftest.hip)

namespace kc {

constexpr uint64_t KEY_INIT = 0xFull << 60;   // parent key of an Init state (| init index)

template <class M>
class ShardT final : public ShardBase {
  using State = typename M::State;
  using Rec = Record<M>;

 public:
  ShardT(const kc_model_config& cfg, int rank, int world)
      : cfg_(cfg), rank_(rank), world_(world) {
    flags_ = flags_of(cfg);
    spill_ = cfg.seen_hbm_bytes > 0;
    if (cfg.spill_dir) spill_dir_ = cfg.spill_dir;   // (the seen-set's disk tier)
    cfg_.spill_dir = nullptr;      // (the caller's string is not kept)
    // A/B switches (round 5): KC_STAGE=0 packs every level with k_shard_pack
    // (re-expansion + per-parent owner scan); KC_SHARD_TSCAN=0 positions the
    // winners with per-parent / per-record device scans
    stage_on_ = env_flag("KC_STAGE", true);
    tcount_ = env_flag("KC_SHARD_TSCAN", true);
    defer_check_ = env_flag("KC_DEFER_CHECK", false);   // diagnostic: rebuilt states against materialised ones
    tlc_ = cfg.tlc_order && world > 1;
    // first-claim mode on the counted levels (k_claim FIRST, k_rec_claim_first;
    // no candidates, no settle passes): the first inserter owns a state, as in
    // a TLC -workers N run
    first_ = cfg.first_claim != 0;
    ocscan_ = env_flag("KC_CHUNK_SCAN", true);
    // (its ClaimSet holds fp words only, as the engine's in this mode: 8-B
    // slots, half the table to clear; the narrow levels write no claim words)
    cs_.compact = first_;
  }
  ~ShardT() override { (void)hipSetDevice(cfg_.device); }   // (the members free themselves on it)

  int setup() override {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      set_error("kc_shard: no HIP device visible (no CPU fallback)");
      return -ENODEV;
    }
    if (world_ < 1 || world_ > 15 || rank_ < 0 || rank_ >= world_) {
      set_error("kc_shard: bad rank/world %d/%d (1..15 ranks)", rank_, world_);
      return -EINVAL;
    }
    if (cfg_.device < 0 || cfg_.device >= ndev) {
      set_error("kc_shard: bad device %d", cfg_.device);
      return -EINVAL;
    }
    if (tlc_ && (spill_ || !tcount_)) {
      set_error("kc_shard: tlc_order needs the deferred frontier (no seen-set spill, KC_SHARD_TSCAN on)");
      return -EINVAL;
    }
    if (first_ && (tlc_ || spill_ || !tcount_)) {
      set_error("kc_shard: first_claim cannot run with %s", tlc_ ? "tlc_order (a deterministic claim order)"
                                                         : spill_ ? "the seen-set spill (its cold check settles winners)"
                                                                  : "KC_SHARD_TSCAN=0 (it needs the tile counts)");
      return -EINVAL;
    }
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    KC_TRY(st_.create(hipStreamNonBlocking));
    KC_TRY(d_ctr_.alloc(1));
    KC_TRY(h_ctr_.alloc(1));
    KC_TRY(h_exp_.alloc(1));         // (kCtrHead bytes of it are used)
    KC_TRY(d_owner_base_.alloc(16));
    KC_TRY(d_ovf_cnt_.alloc(1));     // (zeroed by k_head_reset every level)
    KC_TRY(d_stage_cur_.alloc(1));   // (likewise)
    KC_TRY(h_owner_base_.alloc(16));
    KC_TRY(ev_[0].create());
    return ev_[1].create();
  }

  // k_claim time (HIP events, cfg.timing != 0), launches and parents since
  // the last call to this function (reset on read).
  void claim_times(double* ms, uint64_t* launches, uint64_t* parents) override {
    *ms = claim_ms_;
    *launches = claim_launches_;
    *parents = claim_parents_;
    claim_ms_ = 0;
    claim_launches_ = claim_parents_ = 0;
  }

  int set_stream(hipStream_t st) override {
    return st_.borrow(st);
  }

  int init(uint64_t* n_local) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    const uint64_t fp_slots = cfg_.fpset_slots ? cfg_.fpset_slots : (1ull << 20);
    if (spill_) {
      KC_TRY(spill_setup());
    } else if (cs_.t && cs_.capacity() >= fp_slots) {
      KC_TRY(cs_.clear(st_));
    } else {
      KC_TRY(cs_.init(fp_slots, st_));
    }
    KC_HIP_TRY(hipMemsetAsync(d_ctr_, 0, sizeof(Counters), st_));
    // k_owner_cscan's chunk sums: zero when a level starts (a run that
    // stopped between k_claim and the scan left them dirty)
    if (ocsum_) KC_HIP_TRY(hipMemsetAsync(ocsum_, 0, ocsum_.cap * sizeof(uint32_t), st_));
    std::vector<State> mine;
    std::vector<unsigned long long> keys;
    std::vector<uint64_t> fps;
    cand_ = 0;
    for (int k = 0; k < M::num_init(); ++k) {
      State s;
      M::init_state(k, s, cfg_.variant);
      const uint64_t fp = M::template fingerprint<1>(s);
      const uint32_t o = (uint32_t)(((unsigned __int128)(fp << 1) * (uint64_t)world_) >> 64);
      if ((int)o != rank_) continue;
      mine.push_back(s);
      keys.push_back(KEY_INIT | (uint64_t)k);
      fps.push_back(fp);
      cand_ += (uint64_t)M::plan(s, flags_).total;
      // an Init-state violation's key orders by the Init state's index in
      // TLC's order (k << 16; the rank in bits 8-15), so the minimum over
      // the ranks is the first violating Init state TLC would report
      if (M::check(s, flags_.inv_mask) >= 0 && init_err_ == ~0ull)
        init_err_ = ((uint64_t)k << 16) | ((uint64_t)rank_ << 8) | 0x12;
    }
    n_ = mine.size();
    init_key_ = init_err_;
    cur_deferred_ = false;
    emitted_links_ = false;
    deferred_states_ = 0;
    cand_est_ = next_cand_est_ = false;
    last_new_ = 0;
    prev_rec_ = nullptr;
    defer_err_ = ~0ull;
    level_ = 1;
    level_base_.assign(1, 0);
    gen_init_ = n_;
    cand_total_ = 0;
    KC_TRY(cur_.grow(std::max<uint64_t>(n_, 1), st_));
    KC_TRY(pkeys_.grow(std::max<uint64_t>(n_, 1), st_));
    if (tlc_) {
      // level 1 in TLC order: Init states are distinct, each at its index
      // (G = k); this rank's in increasing k
      const uint64_t W = (uint64_t)M::num_init(), words = W / 32 + 1;
      std::vector<uint32_t> g, bits(words, 0), brank(words, 0);
      for (auto k : keys) {
        const uint32_t gk = (uint32_t)(k & 0xffffffffull);
        g.push_back(gk);
        bits[gk >> 5] |= 1u << (gk & 31);
      }
      for (uint64_t w = 1; w < words; ++w) brank[w] = brank[w - 1] + (uint32_t)__builtin_popcount(bits[w - 1]);
      KC_TRY(gpos_all_.grow(pkeys_.cap, st_));
      KC_TRY(gbits_cur_.grow(words, st_));
      KC_TRY(grank_cur_.grow(words, st_));
      if (n_) KC_HIP_TRY(hipMemcpyAsync(gpos_all_, g.data(), n_ * 4, hipMemcpyHostToDevice, st_));
      KC_HIP_TRY(hipMemcpyAsync(gbits_cur_, bits.data(), words * 4, hipMemcpyHostToDevice, st_));
      KC_HIP_TRY(hipMemcpyAsync(grank_cur_, brank.data(), words * 4, hipMemcpyHostToDevice, st_));
      KC_HIP_TRY(hipStreamSynchronize(st_));
    }
    if (n_) {
      KC_HIP_TRY(hipMemcpyAsync(cur_, mine.data(), n_ * sizeof(State), hipMemcpyHostToDevice, st_));
      KC_HIP_TRY(hipMemcpyAsync(pkeys_, keys.data(), n_ * 8, hipMemcpyHostToDevice, st_));
      DeviceArray<uint64_t> d_fps;
      KC_TRY(d_fps.alloc(n_));
      KC_HIP_TRY(hipMemcpyAsync(d_fps, fps.data(), n_ * 8, hipMemcpyHostToDevice, st_));
      launch_claimset_insert_list(d_fps.p, n_, cs_, 1u, nullptr, st_);
      KC_HIP_TRY(hipStreamSynchronize(st_));
    }
    KC_HIP_TRY(hipStreamSynchronize(st_));
    cs_.count = n_;
    distinct_ = n_;
    *n_local = n_;
    return 0;
  }

  // Claims this rank's own successors of the level; counts the rest per owner.
  int expand(uint64_t* counts, uint64_t* err_key) override {
    KC_TRY(expand_dev(0, ~0ull, false, nullptr));
    if (!dev_empty_) KC_HIP_TRY(hipStreamSynchronize(st_));
    return expand_done(counts, err_key);
  }
  // k_claim<M, 0, SH, OWN, TLC, FIRST, C8> over the level's n_ parents
  template <bool SH, int OWN = SH ? 1 : 0, bool TLC = false, bool FIRST = false, bool C8 = false>
  void claim(uint64_t tiles, size_t dyn, const ShardArgs& sh, const DeferArgs& df) {
    launch_claim<M, 0, SH, OWN, TLC, FIRST, C8>(st_, (unsigned)tiles, dyn, cur_, n_, 0, flags_, cfg_.check_deadlock, cs_,
                                                (uint32_t)level_ + 1,
                                                ClaimBufs{nullptr, rcount_, rec_fp_, rec_lk_, newmask_, d_ctr_}, sh, df);
  }
  int expand_dev(uint64_t status_new, uint64_t status_err, bool level1, uint64_t* d_row) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    rebuilt_ = false;
    gen_snap_ok_ = false;
    hipLaunchKernelGGL(k_head_reset, dim3(1), dim3(64), 0, st_, d_ctr_, d_ovf_cnt_, d_stage_cur_);
    send_total_ = 0;
    dev_init_err_ = init_err_;
    init_err_ = ~0ull;
    dev_empty_ = n_ == 0;
    if (n_ == 0) {
      // nothing to claim; a device row still gets its status words
      if (d_row)
        hipLaunchKernelGGL(k_owner_totals, dim3(1), dim3(64), 0, st_, off_, cnt_, (uint64_t)0, (uint32_t)world_,
                           d_owner_base_, d_ctr_, h_owner_base_, reinterpret_cast<unsigned long long*>(h_exp_.p),
                           d_row, status_new, status_err, (int)level1, dev_init_err_);
      dev_empty_ = d_row == nullptr;
      dev_zero_ = true;
      return 0;
    }
    dev_zero_ = false;
    if (n_ >= (1ull << 32)) {
      set_error("kc_shard_expand: frontier wider than 2^32 states");
      return -ENOMEM;
    }
    if (spill_) {
      // the level's claims (own successors and received records: about
      // cand_ successors together, of which the last level's fraction
      // filled hot slots) go into the fixed hot table; flush it first when
      // they might take it past 1/2 load
      const uint64_t need = std::min<uint64_t>(cand_, (uint64_t)((double)cand_ * sp_ratio_ * 1.25) + 4096);
      if (cs_.count > 0 && cs_.count + need > sp_.hot_limit) KC_TRY(spill_flush());
    } else {
      // (a deferred frontier's successor count is an estimate: 16 per parent
      // at least, so even MAXSUCC = 32 cannot fill the table, as the engine)
      KC_TRY(cs_.reserve(cand_est_ ? std::max<uint64_t>(cand_, 16 * n_) : cand_, st_));
    }
    const uint64_t tiles = (n_ + CLAIM_TILE - 1) / CLAIM_TILE;
    KC_TRY(rcount_.grow(tiles, st_));
    // (first-claim mode has no candidates: no records, no overflow list; its
    // k_claim writes each tile's new-state count, k_win_scan's input)
    if (first_) KC_TRY(wtot_.grow(tiles + 8, st_));
    if (!first_) KC_TRY(rec_fp_.grow(tiles * CLAIM_RCAP, st_));
    if (!first_) KC_TRY(rec_lk_.grow(tiles * CLAIM_RCAP, st_));
    // candidates past a tile's segment: one overflow list, bounded by the
    // level's successor count
    if (!first_) {
      // (estimated: at least two per parent; the list holds only the
      // candidates past a tile's first 256, a few percent of the successors)
      const uint64_t bound = cand_est_ ? std::max<uint64_t>(cand_, 2 * n_) : std::max<uint64_t>(cand_, 1);
      KC_TRY(ovf_fp_.grow_tight(bound, st_));
      KC_TRY(ovf_lk_.grow_tight(bound, st_));
      KC_TRY(ovf_tile_.grow_tight(bound, st_));
      ovf_ = CandOvf{d_ovf_cnt_, ovf_fp_, ovf_lk_, ovf_tile_, std::min(ovf_fp_.cap, std::min(ovf_lk_.cap, ovf_tile_.cap))};
    }
    KC_TRY(newmask_.grow(n_, st_));
    KC_TRY(cnt_.grow(n_ * world_, st_));
    KC_TRY(repmask_.grow(n_, st_));
    ShardArgs sh;
    sh.world = (uint32_t)world_;
    sh.rank = (uint32_t)rank_;
    sh.repmask = repmask_;
    sh.cnt = cnt_;
    sh.ovf = ovf_;
    if (tlc_) sh.gpos = gpos_cur();
    if (first_) sh.ttot = wtot_;
    // record staging (world > 1): an estimate from the last level's records
    // per parent, at most the level's successors; a level past it packs the
    // old way (DF_STAGE, pack())
    stage_level_ = world_ > 1 && stage_on_;
    if (stage_level_) {
      const uint64_t est = std::min<uint64_t>(std::max<uint64_t>(cand_, 1),
                                              (uint64_t)((double)n_ * rec_ratio_ * 1.5) + 65536);
      KC_TRY(stage_.grow_tight(est, st_));
      const uint64_t cells = tiles * (uint64_t)world_;
      KC_TRY(tcnt_.grow(cells + 8, st_));
      KC_TRY(toff_.grow(cells + 8, st_));
      KC_TRY(stoff_.grow(tiles, st_));
      ocscan_level_ = ocscan_;
      if (ocscan_level_) {
        const uint64_t old = ocsum_.cap;
        KC_TRY(ocsum_.grow((tiles / CSUM_TILES + 1) * (uint64_t)world_ + 8, st_));
        if (ocsum_.cap != old) KC_HIP_TRY(hipMemsetAsync(ocsum_, 0, ocsum_.cap * sizeof(uint32_t), st_));
        sh.ocsum = ocsum_;
      }
      sh.stage = stage_;
      sh.stage_cur = d_stage_cur_;
      sh.stage_cap = stage_.cap;
      sh.tcnt = tcnt_;
      sh.stoff = stoff_;
    }
    const size_t dyn = (size_t)(CLAIM_TILE + ((world_ + 3) / 4) * CLAIM_TILE) * sizeof(unsigned int);
    // the deferred frontier: this level's plans kept for the next level's
    // rebuild; a deferred frontier rebuilt into cur_ (the free buffer) from
    // the previous frontier (next_) and the last receive buffer
    DeferArgs df;
    if (defer_on_) {
      KC_TRY(pc_cur_.grow(n_, st_));
      df.counts_out = pc_cur_;
    }
    rebuilt_ = cur_deferred_;
    if (cur_deferred_) {
      KC_TRY(cur_.grow(n_, st_));
      df.prev = next_;
      df.link = link_cur_;
      df.prev_rec = prev_rec_;
      df.out = cur_;
      df.prev_counts = pc_prev_;
      if (tlc_) df.prev_gpos = gpos_prev();
      cur_deferred_ = false;
      ++deferred_levels_;
      deferred_states_ += n_;     // (rebuilt inside this k_claim: its algorithmic bytes, bench.py)
      // (the solo path stops on this level's deferred invariant after the
      // expand has counted its successors, where the exact path stops before
      // it: drop_last_expand then subtracts them, from the rebuilt states
      // and the plans this k_claim keeps)
      gen_snap_ok_ = d_row == nullptr && df.counts_out != nullptr;
      if (defer_check_) {
        KC_TRY(d_dchk_.alloc(4));
        const unsigned long long init[4] = {0ull, ~0ull, ~0ull, 0ull};
        KC_HIP_TRY(hipMemcpyAsync(d_dchk_, init, 32, hipMemcpyHostToDevice, st_));
        KC_HIP_TRY(hipStreamSynchronize(st_));
        df.check = d_dchk_;
      }
    }
    if (cfg_.timing) KC_HIP_TRY(hipEventRecord(ev_[0], st_));
    if (world_ == 1) {
      // one rank owns everything: the single-GPU engine's claim kernel (no
      // owner counting; claim keys then carry rank 0, which they do anyway)
      if (first_)
        claim<false, 1, false, true, true>(tiles, 0, sh, df);
      else
        claim<false, 1>(tiles, 0, sh, df);
    } else if (first_) {
      claim<true, 1, false, true, true>(tiles, dyn, sh, df);
    } else {
      if (tlc_)
        claim<true, 1, true>(tiles, dyn, sh, df);
      else
        claim<true>(tiles, dyn, sh, df);
    }
    if (cfg_.timing) KC_HIP_TRY(hipEventRecord(ev_[1], st_));
#ifdef KC_CLAIM_TRACE
    {
      unsigned long long t[16];
      KC_HIP_TRY(hipStreamSynchronize(st_));
      KC_HIP_TRY(hipMemcpyFromSymbol(t, HIP_SYMBOL(g_ctrace), sizeof t));
      if (t[0])
        fprintf(stderr, "ctrace rank %d level %d n %llu tiles %llu | us/block: prep %.2f deal %.2f succ %.2f compact %.2f "
                "claims %.2f stage %.2f tail %.2f | longest %.2f span %.2f\n", rank_, level_, (unsigned long long)n_,
                (unsigned long long)tiles, t[1] * 0.01 / t[0], t[2] * 0.01 / t[0], t[3] * 0.01 / t[0],
                t[4] * 0.01 / t[0], t[5] * 0.01 / t[0], t[6] * 0.01 / t[0], t[7] * 0.01 / t[0], t[8] * 0.01,
                (t[10] - t[9]) * 0.01);
      memset(t, 0, sizeof t);
      t[9] = ~0ull;
      KC_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_ctrace), t, sizeof t));
    }
#endif
    if (stage_level_) {
      // positions of the tiles' segments in the owner-grouped send buffer and
      // the owner totals (the all-gather row)
      if (tiles * (uint64_t)world_ >= (1ull << 31)) {
        set_error("kc_shard_expand: %llu tile x owner cells exceed one scan", (unsigned long long)(tiles * world_));
        return -ENOMEM;
      }
      if (ocscan_level_)
        hipLaunchKernelGGL(k_owner_cscan, dim3(1), dim3(TSCAN_THREADS), 0, st_, ocsum_,
                           (uint32_t)((tiles + CSUM_TILES - 1) / CSUM_TILES), (uint32_t)world_, toff_, d_owner_base_,
                           d_ctr_, h_owner_base_, reinterpret_cast<unsigned long long*>(h_exp_.p), d_row, status_new,
                           status_err, (int)level1, dev_init_err_);
      else
      hipLaunchKernelGGL(k_owner_tscan, dim3(1), dim3(TSCAN_THREADS), 0, st_, tcnt_, (uint32_t)tiles, (uint32_t)world_,
                         toff_, d_owner_base_, d_ctr_, h_owner_base_, reinterpret_cast<unsigned long long*>(h_exp_.p),
                         d_row, status_new, status_err, (int)level1, dev_init_err_);
      KC_HIP_TRY(hipGetLastError());
      return 0;
    }
    // one exclusive scan over the owner-major matrix = every record's position
    // in the owner-grouped send buffer (nothing to send at world 1)
    const uint64_t cells = n_ * (uint64_t)world_;
    KC_TRY(off_.grow(cells, st_));
    if (cells >= (1ull << 31)) {
      set_error("kc_shard_expand: frontier x world = %llu cells exceeds one scan (2^31)",
                (unsigned long long)cells);
      return -ENOMEM;
    }
    if (world_ > 1 && cells <= OWNER_SMALL_SCAN) {
      hipLaunchKernelGGL(k_owner_scan_small, dim3(1), dim3(1024), 0, st_, cnt_, off_, n_, (uint32_t)world_,
                         d_owner_base_, d_ctr_, h_owner_base_, reinterpret_cast<unsigned long long*>(h_exp_.p),
                         d_row, status_new, status_err, (int)level1, dev_init_err_);
    } else {
      if (world_ > 1) {
        size_t tmp_bytes = 0;
        const hipcub::TransformInputIterator<uint32_t, Widen8, const uint8_t*> cnt32(cnt_, Widen8());
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt32, off_.p, (int)cells, st_));
        KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, cnt32, off_.p, (int)cells, st_));
      }
      hipLaunchKernelGGL(k_owner_totals, dim3(1), dim3(64), 0, st_, off_, cnt_, n_, (uint32_t)world_,
                         d_owner_base_, d_ctr_, h_owner_base_, reinterpret_cast<unsigned long long*>(h_exp_.p),
                         d_row, status_new, status_err, (int)level1, dev_init_err_);
    }
    KC_HIP_TRY(hipGetLastError());
    return 0;
  }
  // after the stream sync that follows expand_dev
  int expand_done(uint64_t* counts, uint64_t* err_key) override {
    for (int o = 0; o < world_; ++o) counts[o] = 0;
    *err_key = dev_init_err_;
    defer_err_ = ~0ull;
    if (dev_zero_) return 0;
    defer_err_ = h_exp_->defer_err;
    const bool init_violated = dev_init_err_ != ~0ull;   // then it is THE error (see k_owner_totals)
    if (cfg_.timing) {
      float ms = 0;
      KC_HIP_TRY(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
      claim_ms_ += ms;
      ++claim_launches_;
    }
    claim_parents_ += n_;
    // (expand's head has a pinned copy of its own, h_exp_: a caller with
    // nothing to gather reads it only after insert's sync)
    if (h_exp_->overflow || h_exp_->batch_used) {
      set_error("kc_shard_expand: successor overflow or full table");
      return -ENOMEM;
    }
    staged_ = stage_level_ && !(h_exp_->defer_flags & DF_STAGE);
    if (defer_check_ && rebuilt_) {
      unsigned long long c[4];
      KC_HIP_TRY(hipMemcpy(c, d_dchk_, 32, hipMemcpyDeviceToHost));
      if (c[0])
        fprintf(stderr, "kc_shard rank %d level %d: %llu of %llu rebuilt states differ (first %lld, first record link %lld)\n",
                rank_, level_, c[0], (unsigned long long)n_, (long long)c[1], (long long)c[2]);
    }
    if (stage_level_ && !staged_) ++stage_fallbacks_;
    for (int o = 0; o < world_; ++o) {
      counts[o] = h_owner_base_[o];
      send_total_ += counts[o];
    }
    if (n_) rec_ratio_ = std::max(0.01, (double)(send_total_ - counts[rank_]) / (double)n_);
    if (h_exp_->err_key != ~0ull && !init_violated) {
      uint64_t e = ((uint64_t)rank_ << 60) | (uint64_t)h_exp_->err_key;
      if (tlc_) {
        // TLC order: the parent's G, no rank (the trace walk locates it)
        const uint64_t pidx = (h_exp_->err_key >> 16) & ((1ull << 44) - 1);
        uint32_t g = 0;
        KC_HIP_TRY(hipMemcpy(&g, gpos_cur() + pidx, 4, hipMemcpyDeviceToHost));
        e = ((uint64_t)g << 16) | (h_exp_->err_key & 0xffffull);
      }
      *err_key = std::min<uint64_t>(*err_key, e);
    }
    if (cfg_.verbose > 1)
      fprintf(stderr, "kc_shard rank %d level %d: expand n %llu rebuilt %d e1 %llx deferred-invariant %llx\n", rank_,
              level_, (unsigned long long)n_, (int)rebuilt_, (unsigned long long)*err_key,
              (unsigned long long)defer_err_);
    return 0;
  }

  uint64_t record_bytes() const override { return sizeof(Rec); }
  uint64_t init_error() const override { return init_key_; }
  hipStream_t stream() const override { return st_; }
  int rank() const override { return rank_; }
  int world() const override { return world_; }
  int device() const override { return cfg_.device; }
  int tuple_words() const override { return M::TUPLE_WORDS; }
  const kc_model_config& config() const override { return cfg_; }
  void set_async_pack(bool on) override { async_pack_ = on; }

  // Rebuild a counterexample on the host (TLC's trace file walk): from Init
  // state `init_idx` follow the successor ordinals, then add the violating
  // successor `pos` (invariant errors).  The same plan/apply code the
  // kernels run, compiled for the host.
  int replay(int init_idx, const std::vector<int>& ords, int kind, int pos,
             std::vector<std::vector<uint64_t>>& tuples, int* err_action, int* err_self,
             int* err_inv) override {
    if (init_idx < 0 || init_idx >= M::num_init()) {
      set_error("kc_shard replay: bad Init index %d", init_idx);
      return -EIO;
    }
    std::vector<State> path(1);
    M::init_state(init_idx, path[0], cfg_.variant);
    for (int t : ords) {
      const State& s = path.back();
      const typename M::Plan pl = M::plan(s, flags_);
      if (t < 0 || t >= pl.total) {
        set_error("kc_shard replay: ordinal %d out of %d", t, pl.total);
        return -EIO;
      }
      int slot, j;
      M::locate(pl, t, slot, j);
      State x;
      M::apply(s, slot, j, flags_, x);
      path.push_back(x);
    }
    *err_action = *err_self = *err_inv = -1;
    const State& s = path.back();
    const typename M::Plan pl = M::plan(s, flags_);
    if (kind == E_INVARIANT) {
      int slot, j;
      M::locate(pl, pos, slot, j);
      State x;
      M::apply(s, slot, j, flags_, x);
      path.push_back(x);
      *err_inv = M::check(x, flags_.inv_mask);
    } else if (kind == 0x12) {
      *err_inv = M::check(s, flags_.inv_mask);
    } else if (kind == E_ASSERT && pl.fail_slot >= 0) {
      *err_action = M::slot_action(s, pl.fail_slot);
      *err_self = pl.fail_slot < M::A ? pl.fail_slot
                  : pl.fail_slot < 2 * M::A ? pl.fail_slot - M::A
                                           : M::A + (pl.fail_slot - 2 * M::A);
    }
    tuples.assign(path.size(), std::vector<uint64_t>(M::TUPLE_WORDS));
    for (size_t k = 0; k < path.size(); ++k) M::to_tuple(path[k], tuples[k].data());
    return 0;
  }

  int pack(void* send) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    if (n_ && send_total_ && staged_) {
      // the tiles' staged segments, in tile order per owner
      const unsigned tiles = (unsigned)((n_ + CLAIM_TILE - 1) / CLAIM_TILE);
      hipLaunchKernelGGL(k_shard_gather<M>, dim3(tiles), dim3(256), 0, st_, stage_, stoff_, tcnt_, toff_, tiles,
                         (uint32_t)world_, (Rec*)send, ocscan_level_ ? 1 : 0);
      KC_HIP_TRY(hipGetLastError());
    } else if (n_ && send_total_) {
      if (stage_level_) {
        // (staging overflowed this level: the per-parent owner-major scan
        // that k_shard_pack positions its records with)
        const uint64_t cells = n_ * (uint64_t)world_;
        KC_TRY(off_.grow(cells, st_));
        size_t tmp_bytes = 0;
        const hipcub::TransformInputIterator<uint32_t, Widen8, const uint8_t*> cnt32(cnt_, Widen8());
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt32, off_.p, (int)cells, st_));
        KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, cnt32, off_.p, (int)cells, st_));
      }
      hipLaunchKernelGGL(k_shard_pack<M>, dim3((unsigned)((n_ + 255) / 256)), dim3(256), 0, st_,
                         cur_, n_, flags_, (uint32_t)world_, (uint64_t)rank_, off_, repmask_,
                         (Rec*)send, tlc_ ? gpos_cur() : (const uint32_t*)nullptr);
      KC_HIP_TRY(hipGetLastError());
    }
    // else stream-ordered with the caller (set_stream, or the native level
    // loop, which synchronises before it moves the records itself)
    if (st_.owned() && !async_pack_) KC_HIP_TRY(hipStreamSynchronize(st_));
    return 0;
  }

  // Claims the received records, settles local and record claims together,
  // emits the winners.  `recv` must be complete (caller's stream synced).
  int insert(const void* recv, uint64_t n, uint64_t* n_new, uint64_t* err_key) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    const Rec* in = (const Rec*)recv;
    *n_new = 0;
    *err_key = ~0ull;
    next_n_ = 0;
    next_cand_ = 0;
    next_cand_est_ = false;
    last_new_ = 0;
    // (an empty level emits nothing: advance must not take the last level's
    // links or plans for this one's)
    emitted_links_ = false;
    if (n_ == 0 && n == 0) return 0;
    if (n >= (1ull << 31) || n_ >= (1ull << 31)) {
      set_error("kc_shard_insert: more than 2^31 records or parents in one level");
      return -ENOMEM;
    }
    if (!spill_) KC_TRY(cs_.reserve(cand_ + n, st_));     // count excludes this level's local inserts (<= cand_)
    const uint32_t succ_level = (uint32_t)level_ + 1;
    const unsigned tiles = (unsigned)((n_ + CLAIM_TILE - 1) / CLAIM_TILE);
    const unsigned rgrid = (unsigned)((n + 255) / 256);
    if (first_) {
      // first-claim mode: the records' CASes (their block counts after this
      // level's own tile counts, which k_claim wrote), one scan, the emit
      const unsigned lt = n_ ? tiles : 0u, rb = n ? rgrid : 0u;
      KC_TRY(wtot_.grow((uint64_t)lt + rb + 8, st_, true));
      KC_TRY(woff_.grow((uint64_t)lt + rb + 8, st_));
      if (n) {
        KC_TRY(isnew_.grow(n, st_));
        hipLaunchKernelGGL(k_rec_claim_first<M>, dim3(rgrid), dim3(256), 0, st_, in, n, cs_.t, cs_.nslots, isnew_,
                           wtot_ + lt, d_ctr_, cs_.compact ? 1 : 0);
      }
      hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, wtot_, lt, rb, woff_, d_ctr_);
      return insert_emit(in, n, true, n_new, err_key);
    }
    if (n) {
      KC_TRY(rfp_.grow(n, st_));
      KC_TRY(flag_.grow(n, st_));
      KC_TRY(isnew_.grow(n, st_));
      KC_TRY(ioff_.grow(n, st_));
      hipLaunchKernelGGL(k_rec_claim<M>, dim3(rgrid), dim3(256), 0, st_, in, n, cs_.t, cs_.nslots,
                         succ_level, rfp_, flag_, d_ctr_, (int)tlc_);
    }
    // settle pass A (own tiles, records and the tiles' overflow list in one
    // launch), then pass B; n_ = 0 with n > 0 still runs pass A's first
    // workgroup, which resets the error key
    const unsigned lt = n_ ? tiles : 0u, ob = n_ ? SHARD_OVF_BLOCKS : 0u, rb = n ? rgrid : 0u;
    const unsigned sgrid = std::max(lt + rb + ob, 1u);
    // the tile-count path (not with the seen-set spill, whose cold check
    // works on per-parent / per-record offsets): pass B counts each own
    // tile's and each record block's new states, the overflow list's pass B
    // adds its winners to their tiles, one scan positions them all
    const bool tc = tcount_ && !spill_;
    ClaimKeys ck((uint32_t)rank_);
    if (tlc_) {
      if (!(defer_on_ && tc)) {
        set_error("kc_shard_insert: tlc_order needs the deferred frontier");
        return -EINVAL;
      }
      ck.gpos = gpos_cur();
      ck.gbits = gbits_cur_;
      ck.grank = grank_cur_;
    }
    // (one workgroup per own tile: round 5 measured 4 tiles per workgroup
    // slower at R = 8)
    auto settle = [&](int pass, unsigned ob_blocks, uint32_t* wt) {
      const unsigned g = std::max(lt + rb + ob_blocks, 1u);
      if (pass == 0)
        hipLaunchKernelGGL((k_settle_both<M, 0>), dim3(g), dim3(256), 0, st_, lt, rb, n_, cs_.t, cs_.nslots,
                           succ_level, ck, rcount_, rec_fp_, rec_lk_, newmask_, in, n, rfp_, flag_, isnew_, d_ctr_,
                           ovf_, wt);
      else
        hipLaunchKernelGGL((k_settle_both<M, 1>), dim3(g), dim3(256), 0, st_, lt, rb, n_, cs_.t, cs_.nslots,
                           succ_level, ck, rcount_, rec_fp_, rec_lk_, newmask_, in, n, rfp_, flag_, isnew_, d_ctr_,
                           ovf_, wt);
    };
    settle(0, ob, (uint32_t*)nullptr);
    if (tc) {
      KC_TRY(wtot_.grow((uint64_t)lt + rb + 8, st_));
      KC_TRY(woff_.grow((uint64_t)lt + rb + 8, st_));
      if (lt + rb) settle(1, 0, wtot_);
      if (n_ && n_ <= FUSE_OVF_SCAN_MAX) {
        hipLaunchKernelGGL(k_ovf_win_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, ovf_, n_, cs_.t, cs_.nslots,
                           succ_level, newmask_, d_ctr_, ck, wtot_, lt, rb, woff_);
      } else {
        if (n_)
          hipLaunchKernelGGL(k_settle_ovf<1>, dim3(SHARD_OVF_BLOCKS), dim3(256), 0, st_, ovf_, n_, (uint64_t)0, cs_.t,
                             cs_.nslots, succ_level, newmask_, d_ctr_, ck, wtot_);
        hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(TSCAN_THREADS), 0, st_, wtot_, lt, rb, woff_, d_ctr_);
      }
    } else {
      hipLaunchKernelGGL((k_settle_both<M, 1>), dim3(sgrid), dim3(256), 0, st_, lt, rb, n_, cs_.t,
                         cs_.nslots, succ_level, ck, rcount_, rec_fp_, rec_lk_, newmask_, in, n, rfp_,
                         flag_, isnew_, d_ctr_, ovf_, (uint32_t*)nullptr);
      // positions: this rank's own winners first, then the records'
      KC_TRY(scan_winners(n));
      if (spill_) {
        bool changed = false;
        KC_TRY(spill_check(n, tiles, rgrid, &changed));
        if (changed) KC_TRY(scan_winners(n));
      }
    }
    return insert_emit(in, n, tc, n_new, err_key);
  }

  // The emit half of insert(): the winners' positions are known (woff_ on
  // the tile-count path `tc`, else offsets_ / ioff_).
  int insert_emit(const Rec* in, uint64_t n, bool tc, uint64_t* n_new, uint64_t* err_key) {
    const unsigned rgrid = (unsigned)((n + 255) / 256);
    // capacity: at most one new state per own successor and per record
    // (the deferred frontier: links and parent keys only, sized by the
    // estimate when the level's successor count is one; past it the emit
    // runs again with the exact count)
    const bool links = defer_on_ && tc;
    emitted_links_ = links;
    last_in_ = in;
    const uint64_t bound = cand_ + n;
    if (!links || defer_check_) KC_TRY(next_.grow(std::max<uint64_t>(bound, 1), st_));
    const uint64_t next_gidx = level_base_.back() + n_;
    KC_TRY(pkeys_.grow(next_gidx + bound + 1, st_, true));
    if (tlc_) KC_TRY(gpos_all_.grow(pkeys_.cap, st_, true));
    if (links) KC_TRY(link_next_.grow(std::max<uint64_t>(bound, 1), st_));
    const unsigned lb = (unsigned)((n_ + 255) / 256), eg = std::max(lb + (n ? rgrid : 0u), 1u);
    const int tail = eg <= SHARD_TAIL_BLOCKS;
    if (links && defer_check_) {
      // (diagnostic) the materialising emit too, into next_ — which the next
      // level's rebuild then compares with — on scratch counters and keys
      KC_TRY(d_ctr_dbg_.alloc(1));
      KC_TRY(pk_dbg_.grow(bound + 1, st_));
      hipLaunchKernelGGL(k_shard_emit<M>, dim3(eg), dim3(256), 0, st_, cur_, n_, lb, flags_, (uint64_t)rank_, newmask_,
                         offsets_, in, n, isnew_, ioff_, next_, pk_dbg_, (uint64_t)0, d_ctr_dbg_,
                         (unsigned long long*)nullptr, 0, woff_);
    }
    auto emit = [&]() {
      if (links)
        hipLaunchKernelGGL(k_shard_emit_links<M>, dim3(eg), dim3(256), 0, st_, n_, lb, (uint64_t)rank_,
                           tlc_ ? gpos_cur() : (const uint32_t*)nullptr, newmask_, in, n,
                           isnew_, woff_, link_next_, pkeys_, next_gidx,
                           std::min<uint64_t>(link_next_.cap, pkeys_.cap - next_gidx), d_ctr_,
                           reinterpret_cast<unsigned long long*>(h_ctr_.p), tail);
      else
        hipLaunchKernelGGL(k_shard_emit<M>, dim3(eg), dim3(256), 0, st_, cur_, n_, lb, flags_, (uint64_t)rank_,
                           newmask_, offsets_, in, n, isnew_, ioff_, next_, pkeys_, next_gidx, d_ctr_,
                           reinterpret_cast<unsigned long long*>(h_ctr_.p), tail,
                           tc ? woff_ : (const uint32_t*)nullptr);
      if (!tail)
        hipLaunchKernelGGL(k_shard_cand, dim3(1), dim3(64), 0, st_, d_ctr_,
                           reinterpret_cast<unsigned long long*>(h_ctr_.p));
    };
    emit();
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipStreamSynchronize(st_));
    if (links && (h_ctr_->defer_flags & DF_CAPACITY)) {
      const uint64_t need = h_ctr_->level_new;
      KC_TRY(link_next_.grow(need, st_));
      KC_TRY(pkeys_.grow(next_gidx + need + 1, st_, true));
      if (tlc_) KC_TRY(gpos_all_.grow(pkeys_.cap, st_, true));
      KC_HIP_TRY(hipMemsetAsync(&d_ctr_->defer_flags, 0, 8, st_));
      ++emit_retries_;
      emit();
      KC_HIP_TRY(hipGetLastError());
      KC_HIP_TRY(hipStreamSynchronize(st_));
      if (h_ctr_->defer_flags & DF_CAPACITY) {
        set_error("kc_shard_insert: %llu links do not fit %llu", (unsigned long long)need,
                  (unsigned long long)link_next_.cap);
        return -ENOMEM;
      }
    }
    if (h_ctr_->overflow || h_ctr_->batch_used) {
      set_error("kc_shard_insert: table full or claim protocol violation");
      return -ENOMEM;
    }
    next_n_ = h_ctr_->level_new;
    const uint64_t dc = h_ctr_->cand_total - cand_total_;
    cand_total_ = h_ctr_->cand_total;
    if (links) {
      // successors counted this level: those of this level's rebuilt states
      // (or none: a level k_claim did not rebuild has an exact count already);
      // the next level's, for its buffers, estimated from them
      const uint64_t cur_cand = rebuilt_ ? dc : cand_;
      if (n_ && (rebuilt_ || !cand_est_)) succ_ratio_ = std::max(1.0, (double)cur_cand / (double)n_);
      next_cand_ = next_n_ ? (uint64_t)((double)next_n_ * succ_ratio_ * 1.25) + 4096 : 0;
      next_cand_est_ = true;
    } else {
      next_cand_ = dc;
      next_cand_est_ = false;
    }
    last_new_ = next_n_;
    if (!spill_) cs_.count += next_n_;   // (spill: spill_check counted the hot slots)
    distinct_ += next_n_;
    if (h_ctr_->err_key != ~0ull) *err_key = h_ctr_->err_key;
    *n_new = next_n_;
    if (cfg_.verbose > 1)
      fprintf(stderr, "kc_shard rank %d level %d: insert records %llu new %llu links %d e2 %llx\n", rank_, level_,
              (unsigned long long)n, (unsigned long long)next_n_, (int)links, (unsigned long long)*err_key);
    return 0;
  }

  // Exclusive scans of the own winners' newmask popcounts (offsets_) and the
  // records' isnew flags (ioff_); C->chunk_base / level_new = the totals.
  int scan_winners(uint64_t n) {
    if (n_) KC_TRY(offsets_.grow(n_, st_));
    if (n_ <= SHARD_SMALL_SCAN && n <= SHARD_SMALL_SCAN) {
      hipLaunchKernelGGL(k_shard_scan_small, dim3(1), dim3(1024), 0, st_, newmask_, n_, offsets_, isnew_, n, ioff_,
                         d_ctr_);
    } else {
      size_t tmp_bytes = 0;
      if (n_) {
        const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> newcnt(newmask_, NewCount());
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, newcnt, offsets_.p, (int)n_, st_));
        KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, newcnt, offsets_.p, (int)n_, st_));
      }
      if (n) {
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, isnew_.p, ioff_.p, (int)n, st_));
        KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
        KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, isnew_.p, ioff_.p, (int)n, st_));
      }
      hipLaunchKernelGGL(k_shard_base, dim3(1), dim3(64), 0, st_, offsets_, newmask_, n_, ioff_, isnew_, n, d_ctr_);
    }
    return 0;
  }

  // ---- seen-set spill (cfg.seen_hbm_bytes > 0; the tier is SeenSpill,
  // engine_spill.h, as the engine's), with whole levels: the sharded level
  // cannot be cut into chunks without cutting every rank's.
  // Budget B per rank: the hot table is flushed before a level whose claims
  // might take it past 1/2 load (a level may go on to 7/8, hot_hard_: an
  // estimate, not a bound, decides the flush); the arena serves the flush
  // (up to 7/8 of the slots' keys) and the level's cold check (q_max queries
  // per window, 64-bit locations).
  int spill_setup() {
    typename SeenSpill<uint64_t>::Policy pol;
    hot_hard_ = SeenSpill<uint64_t>::hot_slots(cfg_.seen_hbm_bytes) / 8 * 7;
    pol.flush_cap = hot_hard_;
    pol.q_max = std::max<uint64_t>(256, hot_hard_ * 8 / 48 / 256 * 256);
    // KC_SEEN_QMAX: queries per cold-check window (tests: many windows)
    if (const uint64_t qm = env_u64("KC_SEEN_QMAX"); qm >= 256) pol.q_max = std::min<uint64_t>(pol.q_max, qm / 256 * 256);
    pol.who = "kc_shard";
    pol.dir = spill_dir_;
    KC_TRY(sp_.setup(cfg_, cs_, st_, pol));
    sp_ratio_ = 1.0;
    return 0;
  }

  // Hot table -> one sorted cold run; the table starts over empty.
  int spill_flush() {
    KC_TRY(sp_.flush(cs_, hot_hard_, st_));
    cs_.count = 0;
    return 0;
  }

  // The level's winners w.r.t. the hot table (C->level_new after the first
  // scans) against the cold tier; those found lose.  *changed: some did.
  int spill_check(uint64_t n, unsigned tiles, unsigned rgrid, bool* changed) {
    *changed = false;
    KC_HIP_TRY(hipMemcpyAsync(sp_.h_spctr + 2, &d_ctr_->level_new, 8, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    const uint64_t m = sp_.h_spctr[2];
    cs_.count += m;                   // the hot slots this level filled
    sp_.queries += m;
    if (cand_) sp_ratio_ = std::min(1.0, (double)m / (double)cand_);
    if (cs_.count > hot_hard_) {
      set_error("kc_shard: one level put %llu fingerprints into a hot seen-set of %llu slots; raise seen_hbm_bytes",
                (unsigned long long)m, (unsigned long long)cs_.nslots);
      return -ENOMEM;
    }
    if (m == 0 || sp_.cold.empty()) return 0;
    const auto q = sp_.carve();
    const uint64_t q_max = sp_.q_max;
    const unsigned lb = n_ ? tiles : 0u;
    // windows from the last to the first: a winner that loses clears its
    // bit, which would shift the positions of its parent's later winners,
    // so every window is taken before any lower one changes
    const uint64_t nwin = (m + q_max - 1) / q_max;
    for (uint64_t wi = nwin; wi-- > 0;) {
      const uint64_t w0 = wi * q_max, w1 = std::min(m, w0 + q_max), c = w1 - w0;
      hipLaunchKernelGGL(k_shard_spill_queries<M>, dim3(std::max(lb + rgrid, 1u)), dim3(256), 0, st_, cur_.p, n_, lb,
                         flags_, newmask_.p, offsets_.p, n, rfp_.p, isnew_.p, ioff_.p, d_ctr_.p, w0, w1, q.qk, q.ql);
      hipcub::DoubleBuffer<uint64_t> kb(q.qk, q.qk2);
      hipcub::DoubleBuffer<uint64_t> vb(q.ql, q.ql2);
      size_t tb = sp_.sp_qtmp_bytes;
      KC_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(q.tmp, tb, kb, vb, (int)c, 0, 64, st_));
      KC_HIP_TRY(hipMemsetAsync(q.found, 0, c, st_));
      KC_TRY(sp_.cold.probe(kb.Current(), c, q.found, sp_.d_spctr, st_));
      hipLaunchKernelGGL(k_shard_spill_apply, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, st_, kb.Current(),
                         vb.Current(), q.found, c, newmask_.p, isnew_.p, cs_.t, cs_.nslots, d_ctr_.p);
      KC_HIP_TRY(hipGetLastError());
    }
    *changed = true;
    return 0;
  }

  // ---- device-driven narrow levels (shard_narrow.h)
  int sn_setup(uint32_t cap) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    sn_cap_ = std::max<uint32_t>(1, std::min<uint32_t>(cap, SN_SLOT_MAX));
    KC_TRY(d_snc_.alloc(1));
    KC_TRY(h_snc_.alloc(1));
    KC_TRY(d_sns_.alloc(1));
    KC_TRY(sn_send_.alloc((uint64_t)world_ * sn_slot_bytes() / 8));
    KC_TRY(sn_recv_.alloc((uint64_t)world_ * sn_slot_bytes() / 8));
    KC_HIP_TRY(hipMemset(d_snc_, 0, sizeof(SNCtl)));
    KC_HIP_TRY(hipMemset(sn_send_, 0, (uint64_t)world_ * sn_slot_bytes()));
    KC_HIP_TRY(hipMemset(sn_recv_, 0, (uint64_t)world_ * sn_slot_bytes()));
    return 0;
  }
  uint64_t sn_slot_bytes() const override { return (uint64_t)(sn_cap_ + 1) * sizeof(Rec); }
  void* sn_send() override { return sn_send_; }
  void* sn_recv() override { return sn_recv_; }

  // A batch's control block.  It is written whatever happens: when a buffer
  // cannot be grown the block says "failed", so this rank's next level stops
  // every rank (through its headers) instead of running on short buffers.
  int sn_begin(uint64_t status_new, uint64_t status_err, int batch) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    int rc = 0;
    if (status_new != n_) {
      set_error("kc_shard narrow: status %llu is not the frontier's width %llu", (unsigned long long)status_new,
                (unsigned long long)n_);
      rc = -EIO;
    }
    const uint64_t in = (uint64_t)(world_ - 1) * sn_cap_;
    const uint64_t per = SN_CAND_MAX + in + 1;           // new states one level may add, at most
    const uint64_t bufs = std::max<uint64_t>(SN_MAX, per);
    const uint64_t base = level_base_.back();
    if (!rc) rc = cur_.grow(bufs, st_, true);
    if (!rc) rc = next_.grow(bufs, st_);
    if (!rc) rc = pkeys_.grow(base + n_ + (uint64_t)batch * per + 1, st_, true);
    // ClaimSet room for the batch: a few times the first level's bound, not
    // the batch's worst case (that forced ~2M entries on every model; ADVICE
    // r4).  The device stops a level whose claims might not fit (room below,
    // sn_local_stop: SN_STOP, the counted path takes it), so a reserve that
    // finds no memory is not a failure either (the table is unchanged then).
    if (!rc && cs_.reserve(std::min<uint64_t>((uint64_t)batch * per, 4 * (cand_ + in + 1) + (1u << 16)), st_) < 0)
      (void)hipGetLastError();
    SNCtl& h = *h_snc_;
    memset(&h, 0, offsetof(SNCtl, lwidths));
    h.active = 1;
    h.level = (uint32_t)level_;
    h.world = (uint32_t)world_;
    h.rank = (uint32_t)rank_;
    h.slot_cap = sn_cap_;
    h.stop_level = (uint32_t)cfg_.max_levels;
    h.n = n_;
    h.level_gidx = base;
    h.cand = cand_;
    h.err[(level_ - 1) & 1] = status_err;
    h.err[level_ & 1] = ~0ull;
    if (rc) {
      h.fail = 1;           // (buf_cap = room = par_cap = 0: nothing runs)
    } else {
      h.room = cs_.capacity() / 2 > cs_.count ? cs_.capacity() / 2 - cs_.count : 0;
      h.buf_cap = std::min(cur_.cap, next_.cap);
      h.par_cap = pkeys_.cap;
    }
    sn_n0_ = n_;
    KC_HIP_TRY(hipMemcpyAsync(d_snc_, h_snc_, offsetof(SNCtl, lwidths), hipMemcpyHostToDevice, st_));
    KC_HIP_TRY(hipMemsetAsync(d_sns_->lt, 0, sizeof(d_sns_->lt), st_));
    return rc;
  }
  int sn_pre(uint32_t lev, bool fail) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    if (fail) hipLaunchKernelGGL(k_sn_fail, dim3(1), dim3(64), 0, st_, d_snc_);
    hipLaunchKernelGGL(k_sn_expand<M>, dim3(SN_XWG), dim3(SN_THREADS), 0, st_, cur_, next_, flags_,
                       cfg_.check_deadlock, lev, d_snc_, d_sns_);
    if (world_ > 1)
      hipLaunchKernelGGL(k_sn_pack<M>, dim3(SN_PWG), dim3(SN_THREADS), 0, st_, cur_, next_, flags_, lev, d_snc_,
                         d_sns_, sn_send_);
    KC_HIP_TRY(hipGetLastError());
    return 0;
  }
  int sn_post(uint32_t lev) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    const unsigned rgrid = world_ > 1 ? (unsigned)(((uint64_t)world_ * sn_cap_ + SN_THREADS - 1) / SN_THREADS) : 0u;
    if (world_ > 1)
      hipLaunchKernelGGL(k_sn_recv<M>, dim3(rgrid), dim3(SN_THREADS), 0, st_, lev, d_snc_, d_sns_, sn_recv_, d_ctr_);
    hipLaunchKernelGGL(k_sn_claim<M>, dim3(SN_CWG + rgrid), dim3(SN_THREADS), 0, st_, lev, d_snc_, d_sns_, sn_recv_,
                       cs_.t, cs_.nslots, d_ctr_, cs_.word_shift());
    hipLaunchKernelGGL(k_sn_emit<M>, dim3(SN_EWG + rgrid), dim3(SN_THREADS), 0, st_, cur_, next_, flags_, lev, d_snc_,
                       d_sns_, sn_recv_, pkeys_, d_ctr_);
    KC_HIP_TRY(hipGetLastError());
    return 0;
  }
  int sn_end(SNOut* out) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    KC_HIP_TRY(hipMemcpyAsync(h_snc_, d_snc_, sizeof(SNCtl), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, kCtrHead, hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    const SNCtl& h = *h_snc_;
    // (the outcome is filled in before a failure is reported: the caller
    // keeps in step with its peers on it, shard_driver.hip)
    out->filled = true;
    out->levels = (int)h.levels;
    out->reason = h.active ? SN_RUN : h.reason;
    out->widths.assign(h.gwidths, h.gwidths + std::min<uint32_t>(h.levels, KC_MAX_LEVELS));
    uint64_t w = sn_n0_;
    for (uint32_t k = 0; k < h.levels; ++k) {
      level_base_.push_back(level_base_.back() + w);
      w = k < (uint32_t)KC_MAX_LEVELS ? h.lwidths[k] : 0;
    }
    cs_.count += h.new_total;
    distinct_ += h.new_total;
    level_ = (int)h.level;
    n_ = h.n;
    cand_ = h.cand;
    if (h.levels & 1) {
      cur_.swap(next_);
    }
    out->status_new = n_;
    out->status_err = h.err[(h.level - 1) & 1];
    out->sent = h.sent_total;
    if (h_ctr_->overflow) {
      set_error("kc_shard narrow: a full level table or ClaimSet, or a header of another level");
      return -ENOMEM;
    }
    return 0;
  }

  int advance() override {
    level_base_.push_back(level_base_.back() + n_);
    cur_.swap(next_);
    if (emitted_links_) {
      // the new frontier is links into the old one (now next_) and into the
      // receive buffer; this level's plans become the previous level's
      link_cur_.swap(link_next_);
      pc_cur_.swap(pc_prev_);
      prev_rec_ = last_in_;
      cur_deferred_ = next_n_ > 0;
      emitted_links_ = false;
    }
    if (tlc_) {
      gbits_cur_.swap(gbits_next_);
      grank_cur_.swap(grank_next_);
    }
    n_ = next_n_;
    cand_ = next_cand_;
    cand_est_ = next_cand_est_;
    next_cand_ = 0;
    next_cand_est_ = false;
    ++level_;
    return 0;
  }

  void set_deferred(bool on) override { defer_on_ = on && !spill_ && tcount_; }
  uint64_t defer_error() const override { return defer_err_; }
  void drop_last_insert() override {
    distinct_ -= last_new_;
    last_new_ = 0;
  }
  int drop_last_expand() override {
    if (!gen_snap_ok_) return 0;
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    if (n_)
      hipLaunchKernelGGL(k_undo_gen<M>, dim3((unsigned)((n_ + 255) / 256)), dim3(256), 0, st_, cur_, pc_cur_, n_, d_ctr_);
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipStreamSynchronize(st_));
    gen_snap_ok_ = false;
    return 0;
  }
  int materialize(uint64_t* derr) override {
    *derr = ~0ull;
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    if (!cur_deferred_ || n_ == 0) {
      cur_deferred_ = false;
      return 0;
    }
    KC_TRY(cur_.grow(n_, st_));
    DeferArgs df;
    df.prev = next_;
    df.link = link_cur_;
    df.prev_rec = prev_rec_;
    df.out = cur_;
    df.prev_counts = pc_prev_;
    if (tlc_) df.prev_gpos = gpos_prev();
    KC_HIP_TRY(hipMemsetAsync(&d_ctr_->defer_err, 0xff, 8, st_));
    if (tlc_)
      hipLaunchKernelGGL((k_shard_materialize<M, true>), dim3((unsigned)((n_ + 255) / 256)), dim3(256), 0, st_, df, n_,
                         flags_, (uint64_t)rank_, d_ctr_);
    else
      hipLaunchKernelGGL((k_shard_materialize<M, false>), dim3((unsigned)((n_ + 255) / 256)), dim3(256), 0, st_, df,
                         n_, flags_, (uint64_t)rank_, d_ctr_);
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipMemcpyAsync(h_ctr_, d_ctr_, sizeof(Counters), hipMemcpyDeviceToHost, st_));
    KC_HIP_TRY(hipStreamSynchronize(st_));
    cur_deferred_ = false;
    ++deferred_levels_;
    const uint64_t tot = h_ctr_->next_cand();      // (the stripes: materialize added this level's successors)
    cand_ = tot - cand_total_;
    cand_total_ = tot;
    cand_est_ = false;
    if (n_) succ_ratio_ = std::max(1.0, (double)cand_ / (double)n_);
    *derr = h_ctr_->defer_err;
    return 0;
  }

  bool tlc() const override { return tlc_; }
  const uint32_t* gpos_cur() const { return gpos_all_ + level_base_.back(); }
  const uint32_t* gpos_prev() const {
    return gpos_all_ + (level_base_.size() >= 2 ? level_base_[level_base_.size() - 2] : 0);
  }
  int tlc_masks(uint64_t W, uint32_t** mask) override {
    *mask = nullptr;
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    if (!tlc_ || W >= (1ull << 31)) {
      set_error("kc_shard tlc_masks: %s", tlc_ ? "a level of 2^31 states or more" : "not in TLC order");
      return -EINVAL;
    }
    KC_TRY(wmask_.grow(W, st_));
    KC_HIP_TRY(hipMemsetAsync(wmask_, 0, W * 4, st_));
    const uint64_t next_gidx = level_base_.back() + n_;
    if (next_n_)
      hipLaunchKernelGGL(k_tlc_mask, dim3((unsigned)((next_n_ + 255) / 256)), dim3(256), 0, st_, pkeys_ + next_gidx,
                         next_n_, wmask_, W, d_ctr_);
    KC_HIP_TRY(hipGetLastError());
    *mask = wmask_;
    return 0;
  }
  int tlc_order(uint64_t W) override {
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    // (the next level has at most 32 W states: W + 1 bitmap words)
    const uint64_t words = W + 1;
    KC_TRY(gbits_next_.grow(words, st_));
    KC_TRY(grank_next_.grow(words, st_));
    KC_TRY(wbase_.grow(W, st_));
    KC_HIP_TRY(hipMemsetAsync(gbits_next_, 0, words * 4, st_));
    size_t tmp_bytes = 0;
    const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> wc(wmask_, NewCount());
    KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, wc, wbase_.p, (int)W, st_));
    KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
    KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, wc, wbase_.p, (int)W, st_));
    const uint64_t nn = next_n_, next_gidx = level_base_.back() + n_;
    const unsigned g = (unsigned)((nn + 255) / 256);
    if (nn) {
      KC_TRY(gnew_.grow(nn, st_));
      hipLaunchKernelGGL(k_tlc_pos, dim3(g), dim3(256), 0, st_, pkeys_ + next_gidx, nn, wmask_, wbase_, gnew_,
                         gbits_next_);
    }
    const hipcub::TransformInputIterator<uint32_t, NewCount, const uint32_t*> bc(gbits_next_, NewCount());
    KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, bc, grank_next_.p, (int)words, st_));
    KC_TRY(scan_tmp_.grow(tmp_bytes + 16, st_));
    KC_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp_.p, tmp_bytes, bc, grank_next_.p, (int)words, st_));
    if (nn) {
      KC_TRY(link_tmp_.grow(std::max(nn, link_next_.cap), st_));
      KC_TRY(pk_tmp_.grow(nn, st_));
      hipLaunchKernelGGL(k_tlc_perm, dim3(g), dim3(256), 0, st_, nn, gnew_, gbits_next_, grank_next_, link_next_,
                         pkeys_ + next_gidx, link_tmp_, pk_tmp_, gpos_all_ + next_gidx);
      KC_HIP_TRY(hipMemcpyAsync(pkeys_ + next_gidx, pk_tmp_, nn * 8, hipMemcpyDeviceToDevice, st_));
      link_next_.swap(link_tmp_);
    }
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipStreamSynchronize(st_));
    KC_HIP_TRY(hipMemcpy(h_ctr_, d_ctr_, kCtrHead, hipMemcpyDeviceToHost));
    if (h_ctr_->overflow) {
      set_error("kc_shard tlc_order: a parent key outside its level");
      return -EIO;
    }
    return 0;
  }
  int tlc_locate(int level, uint64_t G, uint64_t* idx, bool* found) override {
    *found = false;
    if (!tlc_ || level < 1 || level > (int)level_base_.size()) {
      set_error("kc_shard tlc_locate: bad level %d", level);
      return -EINVAL;
    }
    KC_HIP_TRY(hipSetDevice(cfg_.device));
    const uint64_t b = level_base_[level - 1];
    const uint64_t cnt = level < (int)level_base_.size() ? level_base_[level] - b : n_;
    // (a level's G values are sorted: tlc_order)
    uint64_t lo = 0, hi = cnt;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) / 2;
      uint32_t v = 0;
      KC_HIP_TRY(hipMemcpy(&v, gpos_all_ + b + mid, 4, hipMemcpyDeviceToHost));
      if ((uint64_t)v < G) lo = mid + 1; else hi = mid;
    }
    if (lo < cnt) {
      uint32_t v = 0;
      KC_HIP_TRY(hipMemcpy(&v, gpos_all_ + b + lo, 4, hipMemcpyDeviceToHost));
      if ((uint64_t)v == G) {
        *idx = lo;
        *found = true;
      }
    }
    return 0;
  }

  int parent_key(int level, uint64_t idx, uint64_t* key) override {
    if (level < 1 || level > (int)level_base_.size()) {
      set_error("kc_shard_parent_key: bad level %d", level);
      return -EINVAL;
    }
    const uint64_t g = level_base_[level - 1] + idx;
    KC_HIP_TRY(hipMemcpy(key, pkeys_ + g, 8, hipMemcpyDeviceToHost));
    return 0;
  }

  int frontier_tuple(uint64_t idx, uint64_t* out) override {
    if (idx >= n_) { set_error("kc_shard_frontier_tuple: index"); return -EINVAL; }
    State s;
    KC_HIP_TRY(hipMemcpy(&s, cur_ + idx, sizeof(State), hipMemcpyDeviceToHost));
    M::to_tuple(s, out);
    return M::TUPLE_WORDS;
  }

  int result(kc_result* r) override {
    KC_HIP_TRY(hipMemcpy(h_ctr_, d_ctr_, sizeof(Counters), hipMemcpyDeviceToHost));
    memset(r, 0, sizeof *r);
    uint64_t gen = 0;
    for (int a = 0; a < A_COUNT; ++a) {
      r->act_gen[a] = h_ctr_->act_gen(a);
      r->act_dist[a] = h_ctr_->act_dist(a);
      gen += r->act_gen[a];
    }
    r->init = gen_init_;
    r->generated = gen;                 // successors generated by this rank's parents
    r->distinct = distinct_;
    r->fpset_slots = cs_.capacity();
    if (spill_) {
      ColdStats cst;
      sp_.cold.stats(&cst);
      unsigned long long hits = 0;
      KC_HIP_TRY(hipMemcpy(&hits, sp_.d_spctr, 8, hipMemcpyDeviceToHost));
      r->seen_flushes = sp_.flushes;
      r->seen_cold_fps = cst.keys;
      r->seen_cold_runs = cst.runs;
      r->seen_cold_queries = sp_.queries;
      r->seen_cold_hits = hits;
      r->seen_merges = cst.merges;
      r->seen_disk_bytes = cst.disk_written;
    }
    r->fpset_probes = h_ctr_->probes();
    r->batch_inserts = h_ctr_->settles();
    r->nlevels = level_;
    r->claim_mode = first_ ? 1 : tlc_ ? 2 : 0;
    r->deferred_states = deferred_states_;
    return 0;
  }

 private:
  kc_model_config cfg_;
  int rank_, world_;
  Flags flags_{};
  OwnedStream st_;   // (before every buffer: destroyed after them; set_stream: the caller's, not ours)
  DevClaimSet cs_;
  DeviceArray<State> cur_, next_;
  DeviceArray<unsigned long long> pkeys_;
  // expand: owner counts / scan, remote representatives, local claim tiles
  DeviceArray<uint8_t> cnt_;
  DeviceArray<uint32_t> off_, repmask_, newmask_, offsets_;
  DeviceArray<unsigned int> rcount_, rec_lk_;
  DeviceArray<unsigned long long> rec_fp_;
  CandOvf ovf_{};
  DeviceArray<unsigned long long> ovf_fp_;
  DeviceArray<unsigned int> ovf_lk_, ovf_tile_;
  DeviceArray<unsigned long long> d_ovf_cnt_;
  // insert: per received record
  DeviceArray<unsigned long long> rfp_;
  DeviceArray<unsigned int> flag_;
  DeviceArray<uint32_t> isnew_, ioff_;
  DeviceArray<uint8_t> scan_tmp_;
  // record staging (ShardArgs::stage; world > 1)
  DeviceArray<Rec> stage_;
  DeviceArray<unsigned long long> d_stage_cur_;
  DeviceArray<uint32_t> tcnt_, toff_;
  // owner x chunk sums of the staged record counts (k_owner_cscan; zeroed at
  // allocation, at every run's start and by each scan); KC_CHUNK_SCAN=0:
  // k_owner_tscan per tile
  bool ocscan_ = true, ocscan_level_ = false;
  DeviceArray<uint32_t> ocsum_;
  DeviceArray<unsigned long long> stoff_;
  bool stage_on_ = true, stage_level_ = false, staged_ = false;
  bool first_ = false;    // first-claim mode (cfg.first_claim)
  uint64_t stage_fallbacks_ = 0;       // levels packed the old way (staging estimate exceeded)
  double rec_ratio_ = 1.0;             // records sent per parent, last level (the staging estimate)
  // the tile-count insert path: own tiles' and record blocks' new-state counts, their scan
  bool tcount_ = true;
  DeviceArray<uint32_t> wtot_, woff_;
  // the deferred frontier (set_deferred; the native loop's counted levels)
  bool defer_on_ = false;
  bool cur_deferred_ = false;        // cur_ not built: link_cur_ into next_ (the previous frontier) / prev_rec_
  bool emitted_links_ = false;       // the last insert emitted links (advance swaps them in)
  bool rebuilt_ = false;             // this level's k_claim rebuilt its parents
  bool cand_est_ = false, next_cand_est_ = false;   // cand_ / next_cand_ estimated, not counted
  DeviceArray<unsigned long long> link_cur_, link_next_;
  DeviceArray<unsigned long long> pc_cur_, pc_prev_;   // plans of this / the previous level's parents
  const Rec* prev_rec_ = nullptr;    // the receive buffer the links point into
  const Rec* last_in_ = nullptr;     // the last insert's receive buffer
  uint64_t defer_err_ = ~0ull;       // expand_done: the rebuild's invariant key
  double succ_ratio_ = 5.0;          // successors per state, last counted (the estimates)
  bool gen_snap_ok_ = false;        // drop_last_expand can undo the last expand's act_gen
  uint64_t last_new_ = 0;            // the last insert's new states (drop_last_insert)
  uint64_t deferred_levels_ = 0, emit_retries_ = 0;
  uint64_t deferred_states_ = 0;   // this run's states rebuilt inside k_claim (kc_result.deferred_states)
  bool defer_check_ = false;         // KC_DEFER_CHECK (diagnostic)
  // TLC order (tlc_*): G of every state (parallel to pkeys_), the current /
  // next level's G -> local index map, the per-parent masks and scratch
  bool tlc_ = false;
  DeviceArray<uint32_t> gpos_all_;
  DeviceArray<uint32_t> gbits_cur_, grank_cur_, gbits_next_, grank_next_;
  DeviceArray<uint32_t> wmask_, wbase_, gnew_;
  DeviceArray<unsigned long long> link_tmp_, pk_tmp_;
  DeviceArray<unsigned long long> d_dchk_;
  DeviceArray<Counters> d_ctr_dbg_;
  DeviceArray<unsigned long long> pk_dbg_;
  DeviceArray<uint64_t> d_owner_base_;   // per-owner record totals (device / pinned host)
  PinnedArray<uint64_t> h_owner_base_;
  DeviceArray<Counters> d_ctr_;
  PinnedArray<Counters> h_ctr_;
  PinnedArray<Counters> h_exp_;        // expand's level head (kCtrHead bytes)
  uint64_t n_ = 0, next_n_ = 0, send_total_ = 0, gen_init_ = 0;
  uint64_t cand_ = 0, next_cand_ = 0, cand_total_ = 0;   // successors of the frontier
  uint64_t init_err_ = ~0ull;
  uint64_t init_key_ = ~0ull;       // init_error(): init_err_ as init() found it
  // expand_dev -> expand_done: the Init-state key taken, nothing launched
  // that needs a sync, no claims this level
  uint64_t dev_init_err_ = ~0ull;
  bool dev_empty_ = false, dev_zero_ = false;
  int level_ = 0;
  std::vector<uint64_t> level_base_;
  OwnedEvent ev_[2];
  bool async_pack_ = false;
  // device-driven narrow levels
  DeviceArray<SNCtl> d_snc_;
  PinnedArray<SNCtl> h_snc_;
  DeviceArray<SNScratch> d_sns_;
  DeviceArray<uint64_t> sn_send_, sn_recv_;
  uint32_t sn_cap_ = SN_SLOT_DEFAULT;
  uint64_t sn_n0_ = 0;
  double claim_ms_ = 0;
  uint64_t claim_launches_ = 0, claim_parents_ = 0;
  uint64_t distinct_ = 0;           // new states this rank owns (cs_.count is the hot table's, spilling)
  // seen-set spill
  bool spill_ = false;
  std::string spill_dir_;
  SeenSpill<uint64_t> sp_;
  uint64_t hot_hard_ = 0;           // most hot entries a level may leave (7/8 of the slots)
  double sp_ratio_ = 1.0;           // hot slots filled per successor, last level
};

std::unique_ptr<ShardBase> make_shard(const kc_model_config& cfg, int rank, int world) {
#define KC_MAKE(a, b, c)                                                   \
  if (cfg.nc == a && cfg.np == b && cfg.ns == c)                           \
    return std::unique_ptr<ShardBase>(new ShardT<Model<a, b, c>>(cfg, rank, world));
  KC_FOR_EACH_MODEL(KC_MAKE)
#undef KC_MAKE
  return nullptr;
}

}  // namespace kc

using namespace kc;

extern "C" {

int kc_shard_create(const kc_model_config* cfg, int rank, int world, kc_shard** out) {
  if (!cfg || !out) { set_error("kc_shard_create: NULL"); return -EINVAL; }
  *out = nullptr;
  if (cfg->symmetry) {
    set_error("kc_shard_create: symmetry is not supported in the sharded loop (the owner projection is not "
              "orbit-invariant)");
    return -EINVAL;
  }
  if (con_active(cfg->constraint_stored, cfg->constraint_inflight, cfg->action_constraints)) {
    set_error("kc_shard_create: constraints are not supported in the sharded loop (single-GPU engine only)");
    return -EINVAL;
  }
  if (cfg->action_properties) {
    set_error("kc_shard_create: action properties are not supported in the sharded loop (single-GPU engine only)");
    return -EINVAL;
  }
  auto impl = make_shard(*cfg, rank, world);
  if (!impl) {
    set_error("kc_shard_create: unsupported model nc=%d np=%d ns=%d", cfg->nc, cfg->np, cfg->ns);
    return -EINVAL;
  }
  KC_TRY(impl->setup());
  *out = new kc_shard{std::move(impl)};
  return 0;
}
void kc_shard_destroy(kc_shard* s) { delete s; }
int kc_shard_init(kc_shard* s, uint64_t* n_local) {
  if (!s || !n_local) { set_error("kc_shard_init: NULL"); return -EINVAL; }
  return s->impl->init(n_local);
}

int kc_shard_init_error(kc_shard* s, uint64_t* key) {
  if (!s || !key) { set_error("kc_shard_init_error: NULL"); return -EINVAL; }
  *key = s->impl->init_error();
  return 0;
}
int kc_shard_set_stream(kc_shard* s, void* stream) {
  if (!s) { set_error("kc_shard_set_stream: NULL"); return -EINVAL; }   // stream 0: the default stream
  return s->impl->set_stream((hipStream_t)stream);
}
int kc_shard_expand(kc_shard* s, uint64_t* counts, uint64_t* err_key) {
  if (!s || !counts || !err_key) { set_error("kc_shard_expand: NULL"); return -EINVAL; }
  return s->impl->expand(counts, err_key);
}
uint64_t kc_shard_record_bytes(kc_shard* s) { return s ? s->impl->record_bytes() : 0; }
int kc_shard_pack(kc_shard* s, void* send_dev) {
  if (!s) { set_error("kc_shard_pack: NULL"); return -EINVAL; }
  return s->impl->pack(send_dev);
}
int kc_shard_insert(kc_shard* s, const void* recv_dev, uint64_t n_records, uint64_t* n_new,
                    uint64_t* err_key) {
  if (!s || !n_new || !err_key) { set_error("kc_shard_insert: NULL"); return -EINVAL; }
  return s->impl->insert(recv_dev, n_records, n_new, err_key);
}
int kc_shard_advance(kc_shard* s) {
  if (!s) { set_error("kc_shard_advance: NULL"); return -EINVAL; }
  return s->impl->advance();
}
int kc_shard_parent_key(kc_shard* s, int level, uint64_t idx, uint64_t* key) {
  if (!s || !key) { set_error("kc_shard_parent_key: NULL"); return -EINVAL; }
  return s->impl->parent_key(level, idx, key);
}
int kc_shard_frontier_tuple(kc_shard* s, uint64_t idx, uint64_t* out) {
  if (!s || !out) { set_error("kc_shard_frontier_tuple: NULL"); return -EINVAL; }
  return s->impl->frontier_tuple(idx, out);
}
int kc_shard_result(kc_shard* s, kc_result* r) {
  if (!s || !r) { set_error("kc_shard_result: NULL"); return -EINVAL; }
  return s->impl->result(r);
}
int kc_shard_claim_times(kc_shard* s, double* ms, uint64_t* launches, uint64_t* parents) {
  if (!s || !ms || !launches || !parents) { set_error("kc_shard_claim_times: NULL"); return -EINVAL; }
  s->impl->claim_times(ms, launches, parents);
  return 0;
}
int kc_shard_owner(uint64_t fp, int world) {
  if (world < 1) return -EINVAL;
  return (int)(((unsigned __int128)((fp & 0x7fffffffffffffffull) << 1) * (uint64_t)world) >> 64);
}

}  // extern "C"
