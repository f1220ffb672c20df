// claim_launch.h — the one spelling of a k_claim launch (engine.hip and
// shard.hip differ in the variant and in a few arguments only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine_kernels.h"
#include "fpset_host.h"

namespace kc {

// One k_claim launch.  The template arguments choose the variant exactly as
// k_claim's own do; what every launch shares is spelled once here.
struct ClaimBufs {
  uint32_t* scratch;            // ABL builds only
  unsigned int* rcount;
  unsigned long long* rec_fp;
  unsigned int* rec_lk;
  uint32_t* newmask;
  Counters* ctr;
};
template <class M, int ABL = 0, bool SH = false, int OWN = SH ? 1 : 0, bool TLC = false, bool FIRST = false,
          bool C8 = false>
void launch_claim(hipStream_t st, unsigned tiles, size_t dyn_lds, const typename M::State* cur, uint64_t n,
                  uint64_t base, const Flags& f, int check_deadlock, const DevClaimSet& cs, uint32_t succ_level,
                  const ClaimBufs& b, const ShardArgs& sh, const DeferArgs& df = DeferArgs{}) {
  hipLaunchKernelGGL((k_claim<M, ABL, SH, OWN, TLC, FIRST, C8>), dim3(tiles), dim3(CLAIM_TILE), dyn_lds, st, cur, n,
                     base, f, check_deadlock, cs.t, cs.nslots, succ_level, b.scratch, b.rcount, b.rec_fp, b.rec_lk,
                     b.newmask, b.ctr, sh, df);
}

}  // namespace kc
