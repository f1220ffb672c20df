// claim_selftest_launch.h — the sharded k_claim launch of the test harnesses
// (claim_selftest.hip kind 3; shard_selftest.hip's insert kinds): shard.hip's
// dynamic LDS for the owner counts, base 0, no deferred frontier.  Nothing of
// the product path includes this file.
#pragma once
#include "claim_launch.h"

namespace kc {
namespace selftest {

template <class M, bool TLC = false, bool FIRST = false, bool C8 = false>
void launch_shard_claim(unsigned tiles, const typename M::State* cur, uint64_t n, const Flags& f, int check_deadlock,
                        const DevClaimSet& cs, uint32_t succ_level, const ClaimBufs& bufs, const ShardArgs& sa) {
  const size_t dyn = (size_t)(CLAIM_TILE + ((sa.world + 3) / 4) * CLAIM_TILE) * sizeof(unsigned int);
  launch_claim<M, 0, true, 1, TLC, FIRST, C8>(nullptr, tiles, dyn, cur, n, 0, f, check_deadlock, cs, succ_level, bufs,
                                              sa, DeferArgs{});
}

}  // namespace selftest
}  // namespace kc
