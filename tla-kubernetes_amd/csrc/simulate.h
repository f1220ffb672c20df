// simulate.h — simulation mode (TLC -simulate): the counter-based RNG and one
// step of a random walk, as KC_HD code shared by the walk kernel
// (simulate.hip) and the host replay (kc_sim_replay, spec_abi.hip).
//
// A walk's random choices are a pure function of (seed, walk, step), so the
// GPU stores no trace: the host replays any walk into its full behaviour
// (include/kubecheck.h, "Simulation", has the semantics).
#pragma once
#include <stdint.h>

#include "kubeapi_spec.h"

namespace kc {

// How a walk ended.  1-3 are kc_result.err_kind's values (ErrKind).
enum SimKind : int { SIM_RUNNING = 0, SIM_ASSERT = 1, SIM_INVARIANT = 2, SIM_DEADLOCK = 3,
                     SIM_DEPTH = 4, SIM_TERMINATED = 5, SIM_NKIND = 6 };

// splitmix64's finaliser over a Weyl step: a bijection of 64-bit words
KC_HD uint64_t sim_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// K(w) = mix(mix(seed) ^ w); r(w, k) = mix(K(w) ^ k)
KC_HD uint64_t sim_key(uint64_t seed_mixed, uint64_t walk) { return sim_mix(seed_mixed ^ walk); }
KC_HD uint64_t sim_rand_key(uint64_t key, uint64_t k) { return sim_mix(key ^ k); }
// floor(r * n / 2^64)
KC_HD uint64_t sim_pick(uint64_t r, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, n);
#else
  return (uint64_t)(((unsigned __int128)r * n) >> 64);
#endif
}

// One status word per walk: kind, what failed, and k = the index of the
// walk's current state (it has k + 1 states; k < KC_SIM_MAX_DEPTH = 65535).
//   bits 0-2 kind, 3-7 action (assertion) or invariant index, 8-11 the
//   failing action's process, 16-31 k
KC_HD uint32_t sim_status(int kind, int info, int self, uint32_t k) {
  return (uint32_t)kind | ((uint32_t)info << 3) | ((uint32_t)self << 8) | (k << 16);
}
KC_HD int sim_status_kind(uint32_t st) { return (int)(st & 7); }
KC_HD int sim_status_info(uint32_t st) { return (int)((st >> 3) & 31); }
KC_HD int sim_status_self(uint32_t st) { return (int)((st >> 8) & 15); }
KC_HD uint32_t sim_status_k(uint32_t st) { return st >> 16; }

// Successor t of a plan -> (slot, index within the slot); M::locate with a
// compile-time bound.
template <class M>
KC_HD void sim_locate(const typename M::Plan& pl, int t, int& slot, int& j) {
  slot = 0;
  j = t;
  bool done = false;
  static_for<M::NSLOT>([&](auto SI) {
    const int c = (int)((pl.counts >> (6 * (int)SI)) & 63);
    if (!done) {
      if (j < c) { done = true; slot = (int)SI; }
      else j -= c;
    }
  });
}

// What one step of a walk at its state s = s_k does.
struct SimStep {
  int kind;     // SIM_RUNNING: x = s_{k+1} was chosen; else the walk ends at s
  int info;     // the chosen / failing action, or the violated invariant
  int self;     // assertion: the failing action's process
  int who;      // SIM_RUNNING: the process whose word the action rewrote
};

// Steps 1-5 of the walk (include/kubecheck.h): invariants of s, the depth
// limit, plan (Assert), deadlock / termination, then successor
// pick(r(w, k + 1), total) in kc_spec_successors order into x.
template <class M>
KC_HD SimStep sim_step(const typename M::State& s, uint32_t k, uint64_t key, const Flags& f, int depth,
                       int check_deadlock, typename M::State& x) {
  const int inv = M::check(s, f.inv_mask);
  if (inv >= 0) return SimStep{SIM_INVARIANT, inv, 0, 0};
  if ((int)(k + 1) >= depth) return SimStep{SIM_DEPTH, 0, 0, 0};
  const typename M::Plan pl = M::plan(s, f);
  if (pl.fail_pos >= 0) {
    const int fs = pl.fail_slot;
    const int self = fs < M::A ? fs : fs < 2 * M::A ? fs - M::A : M::A + (fs - 2 * M::A);
    return SimStep{SIM_ASSERT, M::slot_action(s, fs), self, 0};
  }
  if (pl.total == 0) return SimStep{check_deadlock ? SIM_DEADLOCK : SIM_TERMINATED, 0, 0, 0};
  const int t = (int)sim_pick(sim_rand_key(key, (uint64_t)k + 1), (uint64_t)pl.total);
  int slot, j, who;
  sim_locate<M>(pl, t, slot, j);
  M::apply(s, slot, j, f, x, who);
  return SimStep{SIM_RUNNING, M::slot_action(s, slot), 0, who};
}

}  // namespace kc
