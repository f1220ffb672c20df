// liveness.h — temporal properties under WF_vars(Next) or per-process weak
// fairness: the state predicates the elimination runs on and the process of a
// step, as KC_HD code shared by the kernels (liveness.hip) and the host
// (kc_live_stay, kc_live_step_process).  include/kubecheck.h, "Liveness", has the
// semantics; DESIGN.md §4.7 the layout.
//
// Every property reduces to one question about a predicate `stay`: is there a
// behaviour of Spec that reaches a stay state and remains in stay states for
// ever?  live_stay evaluates it on the packed state.
#pragma once
#include <stdint.h>

#include "kubeapi_spec.h"

namespace kc {

// Property ids (kc_live_config.property).  0 and 1 are KubeAPI.tla's own
// (:798, :806); 2 and 3 are build-defined, as NoLostUpdate is among the
// invariants: on this spec 0 and 1 never make the elimination remove a state,
// so these two give the trim rounds something to do.
enum LiveProp : int {
  LP_ReconcileCompletes = 0,   // sR ~> ~sR                     stay = shouldReconcile[Client]
  LP_CleansUpProperly = 1,     // []~sR ~> no Secret/foo stored stay = ~sR /\ apiState has a Secret/foo
  LP_ClientRestarts = 2,       // []<>(pc[Client] = "CStart")   stay = pc[Client] # "CStart"
  LP_SomeActorRestarts = 3,    // []<>(some actor at its start) stay = no actor at its start label
  LP_COUNT = 4
};

// Properties 0-2 speak of "the" client: they need exactly one.
KC_HD bool live_prop_ok(int nc, int prop) {
  return prop >= 0 && prop < LP_COUNT && (prop == LP_SomeActorRestarts || nc == 1);
}

// Fairness conditions (kc_live_config.fairness).
enum LiveFairness : int {
  LF_Next = 0,      // WF_vars(Next)
  LF_Process = 1    // /\_p WF_vars(step of process p): PlusCal's `fair process`
};

// The process that takes the steps of a slot (kubeapi_spec.h's slot order):
// actor a is process a (slot a = its API / ListAPI procedure steps, slot A + a
// = its own labels; pc makes the three mutually exclusive), server k is
// process A + k.  A model has P = A + NS <= 5 processes.
template <class M>
KC_HD int live_slot_process(int slot) {
  return slot < M::A ? slot : slot < 2 * M::A ? slot - M::A : M::A + (slot - 2 * M::A);
}

// stay(s) of property `prop`; live_prop_ok(M::NC, prop) must hold.  The
// lostUpdate ghost (bit 63 of word 0) is not part of apiState: id_mask covers
// U bits only.
template <class M>
KC_HD bool live_stay(const typename M::State& s, int prop) {
  if (prop == LP_SomeActorRestarts) {
    bool none = true;
    static_for<M::A>([&](auto AI) {
      constexpr int a = AI;
      if (M::template pc<a>(s) == (M::is_client(a) ? L_CStart : L_PVCStart)) none = false;
    });
    return none;
  }
  if constexpr (M::NC == 1) {
    const bool sr = M::template fld<0>(s, M::F_SR, 1) != 0;
    if (prop == LP_ReconcileCompletes) return sr;
    if (prop == LP_CleansUpProperly) return !sr && (s.w[0] & M::id_mask(ID_Secret)) != 0;
    return M::template pc<0>(s) != L_CStart;
  }
  return false;
}

}  // namespace kc
