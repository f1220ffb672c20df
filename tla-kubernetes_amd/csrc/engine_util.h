// engine_util.h — small host helpers shared by the single-GPU engine and the
// sharded (multi-GPU) stages.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "kubeapi_spec.h"
#include "owned.h"

namespace kc {

// Run-time switches of a model config (constants, seeded variant,
// invariants to check: 0 = none, as TLC with no INVARIANT in the .cfg).
inline Flags flags_of(const kc_model_config& c) {
  Flags f{c.can_fail, c.can_timeout, c.variant};
  f.inv_mask = c.invariants & 7;
  f.con_stored = c.constraint_stored;
  f.con_inflight = c.constraint_inflight;
  f.act_con = c.action_constraints;
  f.act_props = c.action_properties;
  return f;
}

}  // namespace kc
