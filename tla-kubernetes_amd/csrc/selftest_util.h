// selftest_util.h — host helpers shared by the test-only device harnesses
// (spill_selftest.hip, emit_selftest.hip, coldset_selftest.hip): an untyped device buffer, the
// upload of a host array, and the check that packed parents are states a
// kernel may plan and apply.  Nothing of the product path includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kc_common.h"
#include "kubeapi_spec.h"
#include "owned.h"

namespace kc {
namespace selftest {

// bytes, read as whatever the kernel takes
struct DevBuf : DeviceArray<uint8_t> {
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

inline int upload(DevBuf& d, const void* src, uint64_t bytes) {
  KC_TRY(d.alloc(bytes ? bytes : 8));
  if (bytes) KC_HIP_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

// The packed states are states of the lowered domain (they survive the round
// trip through the canonical tuple) that raise no Assert under `f`; tot[i] =
// successors of state i, capped like the kernels cap them.  Returns nullptr,
// or what is wrong with the input.
template <class M>
const char* check_states(const uint64_t* packed, uint64_t n, const Flags& f, std::vector<int>& tot) {
  tot.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    typename M::State s, r;
    for (int k = 0; k < M::W; ++k) s.w[k] = packed[i * M::W + k];
    uint64_t tup[M::TUPLE_WORDS];
    M::to_tuple(s, tup);
    bool same = M::from_tuple(tup, r);
    for (int k = 0; same && k < M::W; ++k) same = r.w[k] == s.w[k];
    if (!same) return "a parent is not a packed state of the model";
    const typename M::Plan pl = M::plan(s, f);
    if (pl.fail_pos >= 0) return "a parent raises an Assert failure";
    tot[i] = pl.total > M::MAXSUCC ? M::MAXSUCC : pl.total;
  }
  return nullptr;
}

}  // namespace selftest
}  // namespace kc
