// engine_util.h — small host helpers shared by the single-GPU engine and the
// sharded (multi-GPU) stages.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "../../include/kubecheck.h"
#include "kc_common.h"
#include "kubeapi_spec.h"

namespace kc {

// An owned device buffer of `cap` elements (move-only; the destructor frees).
// It reads as the T* it holds, so launches and copies take it as they took
// the raw pointer.  The owner makes its device current before its buffers
// are destroyed, and destroys its stream after them.
template <class T>
struct DeviceArray {
  T* p = nullptr;
  uint64_t cap = 0;

  DeviceArray() = default;
  DeviceArray(DeviceArray&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DeviceArray& operator=(DeviceArray&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  ~DeviceArray() { reset(); }

  operator T*() const { return p; }
  T* operator->() const { return p; }
  void swap(DeviceArray& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }

  // exactly n elements, once (control blocks and other fixed-size buffers)
  int alloc(uint64_t n) {
    if (p) return 0;
    KC_HIP_TRY(hipMalloc(&p, n * sizeof(T)));
    cap = n;
    return 0;
  }
  // exactly n elements in place of what it held (the owner's own growth
  // rule; nothing may still use the old block, contents are not kept)
  int renew(uint64_t n) {
    if (p) KC_HIP_TRY(hipFree(p));
    p = nullptr;
    cap = 0;
    return alloc(n);
  }
  // Grow to >= need elements (doubling); keep contents if asked.
  int grow(uint64_t need, hipStream_t st, bool keep = false) {
    if (need <= cap) return 0;
    uint64_t nc = cap ? cap : 1024;
    while (nc < need) nc *= 2;
    DeviceArray<T> nb;
    KC_HIP_TRY(hipMalloc(&nb.p, nc * sizeof(T)));
    nb.cap = nc;
    // (a failure from here on frees the new block: nb goes out of scope)
    if (keep && p && cap) KC_HIP_TRY(hipMemcpyAsync(nb.p, p, cap * sizeof(T), hipMemcpyDeviceToDevice, st));
    if (p) {
      KC_HIP_TRY(hipStreamSynchronize(st));
      KC_HIP_TRY(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    swap(nb);
    return 0;
  }
  // The same without doubling: capacity need + 1/8 (buffers sized by a
  // level's bound, where doubling would waste up to half of a large one);
  // contents are not kept, and the old block goes before the new one comes
  int grow_tight(uint64_t need, hipStream_t st) {
    if (need <= cap) return 0;
    const uint64_t nc = need + need / 8 + 1024;
    if (p) {
      KC_HIP_TRY(hipStreamSynchronize(st));
      KC_HIP_TRY(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    KC_HIP_TRY(hipMalloc(&p, nc * sizeof(T)));
    cap = nc;
    return 0;
  }
};

// The same for pinned host memory that kernels may write directly (the trace
// file with kc_model_config.trace_host); contents are always kept.
template <class T>
struct PinnedArray {
  T* p = nullptr;
  uint64_t cap = 0;

  PinnedArray() = default;
  PinnedArray(PinnedArray&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  PinnedArray& operator=(PinnedArray&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  PinnedArray(const PinnedArray&) = delete;
  PinnedArray& operator=(const PinnedArray&) = delete;
  ~PinnedArray() { reset(); }

  operator T*() const { return p; }
  T* operator->() const { return p; }
  void swap(PinnedArray& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }

  int alloc(uint64_t n) {
    if (p) return 0;
    KC_HIP_TRY(hipHostMalloc(&p, n * sizeof(T)));
    cap = n;
    return 0;
  }
  int renew(uint64_t n) {
    if (p) KC_HIP_TRY(hipHostFree(p));
    p = nullptr;
    cap = 0;
    return alloc(n);
  }
  int grow(uint64_t need, hipStream_t st) {
    if (need <= cap) return 0;
    uint64_t nc = cap ? cap : 1024;
    while (nc < need) nc *= 2;
    PinnedArray<T> nb;
    KC_HIP_TRY(hipHostMalloc(&nb.p, nc * sizeof(T)));
    nb.cap = nc;
    KC_HIP_TRY(hipStreamSynchronize(st));          // kernels may still write the old buffer
    if (p) {
      memcpy(nb.p, p, cap * sizeof(T));
      KC_HIP_TRY(hipHostFree(p));
      p = nullptr;
      cap = 0;
    }
    swap(nb);
    return 0;
  }
};

// The trace file (parent index + ordinal per state): in HBM, or in pinned
// host RAM that kernels store into directly (kc_model_config.trace_host).
// One of the two kinds is ever allocated.
struct TraceFile {
  DeviceArray<unsigned long long> d_parent;
  DeviceArray<uint8_t> d_ord;
  PinnedArray<unsigned long long> h_parent;
  PinnedArray<uint8_t> h_ord;

  unsigned long long* parent() const { return h_parent.p ? h_parent.p : d_parent.p; }
  uint8_t* ord() const { return h_ord.p ? h_ord.p : d_ord.p; }
  uint64_t cap() const {
    return h_parent.p ? std::min(h_parent.cap, h_ord.cap) : std::min(d_parent.cap, d_ord.cap);
  }
  int grow(bool on_host, uint64_t need, hipStream_t st, bool keep) {
    if (on_host) {
      KC_TRY(h_parent.grow(need, st));
      return h_ord.grow(need, st);
    }
    KC_TRY(d_parent.grow(need, st, keep));
    return d_ord.grow(need, st, keep);
  }
};

// A stream that is destroyed with its holder.  Declared before an owner's
// buffers it is destroyed after them: after their last use.
struct OwnedStream {
  hipStream_t s = nullptr;
  bool own = true;              // false: the caller's stream (never destroyed here)
  OwnedStream() = default;
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  ~OwnedStream() {
    if (s && own) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};

// Run-time switches of a model config (constants, seeded variant,
// invariants to check: 0 = none, as TLC with no INVARIANT in the .cfg).
inline Flags flags_of(const kc_model_config& c) {
  Flags f{c.can_fail, c.can_timeout, c.variant};
  f.inv_mask = c.invariants & 7;
  return f;
}

}  // namespace kc
