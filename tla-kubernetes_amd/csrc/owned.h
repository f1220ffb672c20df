// owned.h — the handles the host side owns: device and pinned buffers,
// streams and events.  Each is move-only and released by its destructor, so
// an early return frees what it had made.  The one rule for a holder: make
// its device current before its members are destroyed, and declare its stream
// before (so it is destroyed after) the buffers and events that use it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "kc_common.h"

namespace kc {

struct DeviceMem {
  static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t put(void* p) { return hipFree(p); }
};
struct PinnedMem {
  static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static hipError_t put(void* p) { return hipHostFree(p); }
};

// An owned buffer of `cap` elements.  It reads as the T* it holds, so
// launches and copies take it as they took the raw pointer.
template <class T, class Mem>
struct OwnedArray {
  T* p = nullptr;
  uint64_t cap = 0;

  OwnedArray() = default;
  OwnedArray(OwnedArray&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  OwnedArray& operator=(OwnedArray&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  OwnedArray(const OwnedArray&) = delete;
  OwnedArray& operator=(const OwnedArray&) = delete;
  ~OwnedArray() { reset(); }

  operator T*() const { return p; }
  T* operator->() const { return p; }
  void swap(OwnedArray& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  void reset() {
    if (p) (void)Mem::put(p);
    p = nullptr;
    cap = 0;
  }

  // exactly n elements, once (control blocks and other fixed-size buffers)
  int alloc(uint64_t n) {
    if (p) return 0;
    KC_HIP_TRY(Mem::get((void**)&p, n * sizeof(T)));
    cap = n;
    return 0;
  }
  // exactly n elements in place of what it held (the owner's own growth
  // rule; nothing may still use the old block, contents are not kept)
  int renew(uint64_t n) {
    if (p) KC_HIP_TRY(Mem::put(p));
    p = nullptr;
    cap = 0;
    return alloc(n);
  }

 protected:
  // the doubled capacity that holds `need` elements
  uint64_t doubled(uint64_t need) const {
    uint64_t nc = cap ? cap : 1024;
    while (nc < need) nc *= 2;
    return nc;
  }
};

template <class T>
struct DeviceArray : OwnedArray<T, DeviceMem> {
  using OwnedArray<T, DeviceMem>::p;
  using OwnedArray<T, DeviceMem>::cap;

  // Grow to >= need elements (doubling); keep contents if asked.
  int grow(uint64_t need, hipStream_t st, bool keep = false) {
    if (need <= cap) return 0;
    DeviceArray<T> nb;
    KC_TRY(nb.alloc(this->doubled(need)));
    // (a failure from here on frees the new block: nb goes out of scope)
    if (keep && p && cap) KC_HIP_TRY(hipMemcpyAsync(nb.p, p, cap * sizeof(T), hipMemcpyDeviceToDevice, st));
    if (p) KC_HIP_TRY(hipStreamSynchronize(st));
    this->swap(nb);
    return 0;
  }
  // The same without doubling: capacity need + 1/8 (buffers sized by a
  // level's bound, where doubling would waste up to half of a large one);
  // contents are not kept, and the old block goes before the new one comes
  int grow_tight(uint64_t need, hipStream_t st) {
    if (need <= cap) return 0;
    if (p) KC_HIP_TRY(hipStreamSynchronize(st));
    return this->renew(need + need / 8 + 1024);
  }
};

// Pinned host memory that kernels may write directly (the trace file with
// kc_model_config.trace_host); grow always keeps the contents.
template <class T>
struct PinnedArray : OwnedArray<T, PinnedMem> {
  using OwnedArray<T, PinnedMem>::p;
  using OwnedArray<T, PinnedMem>::cap;

  int grow(uint64_t need, hipStream_t st) {
    if (need <= cap) return 0;
    PinnedArray<T> nb;
    KC_TRY(nb.alloc(this->doubled(need)));
    KC_HIP_TRY(hipStreamSynchronize(st));          // kernels may still write the old buffer
    if (p) memcpy(nb.p, p, cap * sizeof(T));
    this->swap(nb);
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

// A stream that is destroyed with its holder, or a caller's stream that is
// only borrowed.
class OwnedStream {
 public:
  OwnedStream() = default;
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  ~OwnedStream() {
    if (s_ && own_) (void)hipStreamDestroy(s_);
  }
  operator hipStream_t() const { return s_; }
  bool owned() const { return own_; }

  // hipStreamNonBlocking, or hipStreamDefault for a stream that orders with
  // the legacy default stream
  int create(unsigned flags) {
    if (s_) return 0;
    KC_HIP_TRY(hipStreamCreateWithFlags(&s_, flags));
    return 0;
  }
  // run on the caller's stream from now on (never destroyed here)
  int borrow(hipStream_t st) {
    if (s_ && own_) KC_HIP_TRY(hipStreamDestroy(s_));
    s_ = st;
    own_ = false;
    return 0;
  }

 private:
  hipStream_t s_ = nullptr;
  bool own_ = true;
};

// An event, created on request.
struct OwnedEvent {
  hipEvent_t e = nullptr;

  OwnedEvent() = default;
  OwnedEvent(OwnedEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  OwnedEvent& operator=(OwnedEvent&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~OwnedEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  int create(unsigned flags = hipEventDefault) {
    if (!e) KC_HIP_TRY(hipEventCreateWithFlags(&e, flags));
    return 0;
  }
};

}  // namespace kc
