// coldset_selftest.hip — test-only C ABI over the seen-set's cold tier
// (kc::ColdSet, coldset.h) and its key mix (kc_coldset_*, kc_cold_key_selftest;
// include/kubecheck.h "tests").  The suite drives a ColdSet with runs and
// query sets of its own making (tests/test_gpu_coldset.py) and compares every
// answer and statistic with the host model tests/cold_model.py.
// The harness, not the tests, keeps the kernels inside their buffers: keys
// must be strictly ascending, queries ascending, counts in [1, 2^21], and
// after a failed add (which leaves a run without a directory in the set)
// nothing is probed or read until clear.  Nothing of the product path calls
// this file.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/kubecheck.h"
#include "coldset.h"
#include "kc_common.h"
#include "selftest_util.h"

namespace kc {
namespace {

constexpr uint64_t kColdTestMax = 1ull << 21;     // keys per add, queries per probe

struct ColdHarness {
  OwnedStream st;                   // (before the set: destroyed after its buffers)
  ColdSet cs;
  bool failed = false;              // an add_run failed: no probe / all_keys until clear
};

using selftest::DevBuf;

__global__ void k_cold_key_selftest(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n, int unkey) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = unkey ? cold_unkey(in[i]) : cold_key(in[i]);
}

int have_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("%s: no HIP device", who);
    return -ENODEV;
  }
  return 0;
}

// the words of a are ascending (strictly, if strict)
bool ascending(const uint64_t* a, uint64_t n, bool strict) {
  for (uint64_t i = 1; i < n; ++i)
    if (strict ? a[i - 1] >= a[i] : a[i - 1] > a[i]) return false;
  return true;
}

}  // namespace
}  // namespace kc

using namespace kc;

extern "C" {

int kc_coldset_create(uint64_t meta_hbm_bytes, uint64_t host_bytes, const char* dir, uint64_t window_keys,
                      int bloom_bits, int cache_keys, int merge_div, int merge_threads, void** out) {
  if (!out || bloom_bits < 0 || bloom_bits > 64 || merge_div < 0 || merge_threads < 1 || merge_threads > 64 ||
      window_keys < 64 || (window_keys & 7) || window_keys > (1ull << 23)) {
    set_error("kc_coldset_create: bad argument (window_keys a multiple of 8 in [64, 2^23], bloom_bits 0-64, "
              "merge_div >= 0, merge_threads 1-64)");
    return -EINVAL;
  }
  *out = nullptr;
  KC_TRY(have_device("kc_coldset_create"));
  ColdHarness* h = new (std::nothrow) ColdHarness;
  if (!h) {
    set_error("kc_coldset_create: out of memory");
    return -ENOMEM;
  }
  ColdSet::Config c;
  c.meta_hbm_bytes = meta_hbm_bytes;
  c.host_bytes = host_bytes;
  c.dir = dir ? dir : "";
  c.window_keys = window_keys;
  c.merge_threads = merge_threads;
  c.bloom_bits = bloom_bits;
  c.cache_keys = cache_keys != 0;
  c.merge_div = merge_div;
  int rc = h->cs.init(c);
  if (rc == 0 && h->st.create(hipStreamDefault) < 0) {
    set_error("kc_coldset_create: cannot create a stream");
    rc = -EIO;
  }
  if (rc < 0) {
    delete h;
    return rc;
  }
  *out = h;
  return 0;
}

int kc_coldset_add_run(void* hv, const uint64_t* keys, uint64_t n) {
  ColdHarness* h = static_cast<ColdHarness*>(hv);
  if (!h || !keys || n == 0 || n > kColdTestMax) {
    set_error("kc_coldset_add_run: bad argument (n %llu: 1 to %llu keys)", (unsigned long long)n,
              (unsigned long long)kColdTestMax);
    return -EINVAL;
  }
  if (!ascending(keys, n, true)) {
    set_error("kc_coldset_add_run: keys are not strictly ascending");
    return -EINVAL;
  }
  if (h->failed) {
    set_error("kc_coldset_add_run: an earlier add failed; clear first");
    return -EINVAL;
  }
  DevBuf d;
  KC_TRY(d.alloc(n * 8));
  KC_HIP_TRY(hipMemcpy(d.p, keys, n * 8, hipMemcpyHostToDevice));
  const int rc = h->cs.add_run(d.as<const uint64_t>(), n, h->st);
  (void)hipStreamSynchronize(h->st);       // (a failed add may have left its copy in flight)
  if (rc < 0) h->failed = true;
  return rc;
}

int kc_coldset_probe(void* hv, const uint64_t* q, uint64_t m, uint8_t* found, uint64_t* hits) {
  ColdHarness* h = static_cast<ColdHarness*>(hv);
  if (!h || !q || !found || !hits || m == 0 || m > kColdTestMax) {
    set_error("kc_coldset_probe: bad argument (m %llu: 1 to %llu queries)", (unsigned long long)m,
              (unsigned long long)kColdTestMax);
    return -EINVAL;
  }
  if (!ascending(q, m, false)) {
    set_error("kc_coldset_probe: queries are not ascending");
    return -EINVAL;
  }
  if (h->failed) {
    set_error("kc_coldset_probe: an add failed, the set holds a run without a directory; clear first");
    return -EINVAL;
  }
  DevBuf dq, df, dh;
  KC_TRY(dq.alloc(m * 8));
  KC_TRY(df.alloc(m));
  KC_TRY(dh.alloc(8));
  KC_HIP_TRY(hipMemcpy(dq.p, q, m * 8, hipMemcpyHostToDevice));
  KC_HIP_TRY(hipMemcpy(df.p, found, m, hipMemcpyHostToDevice));
  KC_HIP_TRY(hipMemcpy(dh.p, hits, 8, hipMemcpyHostToDevice));
  const int rc = h->cs.probe(dq.as<const uint64_t>(), m, df.p, dh.as<unsigned long long>(), h->st);
  KC_HIP_TRY(hipStreamSynchronize(h->st));
  KC_TRY(rc);
  KC_HIP_TRY(hipMemcpy(found, df.p, m, hipMemcpyDeviceToHost));
  KC_HIP_TRY(hipMemcpy(hits, dh.p, 8, hipMemcpyDeviceToHost));
  return 0;
}

int kc_coldset_stats(void* hv, uint64_t* out) {
  ColdHarness* h = static_cast<ColdHarness*>(hv);
  if (!h || !out) {
    set_error("kc_coldset_stats: NULL");
    return -EINVAL;
  }
  ColdStats s;
  h->cs.stats(&s);
  const uint64_t v[KC_COLDSET_NSTATS] = {
      s.runs,        s.runs_disk,   s.keys,         s.host_bytes,      s.disk_bytes,   s.meta_bytes,  s.peak_meta_bytes,
      s.merges,      s.merged_keys, s.disk_written, s.disk_read,       s.windows_skipped, s.cached_runs, s.cached_keys,
      s.cache_bytes, s.cache_uploaded, s.filter_tests, s.filter_passed, s.merge_probes};
  for (int i = 0; i < KC_COLDSET_NSTATS; ++i) out[i] = v[i];
  return 0;
}

int64_t kc_coldset_all_keys(void* hv, uint64_t* out, uint64_t cap) {
  ColdHarness* h = static_cast<ColdHarness*>(hv);
  if (!h || (!out && cap)) {
    set_error("kc_coldset_all_keys: NULL");
    return -EINVAL;
  }
  if (h->failed) {
    set_error("kc_coldset_all_keys: an add failed; clear first");
    return -EINVAL;
  }
  std::vector<uint64_t> keys;
  KC_TRY(h->cs.all_keys(keys));
  for (uint64_t i = 0; i < keys.size() && i < cap; ++i) out[i] = keys[i];
  return (int64_t)keys.size();
}

int kc_coldset_clear(void* hv) {
  ColdHarness* h = static_cast<ColdHarness*>(hv);
  if (!h) {
    set_error("kc_coldset_clear: NULL");
    return -EINVAL;
  }
  h->cs.clear();
  h->failed = false;
  return 0;
}

void kc_coldset_destroy(void* hv) {
  ColdHarness* h = static_cast<ColdHarness*>(hv);
  if (!h) return;
  h->cs.clear();
  delete h;
}

int kc_cold_key_selftest(const uint64_t* in, uint64_t* out, uint64_t n, int unkey, int on_device) {
  if (!in || !out || n == 0 || n > kColdTestMax) {
    set_error("kc_cold_key_selftest: bad argument (n %llu)", (unsigned long long)n);
    return -EINVAL;
  }
  if (!on_device) {
    for (uint64_t i = 0; i < n; ++i) out[i] = unkey ? cold_unkey(in[i]) : cold_key(in[i]);
    return 0;
  }
  KC_TRY(have_device("kc_cold_key_selftest"));
  DevBuf di, dout;
  KC_TRY(di.alloc(n * 8));
  KC_TRY(dout.alloc(n * 8));
  KC_HIP_TRY(hipMemcpy(di.p, in, n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_cold_key_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                     di.as<const uint64_t>(), dout.as<uint64_t>(), n, unkey);
  KC_HIP_TRY(hipGetLastError());
  KC_HIP_TRY(hipDeviceSynchronize());
  KC_HIP_TRY(hipMemcpy(out, dout.p, n * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
