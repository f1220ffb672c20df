// probe_selftest.hip — test-only device harness for the seen-set probe
// primitives (kc_probe_selftest, include/kubecheck.h "tests").  It calls the
// product's device functions (fpset_dev.h, lds_claim of engine_kernels.h) and
// rehash kernels (fpset.hip) on a table of exactly the size asked for, so the
// suite can put probe runs at the table's end and fill a table completely;
// tests/probe_model.py is the host model the results are compared with.
// Nothing of the product path calls this file.
#include <hip/hip_runtime.h>

#include "../../include/kubecheck.h"
#include "engine_kernels.h"
#include "fpset_host.h"
#include "kc_common.h"

namespace kc {

enum ProbeKind : int {
  PK_FPSET_INSERT = 0,
  PK_FPSET_CONTAINS = 1,
  PK_CLAIM = 2,           // claimset_claim
  PK_CLAIM_STORE = 3,     // claimset_claim_store, claimset_store_claim of the CL_CUR ones, claimset_get
  PK_CLAIM_GET = 4,       // claimset_get alone
  PK_INSERT_FROM = 5,     // claimset_insert_from from the home slot
  PK_PAIR = 6,            // fpslots_insert_pair, default cas
  PK_PAIR_GROUP = 7,      // k_claim's order: a group's loads, then its CASes, then fpslots_insert_pair(..., cas)
  PK_PAIR_STALE = 8,      // the pair is given (keys[2i], keys[2i+1]): what a lane loaded before the table changed
  PK_BATCH = 9,           // batch_insert, then batch_is_rep
  PK_LDS = 10,            // lds_claim<CLAIM_LDS>
  PK_LDS_SH = 11,         // lds_claim<CLAIM_LDS_SH>
  PK_REHASH_CLAIMSET = 12,
  PK_REHASH_FPSLOTS = 13,
  PK_REHASH_FPSET = 14,
  PK_COUNT
};

// one operation (or, PK_PAIR_GROUP, one group of KC_CLAIM_BATCH) on an HBM table
__device__ __forceinline__ void probe_op(int kind, int phase, unsigned long long* __restrict__ w, uint64_t nslots,
                                         const uint64_t* __restrict__ fps, const uint64_t* __restrict__ keys,
                                         uint64_t n, uint32_t level, uint64_t i, unsigned long long* __restrict__ res) {
  ClaimEntry* cs = reinterpret_cast<ClaimEntry*>(w);
  const uint64_t fp = kind == PK_PAIR_GROUP ? 0 : fps[i];
  switch (kind) {
    case PK_FPSET_INSERT:
      res[i] = (unsigned long long)(long long)fpset_insert(w, nslots / 8, fp);
      break;
    case PK_FPSET_CONTAINS:
      res[i] = (unsigned long long)fpset_contains(w, nslots / 8, fp);
      break;
    case PK_CLAIM:
      res[i] = (unsigned long long)claimset_claim(cs, nslots, fp, make_claim(level, keys[i]), level);
      break;
    case PK_CLAIM_STORE:
      if (phase == 0) {
        res[i] = (unsigned long long)claimset_claim_store(cs, nslots, fp, make_claim(level, keys[i]), level);
      } else if (phase == 1) {
        if (res[i] == (unsigned long long)CL_CUR) claimset_store_claim(cs, nslots, fp, make_claim(level, keys[i]));
      } else {
        res[n + i] = claimset_get(cs, nslots, fp) == ~(unsigned long long)make_claim(level, keys[i]);
      }
      break;
    case PK_CLAIM_GET:
      res[i] = claimset_get(cs, nslots, fp);
      break;
    case PK_INSERT_FROM: {
      const uint64_t h = bucket_of(fp, nslots);
      res[i] = (unsigned long long)claimset_insert_from(cs, nslots, fp, h, cs[h].fp);
      break;
    }
    case PK_PAIR: {
      const uint64_t h = fpslots_home(fp, nslots);
      res[i] = (unsigned long long)fpslots_insert_pair(w, nslots, fp, h, fpslots_first(w, h));
      break;
    }
    case PK_PAIR_STALE: {
      const uint64_t h = fpslots_home(fp, nslots);
      const ulonglong2 e = make_ulonglong2(keys[2 * i], keys[2 * i + 1]);
      const uint64_t j = fpslots_pair_target(h, e, fp);
      unsigned long long cas = ~0ull;
      if (j < ~1ull) cas = atomicCAS(&w[j], 0ull, (unsigned long long)fp);
      res[i] = (unsigned long long)fpslots_insert_pair(w, nslots, fp, h, e, cas);
      break;
    }
    case PK_PAIR_GROUP: {
      unsigned long long fpq[KC_CLAIM_BATCH], cq[KC_CLAIM_BATCH];
      ulonglong2 eq[KC_CLAIM_BATCH];
      uint64_t iq[KC_CLAIM_BATCH];
#pragma unroll
      for (int q = 0; q < KC_CLAIM_BATCH; ++q) {
        const uint64_t k = i * KC_CLAIM_BATCH + q;
        fpq[q] = k < n ? fps[k] : 0ull;
        if (fpq[q]) {
          iq[q] = fpslots_home(fpq[q], nslots);
          eq[q] = fpslots_first(w, iq[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < KC_CLAIM_BATCH; ++q) {
        cq[q] = ~0ull;
        const uint64_t j = fpq[q] ? fpslots_pair_target(iq[q], eq[q], fpq[q]) : ~0ull;
        if (j < ~1ull) cq[q] = atomicCAS(&w[j], 0ull, fpq[q]);
      }
#pragma unroll
      for (int q = 0; q < KC_CLAIM_BATCH; ++q) {
        const uint64_t k = i * KC_CLAIM_BATCH + q;
        if (k < n && fpq[q]) res[k] = (unsigned long long)fpslots_insert_pair(w, nslots, fpq[q], iq[q], eq[q], cq[q]);
      }
      break;
    }
    case PK_BATCH: {
      BatchEntry* bt = reinterpret_cast<BatchEntry*>(w);
      if (phase == 0) batch_insert(bt, nslots - 1, fp, keys[i]);
      else res[i] = batch_is_rep(bt, nslots - 1, fp, keys[i]) ? 1ull : 0ull;
      break;
    }
    default:
      break;
  }
}

// sequential: lane 0 of workgroup 0 runs the units in order; else a lane each
__global__ void __launch_bounds__(64) k_probe_ops(int kind, int phase, int sequential, unsigned long long* __restrict__ w,
                                                  uint64_t nslots, const uint64_t* __restrict__ fps,
                                                  const uint64_t* __restrict__ keys, uint64_t n, uint64_t units,
                                                  uint32_t level, unsigned long long* __restrict__ res) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sequential) {
    if (g == 0)
      for (uint64_t i = 0; i < units; ++i) probe_op(kind, phase, w, nslots, fps, keys, n, level, i, res);
  } else if (g < units) {
    probe_op(kind, phase, w, nslots, fps, keys, n, level, g, res);
  }
}

// lds_claim<NT> in one workgroup: the table (pre-loaded from `img`, NT x
// {fp, key}, or empty) lives in LDS and is copied out
template <int NT>
__global__ void __launch_bounds__(256) k_probe_lds(int sequential, const unsigned long long* __restrict__ img,
                                                   const uint64_t* __restrict__ fps, const uint64_t* __restrict__ keys,
                                                   uint64_t n, unsigned long long* __restrict__ res,
                                                   unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh_fp[NT];
  __shared__ unsigned int sh_key[NT];
  for (int k = threadIdx.x; k < NT; k += blockDim.x) {
    sh_fp[k] = img ? img[2 * k] : 0ull;
    sh_key[k] = img ? (unsigned int)img[2 * k + 1] : ~0u;
  }
  __syncthreads();
  if (sequential) {
    if (threadIdx.x == 0)
      for (uint64_t i = 0; i < n; ++i)
        res[i] = (unsigned long long)(long long)lds_claim<NT>(sh_fp, sh_key, fps[i], (unsigned int)keys[i]);
  } else {
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x)
      res[i] = (unsigned long long)(long long)lds_claim<NT>(sh_fp, sh_key, fps[i], (unsigned int)keys[i]);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < NT; k += blockDim.x) {
    out[2 * k] = sh_fp[k];
    out[2 * k + 1] = sh_key[k];
  }
}

struct ProbeBufs {
  DeviceArray<unsigned long long> w, old, res, fail;
  DeviceArray<uint64_t> fps, keys;
};

static int probe_run(int kind, uint64_t nslots, const uint64_t* fps, const uint64_t* keys, uint64_t n, uint32_t level,
                     int mode, const uint64_t* table_in, uint64_t* res_out, uint64_t* table_out) {
  const bool lds = kind == PK_LDS || kind == PK_LDS_SH;
  const bool rehash = kind >= PK_REHASH_CLAIMSET;
  const bool wide = kind == PK_CLAIM || kind == PK_CLAIM_STORE || kind == PK_CLAIM_GET || kind == PK_INSERT_FROM ||
                    kind == PK_BATCH || kind == PK_REHASH_CLAIMSET || lds;
  const uint64_t wps = wide ? 2 : 1;                                 // u64 words per slot
  const uint64_t nres = rehash ? 1 : kind == PK_CLAIM_STORE ? 2 * n : n;
  const uint64_t nkeys = kind == PK_PAIR_STALE ? 2 * n : n;
  ProbeBufs b;
  hipStream_t st = nullptr;
  KC_TRY(b.w.alloc(nslots * wps));
  if (table_in && !rehash) KC_HIP_TRY(hipMemcpy(b.w, table_in, nslots * wps * 8, hipMemcpyHostToDevice));
  else KC_HIP_TRY(hipMemset(b.w, 0, nslots * wps * 8));
  KC_TRY(b.res.alloc(nres ? nres : 1));
  KC_HIP_TRY(hipMemset(b.res, 0, (nres ? nres : 1) * 8));
  if (rehash) {
    // table_in: the old table of n slots; the new one has nslots
    KC_TRY(b.old.alloc(n * wps));
    KC_HIP_TRY(hipMemcpy(b.old, table_in, n * wps * 8, hipMemcpyHostToDevice));
    KC_TRY(b.fail.alloc(1));
    KC_HIP_TRY(hipMemset(b.fail, 0, 8));
    if (kind == PK_REHASH_CLAIMSET)
      launch_claimset_rehash(reinterpret_cast<const ClaimEntry*>(b.old.p), n, reinterpret_cast<ClaimEntry*>(b.w.p), nslots,
                             b.fail, st);
    else if (kind == PK_REHASH_FPSLOTS)
      launch_fpslots_rehash(b.old, n, b.w, nslots, b.fail, st);
    else
      launch_fpset_rehash(b.old, n, b.w, nslots / 8, b.fail, st);
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipMemcpy(b.res, b.fail, 8, hipMemcpyDeviceToDevice));
  } else if (n) {
    KC_TRY(b.fps.alloc(n));
    KC_HIP_TRY(hipMemcpy(b.fps, fps, n * 8, hipMemcpyHostToDevice));
    KC_TRY(b.keys.alloc(nkeys));
    if (keys) KC_HIP_TRY(hipMemcpy(b.keys, keys, nkeys * 8, hipMemcpyHostToDevice));
    else KC_HIP_TRY(hipMemset(b.keys, 0, nkeys * 8));
    if (lds) {
      // (b.w doubles as the image in and out: the kernel reads it all before it writes)
      KC_TRY(b.old.alloc(nslots * 2));
      KC_HIP_TRY(hipMemcpy(b.old, b.w, nslots * 16, hipMemcpyDeviceToDevice));
      const unsigned long long* img = table_in ? b.old.p : nullptr;
      if (kind == PK_LDS)
        hipLaunchKernelGGL(k_probe_lds<CLAIM_LDS>, dim3(1), dim3(256), 0, st, mode == 0, img, b.fps, b.keys, n, b.res, b.w);
      else
        hipLaunchKernelGGL(k_probe_lds<CLAIM_LDS_SH>, dim3(1), dim3(256), 0, st, mode == 0, img, b.fps, b.keys, n, b.res,
                           b.w);
    } else {
      const uint64_t units = kind == PK_PAIR_GROUP ? (n + KC_CLAIM_BATCH - 1) / KC_CLAIM_BATCH : n;
      const unsigned grid = mode == 0 ? 1u : (unsigned)((units + 63) / 64);
      const int phases = kind == PK_CLAIM_STORE ? 3 : kind == PK_BATCH ? 2 : 1;
      for (int ph = 0; ph < phases; ++ph)
        hipLaunchKernelGGL(k_probe_ops, dim3(grid), dim3(64), 0, st, kind, ph, mode == 0, b.w, nslots, b.fps, b.keys, n,
                           units, level, b.res);
    }
    KC_HIP_TRY(hipGetLastError());
  }
  KC_HIP_TRY(hipDeviceSynchronize());
  if (res_out && nres) KC_HIP_TRY(hipMemcpy(res_out, b.res, nres * 8, hipMemcpyDeviceToHost));
  if (table_out) KC_HIP_TRY(hipMemcpy(table_out, b.w, nslots * wps * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace kc

extern "C" int kc_probe_selftest(int kind, uint64_t nslots, const uint64_t* fps, const uint64_t* keys, uint64_t n,
                                 uint32_t level, int mode, const uint64_t* table_in, uint64_t* res_out,
                                 uint64_t* table_out) {
  using namespace kc;
  const bool lds = kind == PK_LDS || kind == PK_LDS_SH;
  const bool rehash = kind >= PK_REHASH_CLAIMSET && kind < PK_COUNT;
  const bool fpset = kind == PK_FPSET_INSERT || kind == PK_FPSET_CONTAINS || kind == PK_REHASH_FPSET;
  const bool pair = kind == PK_PAIR || kind == PK_PAIR_GROUP || kind == PK_PAIR_STALE || kind == PK_REHASH_FPSLOTS;
  bool ok = kind >= 0 && kind < PK_COUNT && (mode == 0 || mode == 1) && nslots >= 2 && nslots <= (1ull << 24) &&
            n <= (1ull << 24) && level < (1u << 20) && (n == 0 || rehash || fps) && (!rehash || (table_in && n >= 2));
  if (ok && fpset) ok = nslots % 8 == 0 && (!rehash || n % 8 == 0);
  if (ok && pair) ok = nslots % 2 == 0 && (!rehash || n % 2 == 0);
  if (ok && kind == PK_PAIR_STALE) ok = keys != nullptr;
  if (ok && lds) ok = nslots == (uint64_t)(kind == PK_LDS ? CLAIM_LDS : CLAIM_LDS_SH);
  // the batch table's loops have no bound: a power-of-two table at most half full
  if (ok && kind == PK_BATCH) ok = (nslots & (nslots - 1)) == 0 && !table_in && n * 2 <= nslots;
  if (!ok) {
    set_error("kc_probe_selftest: bad argument (kind %d, nslots %llu, n %llu, mode %d)", kind,
              (unsigned long long)nslots, (unsigned long long)n, mode);
    return -EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("kc_probe_selftest: no HIP device");
    return -ENODEV;
  }
  return probe_run(kind, nslots, fps, keys, n, level, mode, table_in, res_out, table_out);
}
