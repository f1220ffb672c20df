// ckpt.hip — the device streams of checkpoint / recover and
// the host-only kc_checkpoint_info.  The engine (engine.hip) decides what is
// saved and when; this file moves it: the seen-set out of its sparse table as
// a dense fingerprint stream, window by window (k_ckpt_pack), plain device
// ranges out and in, and the fingerprints back in through the list-insert
// kernels Init uses, so the probe sequence is the engine's own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/kubecheck.h"
#include "ckpt.h"
#include "ckpt_kernels.h"
#include "kc_common.h"

namespace kc {

namespace {
// accumulator words of CkptStage::d_acc / h_acc: one pack pass per buffer,
// then the upload checksum and the restore's failure count
constexpr int ACC_UP = 2 * CA_WORDS, ACC_BAD = ACC_UP + 2, ACC_WORDS = 16;
}  // namespace

int CkptStage::setup(uint64_t stage_bytes) {
  if (!stage_bytes) stage_bytes = CKPT_STAGE_DEFAULT;
  if (stage_bytes < CKPT_STAGE_MIN) {
    set_error("checkpoint: stage_bytes %llu below %llu", (unsigned long long)stage_bytes,
              (unsigned long long)CKPT_STAGE_MIN);
    return -EINVAL;
  }
  const uint64_t w = stage_bytes / 16 * 2;        // whole 16-B units
  if (w != words) {
    for (int b = 0; b < 2; ++b) {
      KC_TRY(h[b].renew(w));
      KC_TRY(d[b].renew(w));
      KC_TRY(d_res[b].renew(w));
    }
    words = w;
  }
  KC_TRY(h_acc.alloc(ACC_WORDS));
  KC_TRY(d_acc.alloc(ACC_WORDS));
  for (int b = 0; b < 2; ++b) KC_TRY(ev[b].create(hipEventDisableTiming));
  return 0;
}

int ckpt_pack_fps(const DevClaimSet& cs, uint64_t window_slots, CkptStage& sg, hipStream_t st, const CkptSink& sink,
                  uint64_t* count, CkptSum* sum, double* pack_ms) {
  const uint64_t spu = cs.compact ? 2 : 1;                 // slots per 16-B unit
  const uint64_t units = (cs.nslots + spu - 1) / spu;
  uint64_t win = sg.words / spu;                           // a window full of fingerprints fits one buffer
  if (window_slots) win = std::min(win, std::max<uint64_t>(1, window_slots / spu));
  const uint64_t nwin = (units + win - 1) / win;
  const ulonglong2* t = reinterpret_cast<const ulonglong2*>(cs.t.p);
  OwnedEvent evd[2];                                       // a window's fingerprints are in pinned memory
  KC_TRY(evd[0].create(hipEventDisableTiming));
  KC_TRY(evd[1].create(hipEventDisableTiming));
  OwnedEvent tk[2][2];                                     // pack_ms: around each window's kernel
  if (pack_ms) {
    *pack_ms = 0;
    for (int b = 0; b < 2; ++b) {
      KC_TRY(tk[b][0].create());
      KC_TRY(tk[b][1].create());
    }
  }
  auto pack = [&](uint64_t k) -> int {
    const int b = (int)(k & 1);
    const uint64_t u0 = k * win, u1 = std::min(units, u0 + win);
    unsigned long long* acc = sg.d_acc + b * CA_WORDS;
    KC_HIP_TRY(hipMemsetAsync(acc, 0, CA_WORDS * 8, st));
    if (pack_ms) KC_HIP_TRY(hipEventRecord(tk[b][0], st));
    // (a workgroup takes CKPT_UNITS x 256 units per trip: table_grid counts 256 per workgroup)
    const unsigned grid = table_grid((u1 - u0 + CKPT_UNITS - 1) / CKPT_UNITS);
    if (cs.compact)
      hipLaunchKernelGGL(k_ckpt_pack<true>, dim3(grid), dim3(CKPT_THREADS), 0, st, t, cs.nslots, u0, u1, sg.d[b].p,
                         sg.words, acc);
    else
      hipLaunchKernelGGL(k_ckpt_pack<false>, dim3(grid), dim3(CKPT_THREADS), 0, st, t, cs.nslots, u0, u1, sg.d[b].p,
                         sg.words, acc);
    KC_HIP_TRY(hipGetLastError());
    if (pack_ms) KC_HIP_TRY(hipEventRecord(tk[b][1], st));
    KC_HIP_TRY(hipMemcpyAsync(sg.h_acc + b * CA_WORDS, acc, CA_WORDS * 8, hipMemcpyDeviceToHost, st));
    KC_HIP_TRY(hipEventRecord(sg.ev[b], st));
    return 0;
  };
  uint64_t total = 0;
  CkptSum s;
  KC_TRY(pack(0));
  for (uint64_t k = 0; k < nwin; ++k) {
    const int b = (int)(k & 1);
    const uint64_t u0 = k * win, u1 = std::min(units, u0 + win);
    KC_HIP_TRY(hipEventSynchronize(sg.ev[b]));
    if (pack_ms) {
      float ms = 0;
      KC_HIP_TRY(hipEventElapsedTime(&ms, tk[b][0], tk[b][1]));
      *pack_ms += ms;
    }
    const uint64_t c = sg.h_acc[b * CA_WORDS + CA_COUNT];
    if (c > (u1 - u0) * spu || c > sg.words) {
      set_error("checkpoint: a window of %llu slots packed %llu fingerprints", (unsigned long long)((u1 - u0) * spu),
                (unsigned long long)c);
      return -EIO;
    }
    s.sum += sg.h_acc[b * CA_WORDS + CA_SUM];
    s.x ^= sg.h_acc[b * CA_WORDS + CA_XOR];
    total += c;
    if (c) {
      KC_HIP_TRY(hipMemcpyAsync(sg.h[b], sg.d[b], c * 8, hipMemcpyDeviceToHost, st));
      KC_HIP_TRY(hipEventRecord(evd[b], st));
    }
    // the next window goes to the other buffer, which the sink has left
    if (k + 1 < nwin) KC_TRY(pack(k + 1));
    if (c) {
      KC_HIP_TRY(hipEventSynchronize(evd[b]));
      KC_TRY(sink(reinterpret_cast<const uint64_t*>(sg.h[b].p), c));
    }
  }
  *count = total;
  *sum = s;
  return 0;
}

int ckpt_download(const void* dev, uint64_t bytes, CkptStage& sg, hipStream_t st, const CkptSink& sink) {
  const uint8_t* p = static_cast<const uint8_t*>(dev);
  const uint64_t piece = sg.words * 8;
  uint64_t prev_words = 0;
  int k = 0;
  for (uint64_t at = 0; at < bytes; at += piece, ++k) {
    const int b = k & 1;
    const uint64_t len = std::min(piece, bytes - at), w = (len + 7) / 8;
    sg.h[b][w - 1] = 0;                                    // the padding of a last, partial word
    KC_HIP_TRY(hipMemcpyAsync(sg.h[b], p + at, len, hipMemcpyDeviceToHost, st));
    KC_HIP_TRY(hipEventRecord(sg.ev[b], st));
    if (k > 0) {
      KC_HIP_TRY(hipEventSynchronize(sg.ev[b ^ 1]));
      KC_TRY(sink(reinterpret_cast<const uint64_t*>(sg.h[b ^ 1].p), prev_words));
    }
    prev_words = w;
  }
  if (k > 0) {
    const int b = (k - 1) & 1;
    KC_HIP_TRY(hipEventSynchronize(sg.ev[b]));
    KC_TRY(sink(reinterpret_cast<const uint64_t*>(sg.h[b].p), prev_words));
  }
  return 0;
}

namespace {
int read_acc(CkptStage& sg, hipStream_t st, uint64_t* bad, CkptSum* dev_sum) {
  KC_HIP_TRY(hipMemcpyAsync(sg.h_acc + ACC_UP, sg.d_acc + ACC_UP, 3 * 8, hipMemcpyDeviceToHost, st));
  KC_HIP_TRY(hipStreamSynchronize(st));
  dev_sum->sum = sg.h_acc[ACC_UP];
  dev_sum->x = sg.h_acc[ACC_UP + 1];
  if (bad) *bad = sg.h_acc[ACC_BAD];
  return 0;
}
}  // namespace

int ckpt_upload(void* dev, uint64_t n, CkptStage& sg, hipStream_t st, const CkptFeed& feed, CkptSum* dev_sum) {
  unsigned long long* p = static_cast<unsigned long long*>(dev);
  KC_HIP_TRY(hipMemsetAsync(sg.d_acc + ACC_UP, 0, 3 * 8, st));
  int k = 0;
  for (uint64_t at = 0; at < n; at += sg.words, ++k) {
    const int b = k & 1;
    const uint64_t m = std::min(sg.words, n - at);
    if (k >= 2) KC_HIP_TRY(hipEventSynchronize(sg.ev[b]));  // the copy out of this buffer is done
    KC_TRY(feed(reinterpret_cast<uint64_t*>(sg.h[b].p), at, m));
    KC_HIP_TRY(hipMemcpyAsync(p + at, sg.h[b], m * 8, hipMemcpyHostToDevice, st));
    KC_HIP_TRY(hipEventRecord(sg.ev[b], st));
    hipLaunchKernelGGL(k_ckpt_sum, dim3(table_grid(m / 2 + 1)), dim3(CKPT_THREADS), 0, st, p + at, m, sg.d_acc + ACC_UP);
    KC_HIP_TRY(hipGetLastError());
  }
  return read_acc(sg, st, nullptr, dev_sum);
}

int ckpt_restore_fps(const DevClaimSet& cs, uint64_t n, uint64_t window, CkptStage& sg, hipStream_t st,
                     const CkptFeed& feed, uint64_t* bad, CkptSum* dev_sum) {
  const uint64_t win = window ? std::min(window, sg.words) : sg.words;
  KC_HIP_TRY(hipMemsetAsync(sg.d_acc + ACC_UP, 0, 3 * 8, st));
  int k = 0;
  for (uint64_t at = 0; at < n; at += win, ++k) {
    const int b = k & 1;
    const uint64_t m = std::min(win, n - at);
    if (k >= 2) KC_HIP_TRY(hipEventSynchronize(sg.ev[b]));  // the kernels that read this buffer are done
    KC_TRY(feed(reinterpret_cast<uint64_t*>(sg.h[b].p), at, m));
    KC_HIP_TRY(hipMemcpyAsync(sg.d[b], sg.h[b], m * 8, hipMemcpyHostToDevice, st));
    launch_claimset_insert_list(reinterpret_cast<const uint64_t*>(sg.d[b].p), m, cs, 1u, sg.d_res[b].p, st);
    hipLaunchKernelGGL(k_ckpt_count_bad, dim3((unsigned)((m + CKPT_THREADS - 1) / CKPT_THREADS)), dim3(CKPT_THREADS), 0,
                       st, sg.d_res[b].p, m, sg.d_acc + ACC_BAD);
    hipLaunchKernelGGL(k_ckpt_sum, dim3(table_grid(m / 2 + 1)), dim3(CKPT_THREADS), 0, st, sg.d[b].p, m,
                       sg.d_acc + ACC_UP);
    KC_HIP_TRY(hipGetLastError());
    KC_HIP_TRY(hipEventRecord(sg.ev[b], st));
  }
  return read_acc(sg, st, bad, dev_sum);
}

}  // namespace kc

extern "C" int kc_checkpoint_info(const char* dir, struct kc_checkpoint_info* out) {
  using namespace kc;
  if (!dir || !out) {
    set_error("kc_checkpoint_info: NULL argument");
    return -EINVAL;
  }
  CkptFileSource src;
  const std::string path = ckpt_path(dir);
  int rc = src.open(path);
  if (rc) {
    set_error("kc_checkpoint_info: %s: %s", path.c_str(), rc == -ENOENT ? "no such file" : "cannot open");
    return rc;
  }
  std::string err;
  rc = ckpt_validate(src, out, &err);
  if (rc) set_error("kc_checkpoint_info: %s: %s", path.c_str(), err.c_str());
  return rc;
}
