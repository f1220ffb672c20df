// ckpt_selftest.hip — test-only harness for the checkpoint streams
// (kc_ckpt_selftest, include/kubecheck.h "tests"): the product's own
// ckpt_pack_fps and ckpt_restore_fps (ckpt.hip) on a table of exactly the
// size and image asked for, so the suite can put runs across the table's end
// and windows across its occupied and empty stretches; tests/probe_model.py is
// the host model.  Nothing of the product path calls this file.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/kubecheck.h"
#include "ckpt.h"
#include "kc_common.h"

extern "C" int kc_ckpt_selftest(int kind, int layout, uint64_t nslots, const uint64_t* in, uint64_t n, uint64_t window,
                                uint64_t stage_bytes, uint64_t* out, uint64_t* stats_out) {
  using namespace kc;
  const bool ok = (kind == 0 || kind == 1) && (layout == 0 || layout == 1) && nslots >= 2 && nslots <= (1ull << 24) &&
                  (layout == 0 || nslots % 2 == 0) && n <= (1ull << 24) && out && stats_out && (in || (kind == 1 && !n)) &&
                  (kind == 1 || n == nslots * (layout ? 1 : 2));
  if (!ok) {
    set_error("kc_ckpt_selftest: bad argument (kind %d, layout %d, nslots %llu, n %llu)", kind, layout,
              (unsigned long long)nslots, (unsigned long long)n);
    return -EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("kc_ckpt_selftest: no HIP device");
    return -ENODEV;
  }
  OwnedStream st;
  KC_TRY(st.create(hipStreamNonBlocking));
  CkptStage sg;
  KC_TRY(sg.setup(stage_bytes));
  // a table of exactly nslots slots (DevClaimSet::init would round 2..63 up)
  DevClaimSet cs;
  cs.compact = layout == 1;
  cs.nslots = nslots;
  const uint64_t bytes = nslots * cs.slot_bytes();
  KC_TRY(cs.t.alloc(cs.units(nslots)));
  if (kind == 0) {
    KC_HIP_TRY(hipMemcpyAsync(cs.t, in, bytes, hipMemcpyHostToDevice, st));
    uint64_t got = 0, count = 0;
    CkptSum sum;
    const CkptSink sink = [&](const uint64_t* w, uint64_t m) -> int {
      if (got + m > nslots) {
        set_error("kc_ckpt_selftest: more fingerprints than slots");
        return -EIO;
      }
      std::copy(w, w + m, out + got);
      got += m;
      return 0;
    };
    KC_TRY(ckpt_pack_fps(cs, window, sg, st, sink, &count, &sum));
    stats_out[0] = count;
    stats_out[1] = sum.sum;
    stats_out[2] = sum.x;
    stats_out[3] = got;
    return 0;
  }
  KC_HIP_TRY(hipMemsetAsync(cs.t, 0, bytes, st));
  uint64_t bad = 0;
  CkptSum sum;
  const CkptFeed feed = [&](uint64_t* dst, uint64_t at, uint64_t m) -> int {
    std::copy(in + at, in + at + m, dst);
    return 0;
  };
  KC_TRY(ckpt_restore_fps(cs, n, window, sg, st, feed, &bad, &sum));
  KC_HIP_TRY(hipMemcpyAsync(out, cs.t, bytes, hipMemcpyDeviceToHost, st));
  KC_HIP_TRY(hipStreamSynchronize(st));
  stats_out[0] = bad;
  stats_out[1] = sum.sum;
  stats_out[2] = sum.x;
  stats_out[3] = n;
  return 0;
}
