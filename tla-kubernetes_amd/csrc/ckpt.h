// ckpt.h — host side of the checkpoint streams (ckpt.hip): everything that
// leaves or enters HBM goes through two pinned staging buffers, ordered with
// events on the caller's stream (no device-wide sync).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "ckpt_file.h"
#include "fpset_host.h"
#include "owned.h"

namespace kc {

constexpr uint64_t CKPT_STAGE_DEFAULT = 64ull << 20;
constexpr uint64_t CKPT_STAGE_MIN = 4096;

// Two staging buffers of `words` u64 each, in pinned memory and in HBM, the
// list-insert results of a restore and the device accumulators.
struct CkptStage {
  PinnedArray<unsigned long long> h[2], h_acc;
  DeviceArray<unsigned long long> d[2], d_acc;
  DeviceArray<int> d_res[2];
  OwnedEvent ev[2];
  uint64_t words = 0;
  // (re)allocate for stage_bytes per buffer (0 = the default)
  int setup(uint64_t stage_bytes);
};

// takes n words of a stream, in order
using CkptSink = std::function<int(const uint64_t* words, uint64_t n)>;
// fills dst with the n words that start at word `at` of a stream
using CkptFeed = std::function<int(uint64_t* dst, uint64_t at, uint64_t n)>;

// k_ckpt_pack over the whole table, one launch per window of window_slots
// slots (0: as many as one staging buffer takes when full; never more than
// that): window k + 1 is packed while the host takes window k.  *count
// fingerprints went to the sink, with the device's checksum of them.
// pack_ms (may be NULL): the kernels' own time, by events around each launch.
int ckpt_pack_fps(const DevClaimSet& cs, uint64_t window_slots, CkptStage& sg, hipStream_t st, const CkptSink& sink,
                  uint64_t* count, CkptSum* sum, double* pack_ms = nullptr);
// `bytes` of device memory to the sink as whole words (the last zero-padded)
int ckpt_download(const void* dev, uint64_t bytes, CkptStage& sg, hipStream_t st, const CkptSink& sink);
// n words from the feed into device memory (room for n words at dev), and
// their checksum as the device sees them afterwards (k_ckpt_sum)
int ckpt_upload(void* dev, uint64_t n, CkptStage& sg, hipStream_t st, const CkptFeed& feed, CkptSum* dev_sum);
// n fingerprints from the feed into the ClaimSet with the list-insert kernels
// (level 1), at most window fingerprints per launch (0: a staging buffer's
// worth); *bad = how many were not new, dev_sum as above.  cs.count is not
// touched.
int ckpt_restore_fps(const DevClaimSet& cs, uint64_t n, uint64_t window, CkptStage& sg, hipStream_t st,
                     const CkptFeed& feed, uint64_t* bad, CkptSum* dev_sum);

}  // namespace kc
