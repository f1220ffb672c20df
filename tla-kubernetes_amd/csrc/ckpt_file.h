// ckpt_file.h — the checkpoint file (DIR/checkpoint.kc): its layout, the
// writer, and the parser / validator behind kc_checkpoint_info and
// kc_engine_recover.  Host-only C++ (no HIP): csrc/ckpt_file_check.cpp builds
// it alone under the host sanitizers.  The word-by-word layout is documented
// in include/kubecheck.h ("Checkpoint"); tests/ckpt_model.py is an independent
// reader and writer of the same format.
//
// The parser takes hostile input: every offset and size is checked against
// the file's length before anything is read, sizes are derived from the
// header's counts with overflow checks, and a failure is a code plus a text,
// never an out-of-bounds access.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/kubecheck.h"

namespace kc {

constexpr uint64_t CKPT_MAGIC = 0x54504B434542554Bull;   // "KUBECKPT", little-endian
constexpr uint64_t CKPT_VERSION = 1;
constexpr int CKPT_HEADER_WORDS = 64;
constexpr uint64_t CKPT_HEADER_BYTES = CKPT_HEADER_WORDS * 8;
constexpr int CKPT_SECTIONS = KC_CKPT_SECTIONS;
enum CkptSection : int { CS_COUNTERS = 0, CS_FRONTIER = 1, CS_FPS = 2, CS_TRACE_PARENT = 3, CS_TRACE_ORD = 4 };
// header word indices (include/kubecheck.h lists them)
enum CkptWord : int {
  CW_MAGIC = 0, CW_VERSION = 1, CW_HEADER_WORDS = 2, CW_FILE_BYTES = 3,
  CW_NC = 4, CW_NP = 5, CW_NS = 6, CW_CAN_FAIL = 7, CW_CAN_TIMEOUT = 8, CW_CHECK_DEADLOCK = 9, CW_VARIANT = 10,
  CW_INVARIANTS = 11, CW_SYMMETRY = 12, CW_STATE_WORDS = 13, CW_KEEP_TRACE = 14, CW_CLAIM_MODE = 15,
  CW_LEVEL = 16, CW_LEVEL_GIDX = 17, CW_N = 18, CW_CAND = 19, CW_CAND_TOTAL = 20,
  CW_INIT = 21, CW_DISTINCT = 22, CW_NLEVELS = 23, CW_PEAK_FRONTIER = 24, CW_NSECTIONS = 25,
  CW_SECTION0 = 26,                 // CKPT_SECTIONS x {offset, bytes, sum, xor}
  CW_RESERVED = CW_SECTION0 + 4 * CKPT_SECTIONS,
  CW_HEADER_SUM = 62, CW_HEADER_XOR = 63
};
static_assert(CW_RESERVED <= CW_HEADER_SUM, "the section table fits the header");
// the COUNTERS section after level_width[nlevels]: act_gen, act_dist,
// outdeg, then probes, settles, cand_ovf, narrow_probes
constexpr uint64_t CKPT_COUNTER_TAIL = 2 * KC_NACTIONS + 16 + 4;

// (sum mod 2^64, xor) of u64 words: independent of their order
struct CkptSum {
  uint64_t sum = 0, x = 0;
  void add(const uint64_t* w, uint64_t n) {
    uint64_t s = sum, q = x;
    for (uint64_t i = 0; i < n; ++i) {
      s += w[i];
      q ^= w[i];
    }
    sum = s;
    x = q;
  }
  bool operator==(const CkptSum& o) const { return sum == o.sum && x == o.x; }
};

inline std::string ckpt_path(const char* dir) { return std::string(dir ? dir : "") + "/checkpoint.kc"; }

// ------------------------------------------------------------------ sources
// What the parser reads from: a file, or (the stand-alone check) a memory image.
struct CkptSource {
  virtual ~CkptSource() = default;
  virtual uint64_t size() const = 0;
  // exactly len bytes at off; false on a short read or an I/O error
  virtual bool read(uint64_t off, void* dst, uint64_t len) const = 0;
};
struct CkptMemSource final : CkptSource {
  const uint8_t* p;
  uint64_t n;
  CkptMemSource(const void* data, uint64_t len) : p(static_cast<const uint8_t*>(data)), n(len) {}
  uint64_t size() const override { return n; }
  bool read(uint64_t off, void* dst, uint64_t len) const override {
    if (off > n || len > n - off) return false;
    if (len) memcpy(dst, p + off, len);
    return true;
  }
};
struct CkptFileSource final : CkptSource {
  int fd = -1;
  uint64_t n = 0;
  CkptFileSource() = default;
  CkptFileSource(const CkptFileSource&) = delete;
  CkptFileSource& operator=(const CkptFileSource&) = delete;
  ~CkptFileSource() override {
    if (fd >= 0) ::close(fd);
  }
  // 0, or -errno (-ENOENT: no file)
  int open(const std::string& path) {
    fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) return errno == ENOENT || errno == ENOTDIR ? -ENOENT : -EIO;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return -EIO;
    n = (uint64_t)sb.st_size;
    return 0;
  }
  uint64_t size() const override { return n; }
  bool read(uint64_t off, void* dst, uint64_t len) const override {
    if (off > n || len > n - off) return false;
    uint8_t* d = static_cast<uint8_t*>(dst);
    while (len) {
      const ssize_t k = ::pread(fd, d, (size_t)std::min<uint64_t>(len, 1ull << 30), (off_t)off);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) return false;
      d += k;
      off += (uint64_t)k;
      len -= (uint64_t)k;
    }
    return true;
  }
};

// ------------------------------------------------------------------- parser
inline bool ckpt_mul(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_mul_overflow(a, b, out); }
inline bool ckpt_add(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_add_overflow(a, b, out); }

// The bytes each section must have for the header's counts (false: a count
// that overflows).  Sections the checkpoint does not carry have 0.
inline bool ckpt_expected_bytes(const struct kc_checkpoint_info& h, uint64_t exp[CKPT_SECTIONS]) {
  uint64_t t = 0, states = 0;
  if (!ckpt_add((uint64_t)h.nlevels, CKPT_COUNTER_TAIL, &t) || !ckpt_mul(t, 8, &exp[CS_COUNTERS])) return false;
  if (!ckpt_mul(h.n, (uint64_t)h.state_words, &t) || !ckpt_mul(t, 8, &exp[CS_FRONTIER])) return false;
  if (!ckpt_mul(h.distinct, 8, &exp[CS_FPS])) return false;
  exp[CS_TRACE_PARENT] = exp[CS_TRACE_ORD] = 0;
  if (h.keep_trace) {
    if (!ckpt_add(h.level_gidx, h.n, &states) || !ckpt_mul(states, 8, &exp[CS_TRACE_PARENT])) return false;
    if (!ckpt_add(states, 7, &t)) return false;
    exp[CS_TRACE_ORD] = t / 8 * 8;
  }
  return true;
}

// Header and structure: magic, version, the header's checksum, plausible
// counts, every section inside the file, of the size its counts ask for, none
// overlapping another or the header.  0, -EINVAL (not a checkpoint, unknown
// version) or -EIO (truncated, inconsistent, bad header checksum).
inline int ckpt_parse_header(const CkptSource& src, struct kc_checkpoint_info* out, std::string* err) {
  auto fail = [&](int rc, const std::string& m) {
    if (err) *err = m;
    return rc;
  };
  uint64_t w[CKPT_HEADER_WORDS];
  const uint64_t fsize = src.size();
  if (fsize < 8) return fail(-EIO, "truncated: shorter than the magic word");
  if (!src.read(0, w, 8)) return fail(-EIO, "cannot read the magic word");
  if (w[0] != CKPT_MAGIC) return fail(-EINVAL, "not a kubecheck checkpoint (magic)");
  if (fsize < 16) return fail(-EIO, "truncated inside the header");
  if (!src.read(8, w + 1, 8)) return fail(-EIO, "cannot read the version word");
  if (w[CW_VERSION] != CKPT_VERSION)
    return fail(-EINVAL, "unknown checkpoint version " + std::to_string(w[CW_VERSION]));
  if (fsize < CKPT_HEADER_BYTES) return fail(-EIO, "truncated inside the header");
  if (!src.read(0, w, CKPT_HEADER_BYTES)) return fail(-EIO, "cannot read the header");
  CkptSum hs;
  hs.add(w, CW_HEADER_SUM);
  if (hs.sum != w[CW_HEADER_SUM] || hs.x != w[CW_HEADER_XOR]) return fail(-EIO, "header checksum mismatch");
  if (w[CW_HEADER_WORDS] != (uint64_t)CKPT_HEADER_WORDS) return fail(-EIO, "header length field");
  if (w[CW_FILE_BYTES] != fsize)
    return fail(-EIO, "file has " + std::to_string(fsize) + " bytes, the header says " +
                          std::to_string(w[CW_FILE_BYTES]) + " (truncated?)");
  if (w[CW_NSECTIONS] != (uint64_t)CKPT_SECTIONS) return fail(-EIO, "section count");
  // small fields: bounded before they become ints
  static const int small[] = {CW_NC, CW_NP, CW_NS, CW_CAN_FAIL, CW_CAN_TIMEOUT, CW_CHECK_DEADLOCK, CW_VARIANT,
                              CW_INVARIANTS, CW_SYMMETRY, CW_STATE_WORDS, CW_KEEP_TRACE, CW_CLAIM_MODE};
  for (int k : small)
    if (w[k] > 4096) return fail(-EIO, "header word " + std::to_string(k) + " out of range");
  if (w[CW_STATE_WORDS] == 0) return fail(-EIO, "state_words is 0");
  if (w[CW_KEEP_TRACE] > 1) return fail(-EIO, "keep_trace is not 0 or 1");
  if (w[CW_LEVEL] == 0 || w[CW_LEVEL] > KC_MAX_LEVELS) return fail(-EIO, "level out of range");
  if (w[CW_NLEVELS] != w[CW_LEVEL]) return fail(-EIO, "nlevels differs from the level");
  if (w[CW_N] == 0) return fail(-EIO, "empty frontier");
  struct kc_checkpoint_info h;
  memset(&h, 0, sizeof h);
  h.version = w[CW_VERSION];
  h.file_bytes = w[CW_FILE_BYTES];
  h.nc = (int)w[CW_NC], h.np = (int)w[CW_NP], h.ns = (int)w[CW_NS];
  h.can_fail = (int)w[CW_CAN_FAIL], h.can_timeout = (int)w[CW_CAN_TIMEOUT];
  h.check_deadlock = (int)w[CW_CHECK_DEADLOCK], h.variant = (int)w[CW_VARIANT];
  h.invariants = (int)w[CW_INVARIANTS], h.symmetry = (int)w[CW_SYMMETRY];
  h.state_words = (int)w[CW_STATE_WORDS], h.keep_trace = (int)w[CW_KEEP_TRACE];
  h.claim_mode = (int)w[CW_CLAIM_MODE];
  h.level = (int)w[CW_LEVEL], h.nlevels = (int)w[CW_NLEVELS];
  h.level_gidx = w[CW_LEVEL_GIDX], h.n = w[CW_N], h.cand = w[CW_CAND], h.cand_total = w[CW_CAND_TOTAL];
  h.init = w[CW_INIT], h.distinct = w[CW_DISTINCT], h.peak_frontier = w[CW_PEAK_FRONTIER];
  for (int s = 0; s < CKPT_SECTIONS; ++s) {
    h.section_offset[s] = w[CW_SECTION0 + 4 * s];
    h.section_bytes[s] = w[CW_SECTION0 + 4 * s + 1];
    h.section_sum[s] = w[CW_SECTION0 + 4 * s + 2];
    h.section_xor[s] = w[CW_SECTION0 + 4 * s + 3];
  }
  // the counts among themselves
  uint64_t states = 0;
  if (!ckpt_add(h.level_gidx, h.n, &states)) return fail(-EIO, "level_gidx + n overflows");
  if (h.distinct != states) return fail(-EIO, "distinct differs from level_gidx + n");
  if (h.init == 0 || h.peak_frontier > h.distinct) return fail(-EIO, "inconsistent counts");
  uint64_t exp[CKPT_SECTIONS];
  if (!ckpt_expected_bytes(h, exp)) return fail(-EIO, "section sizes overflow");
  static const char* names[CKPT_SECTIONS] = {"COUNTERS", "FRONTIER", "FPS", "TRACE_PARENT", "TRACE_ORD"};
  for (int s = 0; s < CKPT_SECTIONS; ++s) {
    const uint64_t off = h.section_offset[s], len = h.section_bytes[s];
    if (len != exp[s])
      return fail(-EIO, std::string(names[s]) + " has " + std::to_string(len) + " bytes, its counts ask for " +
                            std::to_string(exp[s]));
    if (len == 0) {
      if (off != 0 || h.section_sum[s] || h.section_xor[s]) return fail(-EIO, std::string(names[s]) + ": absent but described");
      continue;
    }
    uint64_t end = 0;
    if (off % 8 || off < CKPT_HEADER_BYTES || !ckpt_add(off, len, &end) || end > fsize)
      return fail(-EIO, std::string(names[s]) + " lies outside the file");
    for (int q = 0; q < s; ++q) {
      const uint64_t qo = h.section_offset[q], ql = h.section_bytes[q];
      if (ql && off < qo + ql && qo < end)
        return fail(-EIO, std::string(names[s]) + " overlaps " + names[q]);
    }
  }
  *out = h;
  return 0;
}

// One section's checksum, streamed through `buf` (any size >= 8 bytes).
inline int ckpt_section_sum(const CkptSource& src, uint64_t off, uint64_t len, std::vector<uint64_t>& buf, CkptSum* out) {
  CkptSum s;
  if (buf.empty()) buf.resize(1 << 16);
  while (len) {
    const uint64_t k = std::min<uint64_t>(len, buf.size() * 8);
    if (!src.read(off, buf.data(), k)) return -EIO;
    s.add(buf.data(), k / 8);
    off += k;
    len -= k;
  }
  *out = s;
  return 0;
}

// The whole validation behind kc_checkpoint_info: the header, then every
// section's checksum.
inline int ckpt_validate(const CkptSource& src, struct kc_checkpoint_info* out, std::string* err) {
  struct kc_checkpoint_info h;
  const int rc = ckpt_parse_header(src, &h, err);
  if (rc) return rc;
  static const char* names[CKPT_SECTIONS] = {"COUNTERS", "FRONTIER", "FPS", "TRACE_PARENT", "TRACE_ORD"};
  std::vector<uint64_t> buf;
  for (int s = 0; s < CKPT_SECTIONS; ++s) {
    if (!h.section_bytes[s]) continue;
    CkptSum got;
    if (ckpt_section_sum(src, h.section_offset[s], h.section_bytes[s], buf, &got) ||
        got.sum != h.section_sum[s] || got.x != h.section_xor[s]) {
      if (err) *err = std::string(names[s]) + " fails its checksum";
      return -EIO;
    }
  }
  // the level widths are the counts' own record: they sum to distinct, the last is n
  std::vector<uint64_t> lw((size_t)h.nlevels);
  if (!src.read(h.section_offset[CS_COUNTERS], lw.data(), (uint64_t)h.nlevels * 8)) return -EIO;
  uint64_t tot = 0;
  for (uint64_t v : lw) tot += v;
  if (tot != h.distinct || lw.back() != h.n) {
    if (err) *err = "level widths do not add up to the header's counts";
    return -EIO;
  }
  *out = h;
  return 0;
}

// ------------------------------------------------------------------- writer
// checkpoint.kc.tmp, sections appended behind a header-sized hole, the header
// written last, fsync, rename over the old file: a process killed while
// writing leaves the previous checkpoint intact.
class CkptWriter {
 public:
  CkptWriter() = default;
  CkptWriter(const CkptWriter&) = delete;
  CkptWriter& operator=(const CkptWriter&) = delete;
  ~CkptWriter() {
    if (fd_ >= 0) {
      ::close(fd_);
      ::unlink(tmp_.c_str());
    }
  }
  int open(const char* dir, std::string* err) {
    dir_ = dir ? dir : "";
    final_ = ckpt_path(dir);
    tmp_ = final_ + ".tmp";
    fd_ = ::open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd_ < 0) {
      if (err) *err = "cannot create " + tmp_ + ": " + strerror(errno);
      return errno == ENOENT || errno == ENOTDIR ? -ENOENT : -EIO;
    }
    off_ = CKPT_HEADER_BYTES;
    return 0;
  }
  // a section starts at the current offset; its words follow through append()
  void begin(int section) {
    cur_ = section;
    sec_off_[section] = off_;
    sec_len_[section] = 0;
    sec_sum_[section] = CkptSum{};
  }
  int append(const uint64_t* words, uint64_t n) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(words);
    uint64_t len = n * 8;
    sec_sum_[cur_].add(words, n);
    sec_len_[cur_] += len;
    while (len) {
      const ssize_t k = ::pwrite(fd_, p, (size_t)std::min<uint64_t>(len, 1ull << 30), (off_t)off_);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) return -EIO;
      p += k;
      off_ += (uint64_t)k;
      len -= (uint64_t)k;
    }
    return 0;
  }
  const CkptSum& sum(int section) const { return sec_sum_[section]; }
  uint64_t bytes(int section) const { return sec_len_[section]; }
  uint64_t file_bytes() const { return off_; }
  // w: the header's words CW_NC .. CW_PEAK_FRONTIER filled by the caller; the
  // rest (magic, lengths, section table, checksum) is filled here
  int finish(uint64_t w[CKPT_HEADER_WORDS], std::string* err) {
    w[CW_MAGIC] = CKPT_MAGIC;
    w[CW_VERSION] = CKPT_VERSION;
    w[CW_HEADER_WORDS] = CKPT_HEADER_WORDS;
    w[CW_FILE_BYTES] = off_;
    w[CW_NSECTIONS] = CKPT_SECTIONS;
    for (int s = 0; s < CKPT_SECTIONS; ++s) {
      const bool on = sec_len_[s] != 0;
      w[CW_SECTION0 + 4 * s] = on ? sec_off_[s] : 0;
      w[CW_SECTION0 + 4 * s + 1] = sec_len_[s];
      w[CW_SECTION0 + 4 * s + 2] = on ? sec_sum_[s].sum : 0;
      w[CW_SECTION0 + 4 * s + 3] = on ? sec_sum_[s].x : 0;
    }
    for (int k = CW_RESERVED; k < CW_HEADER_SUM; ++k) w[k] = 0;
    CkptSum hs;
    hs.add(w, CW_HEADER_SUM);
    w[CW_HEADER_SUM] = hs.sum;
    w[CW_HEADER_XOR] = hs.x;
    bool ok = ::pwrite(fd_, w, CKPT_HEADER_BYTES, 0) == (ssize_t)CKPT_HEADER_BYTES && ::fsync(fd_) == 0;
    ok = (::close(fd_) == 0) && ok;
    fd_ = -1;
    if (ok) ok = ::rename(tmp_.c_str(), final_.c_str()) == 0;
    if (!ok) {
      if (err) *err = "cannot write " + final_ + ": " + strerror(errno);
      ::unlink(tmp_.c_str());
      return -EIO;
    }
    // the rename itself reaches the disk with the directory
    const int dfd = ::open(dir_.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
    if (dfd >= 0) {
      (void)::fsync(dfd);
      ::close(dfd);
    }
    return 0;
  }

 private:
  int fd_ = -1, cur_ = 0;
  uint64_t off_ = 0;
  std::string dir_, final_, tmp_;
  uint64_t sec_off_[CKPT_SECTIONS] = {}, sec_len_[CKPT_SECTIONS] = {};
  CkptSum sec_sum_[CKPT_SECTIONS];
};

}  // namespace kc
