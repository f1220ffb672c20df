// ckpt_file_check.cpp — stand-alone check of the checkpoint parser
// (ckpt_file.h) on hostile input; no HIP, no GPU.  Build it with the host
// compiler, best with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined ckpt_file_check.cpp -o ckpt_file_check
//   ./ckpt_file_check [IMAGE EXPECTED_CODE]...
//
// Each IMAGE file is validated from memory and must give EXPECTED_CODE (0 or a
// negative errno).  Then a checkpoint of its own (written with CkptWriter into
// a temporary directory, so the writer and the file source run too) and every
// IMAGE that was valid are put through a few hundred seeded random
// truncations and byte flips: each must be refused with -EINVAL or -EIO, and
// none may make the parser read outside the image (the sanitizers' part).
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "ckpt_file.h"

using namespace kc;

static int failures = 0;

static int validate(const std::vector<uint8_t>& img, std::string* err) {
  // the exact length, in its own allocation: a read past the end is the sanitizer's
  std::vector<uint8_t> copy(img);
  CkptMemSource src(copy.data(), copy.size());
  struct kc_checkpoint_info info;
  return ckpt_validate(src, &info, err);
}

static void expect(const char* what, const std::vector<uint8_t>& img, int want) {
  std::string err;
  const int rc = validate(img, &err);
  if (rc != want) {
    fprintf(stderr, "FAIL %s: got %d (%s), expected %d\n", what, rc, err.c_str(), want);
    ++failures;
  }
}

static void fuzz(const char* what, const std::vector<uint8_t>& good, uint64_t seed) {
  std::mt19937_64 rng(seed);
  for (int k = 0; k < 300; ++k) {
    std::vector<uint8_t> img(good);
    const int mode = k % 3;
    if (mode == 0) {
      img.resize(rng() % good.size());                       // a truncation, possibly to nothing
    } else if (mode == 1) {
      img[rng() % img.size()] ^= (uint8_t)(1u << (rng() % 8));   // one flipped bit
    } else {
      // a header word replaced outright (sizes and offsets far past the file), resealed so that
      // the structure checks, not the checksum, have to catch it
      uint64_t w[CKPT_HEADER_WORDS];
      memcpy(w, img.data(), sizeof w);
      w[CW_NC + rng() % (CW_RESERVED - CW_NC)] = rng() >> (rng() % 64);
      CkptSum hs;
      hs.add(w, CW_HEADER_SUM);
      w[CW_HEADER_SUM] = hs.sum;
      w[CW_HEADER_XOR] = hs.x;
      memcpy(img.data(), w, sizeof w);
    }
    std::string err;
    const int rc = validate(img, &err);
    // (a replaced word may by chance be the value it had, or one of the two informational ones)
    const bool fine = mode == 2 ? (rc == 0 || rc == -EIO || rc == -EINVAL) : (rc == -EIO || rc == -EINVAL);
    if (!fine) {
      fprintf(stderr, "FAIL %s fuzz %d (mode %d): got %d (%s)\n", what, k, mode, rc, err.c_str());
      ++failures;
    }
  }
}

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a small checkpoint through the writer: W = 4, widths 2, 3, 5
static std::vector<uint8_t> own_image(bool keep_trace) {
  char tmpl[] = "/tmp/kc_ckpt_check_XXXXXX";
  const char* dir = mkdtemp(tmpl);
  if (!dir) {
    perror("mkdtemp");
    exit(2);
  }
  std::string err;
  std::vector<uint8_t> img;
  {
    CkptWriter wr;
    if (wr.open(dir, &err)) {
      fprintf(stderr, "open: %s\n", err.c_str());
      exit(2);
    }
    std::mt19937_64 rng(11);
    const uint64_t lw[3] = {2, 3, 5}, n = 5, gidx = 5, distinct = 10;
    std::vector<uint64_t> v(lw, lw + 3);
    for (uint64_t k = 0; k < CKPT_COUNTER_TAIL; ++k) v.push_back(rng() % 1000);
    wr.begin(CS_COUNTERS);
    wr.append(v.data(), v.size());
    v.assign(n * 4, 0);
    for (auto& x : v) x = rng();
    wr.begin(CS_FRONTIER);
    wr.append(v.data(), v.size());
    v.assign(distinct, 0);
    for (auto& x : v) x = (rng() >> 1) | 1;
    wr.begin(CS_FPS);
    wr.append(v.data(), v.size());
    if (keep_trace) {
      for (auto& x : v) x = rng() % distinct;
      wr.begin(CS_TRACE_PARENT);
      wr.append(v.data(), v.size());
      v.assign(2, 0x0102030405060708ull);
      v[1] &= 0xffff;                                     // 10 bytes, zero-padded to 16
      wr.begin(CS_TRACE_ORD);
      wr.append(v.data(), v.size());
    }
    uint64_t w[CKPT_HEADER_WORDS] = {};
    w[CW_NC] = w[CW_NP] = w[CW_NS] = 1;
    w[CW_INVARIANTS] = 3;
    w[CW_STATE_WORDS] = 4;
    w[CW_KEEP_TRACE] = keep_trace;
    w[CW_LEVEL] = w[CW_NLEVELS] = 3;
    w[CW_LEVEL_GIDX] = gidx, w[CW_N] = n, w[CW_CAND] = 9, w[CW_CAND_TOTAL] = 30;
    w[CW_INIT] = 2, w[CW_DISTINCT] = distinct, w[CW_PEAK_FRONTIER] = 3;
    if (wr.finish(w, &err)) {
      fprintf(stderr, "finish: %s\n", err.c_str());
      exit(2);
    }
  }
  // back through the file source
  {
    CkptFileSource src;
    struct kc_checkpoint_info info;
    if (src.open(ckpt_path(dir)) || ckpt_validate(src, &info, &err) || info.distinct != 10 || info.n != 5 ||
        info.keep_trace != (int)keep_trace) {
      fprintf(stderr, "FAIL: the writer's own file does not validate (%s)\n", err.c_str());
      ++failures;
    }
    CkptFileSource none;
    if (none.open(std::string(dir) + "/nothing-here") != -ENOENT) {
      fprintf(stderr, "FAIL: a missing file is not -ENOENT\n");
      ++failures;
    }
  }
  img = slurp(ckpt_path(dir));
  ::unlink(ckpt_path(dir).c_str());
  ::rmdir(dir);
  return img;
}

int main(int argc, char** argv) {
  if (argc % 2 != 1) {
    fprintf(stderr, "usage: %s [IMAGE EXPECTED_CODE]...\n", argv[0]);
    return 2;
  }
  int given = 0, fuzzed = 0;
  for (int a = 1; a + 1 < argc; a += 2, ++given) {
    const std::vector<uint8_t> img = slurp(argv[a]);
    const int want = atoi(argv[a + 1]);
    expect(argv[a], img, want);
    if (want == 0 && !img.empty()) {
      fuzz(argv[a], img, 1000 + a);
      ++fuzzed;
    }
  }
  for (int kt = 0; kt < 2; ++kt) {
    const std::vector<uint8_t> good = own_image(kt != 0);
    expect("own image", good, 0);
    std::vector<uint8_t> bad(good);
    bad[0] ^= 1;
    expect("own image, magic", bad, -EINVAL);
    bad = good;
    bad[8] ^= 2;
    expect("own image, version", bad, -EINVAL);
    for (size_t cut : {size_t(0), size_t(7), size_t(15), size_t(100), size_t(511), good.size() - 1}) {
      bad.assign(good.begin(), good.begin() + cut);
      expect("own image, cut", bad, -EIO);
    }
    fuzz("own image", good, 5 + kt);
    ++fuzzed;
  }
  printf("ckpt_file_check: %d given images, %d images fuzzed, %d failures\n", given, fuzzed, failures);
  return failures ? 1 : 0;
}
