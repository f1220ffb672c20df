// pred_host_check.cpp — pred.h's host path in a program of its own (host
// compiler, no HIP): a handful of programs validated and evaluated on
// hand-made state words, each answer compared with the value worked out by
// hand.  Built with -fsanitize=address,undefined by tests/test_pred_host.py;
// not part of libkubecheck.so.
#include <stdio.h>

#include <vector>

#include "pred.h"

using namespace kc;

namespace {

int failures = 0;

uint64_t fbits(int word, int shift, int width) {
  return ((uint64_t)word << 8) | ((uint64_t)shift << 16) | ((uint64_t)width << 22);
}
PredInstr leaf(int word, int shift, int width, int cmp, uint64_t c) {
  return PredInstr{(uint64_t)P_LEAF_CONST | ((uint64_t)cmp << 4) | fbits(word, shift, width), c};
}
PredInstr op(int o, int k = 0) { return PredInstr{(uint64_t)o | ((uint64_t)k << 8), 0}; }

// the program and the words live in exactly sized heap blocks, so a read past either end is ASan's to report
void expect(const char* what, const std::vector<PredInstr>& code, const std::vector<uint64_t>& w, int ninv,
            uint32_t want) {
  const char* why = nullptr;
  const int got_inv = pred_validate(code.data(), (int)code.size(), (int)w.size(), &why);
  if (got_inv != ninv) {
    printf("FAIL %s: validate gave %d (%s), expected %d\n", what, got_inv, why ? why : "", ninv);
    ++failures;
    return;
  }
  if (ninv < 0) return;
  const uint32_t got = pred_eval(w.data(), PredProgram{code.data(), (int)code.size()});
  if (got != want) {
    printf("FAIL %s: eval gave %u, expected %u\n", what, got, want);
    ++failures;
  }
}

}  // namespace

int main() {
  const std::vector<uint64_t> w4 = {0x8000000000000005ull, 0x1234, 0, 0xFFFF000000000000ull};
  // a field in the top bits of the last word, a full-width field, and bit 63 alone
  expect("top field", {leaf(3, 48, 16, PC_EQ, 0xFFFF), op(P_END)}, w4, 1, 0);
  expect("top field ne", {leaf(3, 48, 16, PC_NE, 0xFFFF), op(P_END)}, w4, 1, 1);
  expect("whole word", {leaf(0, 0, 64, PC_EQ, 0x8000000000000005ull), op(P_END)}, w4, 1, 0);
  expect("bit 63", {leaf(0, 63, 1, PC_EQ, 1), op(P_END)}, w4, 1, 0);
  // orderings are unsigned
  expect("unsigned lt", {leaf(0, 0, 64, PC_LT, 5), op(P_END)}, w4, 1, 1);
  expect("ge", {leaf(1, 4, 4, PC_GE, 3), op(P_END)}, w4, 1, 0);
  expect("gt", {leaf(1, 4, 4, PC_GT, 3), op(P_END)}, w4, 1, 1);
  expect("le", {leaf(1, 4, 4, PC_LE, 2), op(P_END)}, w4, 1, 1);
  // popcount: the mask leaves the ghost bit out (2 bits), or takes it in (3)
  expect("popc", {PredInstr{(uint64_t)P_LEAF_POPC | (PC_EQ << 4) | (2ull << 32), 0x7FFFFFFFFFFFFFFFull}, op(P_END)}, w4, 1, 0);
  expect("popc ghost", {PredInstr{(uint64_t)P_LEAF_POPC | (PC_EQ << 4) | (3ull << 32), ~0ull}, op(P_END)}, w4, 1, 0);
  expect("popc 64", {PredInstr{(uint64_t)P_LEAF_POPC | (PC_LE << 4) | (64ull << 32), ~0ull}, op(P_END)}, w4, 1, 0);
  // membership: value 4 in {4, 63}; a 7-bit value of 64 or more is in no set
  expect("set", {PredInstr{(uint64_t)P_LEAF_SET | fbits(1, 0, 3), (1ull << 4) | (1ull << 63)}, op(P_END)}, w4, 1, 0);
  expect("set 63", {PredInstr{(uint64_t)P_LEAF_SET | fbits(3, 48, 6), 1ull << 63}, op(P_END)}, w4, 1, 0);
  expect("set wide", {PredInstr{(uint64_t)P_LEAF_SET | fbits(3, 48, 7), ~0ull}, op(P_END)}, w4, 1, 1);
  // two fields: 0x3 (word 1 bits 4..7) against 0x2 (bits 8..11)
  expect("fields", {PredInstr{(uint64_t)P_LEAF_FIELD | (PC_GT << 4) | fbits(1, 4, 4) | (fbits(1, 8, 4) << 24), 0}, op(P_END)},
         w4, 1, 0);
  // connectives and several invariants: k = 0 holds, 1 is violated, 2 holds
  expect("three invariants",
         {leaf(1, 0, 4, PC_EQ, 4), leaf(1, 4, 4, PC_EQ, 9), op(P_OR), op(P_END, 0),
          leaf(1, 0, 4, PC_EQ, 4), leaf(1, 4, 4, PC_EQ, 9), op(P_AND), op(P_END, 1),
          PredInstr{P_PUSH, 0}, op(P_NOT), op(P_END, 2)},
         w4, 3, 2);
  // the limits: 128 instructions and depth 32 pass, 129 and 33 do not
  std::vector<PredInstr> longest;
  for (int k = 0; k < 8; ++k) {
    longest.push_back(leaf(1, 0, 4, PC_EQ, 4));
    for (int j = 0; j < 7; ++j) {
      longest.push_back(leaf(1, 4, 4, PC_EQ, 3));
      longest.push_back(op(P_AND));
    }
    longest.push_back(op(P_END, k));
  }
  expect("128 instructions", longest, w4, 8, 0);
  std::vector<PredInstr> over = longest;
  over.insert(over.begin() + 1, op(P_NOT));
  expect("129 instructions", over, w4, -1, 0);
  std::vector<PredInstr> deep(32, leaf(1, 0, 4, PC_EQ, 4));
  deep.insert(deep.end(), 31, op(P_AND));
  deep.push_back(op(P_END));
  expect("depth 32", deep, w4, 1, 0);
  deep.insert(deep.begin(), leaf(1, 0, 4, PC_EQ, 4));
  deep.insert(deep.end() - 1, op(P_AND));
  expect("depth 33", deep, w4, -1, 0);
  // what validation refuses
  expect("word outside", {leaf(4, 0, 4, PC_EQ, 0), op(P_END)}, w4, -1, 0);
  expect("shift + width", {leaf(1, 61, 4, PC_EQ, 0), op(P_END)}, w4, -1, 0);
  expect("width 0", {leaf(1, 0, 0, PC_EQ, 0), op(P_END)}, w4, -1, 0);
  expect("field B outside",
         {PredInstr{(uint64_t)P_LEAF_FIELD | fbits(1, 0, 4) | (fbits(7, 0, 4) << 24), 0}, op(P_END)}, w4, -1, 0);
  expect("underflow", {op(P_AND), op(P_END)}, w4, -1, 0);
  expect("no END", {leaf(1, 0, 4, PC_EQ, 4)}, w4, -1, 0);
  expect("END order", {leaf(1, 0, 4, PC_EQ, 4), op(P_END, 1)}, w4, -1, 0);
  expect("popc word", {PredInstr{(uint64_t)P_LEAF_POPC | (6ull << 8), 1}, op(P_END)}, w4, -1, 0);
  // a six-word state: the last word is reachable, the seventh is not
  const std::vector<uint64_t> w6 = {0, 0, 0, 0, 0, 0xAB00000000000000ull};
  expect("W = 6 last word", {leaf(5, 56, 8, PC_EQ, 0xAB), op(P_END)}, w6, 1, 0);
  expect("W = 6 word 6", {leaf(6, 0, 8, PC_EQ, 0), op(P_END)}, w6, -1, 0);
  if (failures) {
    printf("pred_host_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("pred_host_check: ok\n");
  return 0;
}
