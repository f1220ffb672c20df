// pred.h — user-defined invariants as a flat predicate program over the packed
// state.  kubecheck/pred.py compiles TLA+-flavoured
// expressions to it; pred_eval runs it on one state, on the device (k_pred,
// pred_kernels.h) and on the host (kc_pred_eval) from the same code, as
// live_stay and cover_visit do.  Nothing here knows the model: a program names
// word indices, shifts and widths, and the caller says how many words a state
// has.
//
// An instruction is 16 bytes, two 64-bit words {hdr, opnd}:
//
//   hdr  bits  0..3   opcode (PredOp)
//        bits  4..6   compare op (PredCmp)                     leaves
//        bits  8..15  word index of field A / the popcount word; END: k
//        bits 16..21  shift of field A
//        bits 22..28  width of field A, 1..64
//        bits 32..39  word index of field B        P_LEAF_FIELD
//                     the constant, 0..64          P_LEAF_POPC
//        bits 40..45  shift of field B             P_LEAF_FIELD
//        bits 46..52  width of field B, 1..64      P_LEAF_FIELD
//   opnd              P_LEAF_CONST: the constant;  P_LEAF_SET: the membership
//                     set (bit v: value v is a member; a value >= 64 is none);
//                     P_LEAF_POPC: the mask;  otherwise 0
//
//   P_LEAF_CONST  push  A cmp opnd              A = (w[word] >> shift) & ones(width)
//   P_LEAF_SET    push  A < 64 && (opnd >> A) & 1
//   P_LEAF_FIELD  push  A cmp B
//   P_LEAF_POPC   push  popcount(w[word] & opnd) cmp constant
//   P_PUSH        push  opnd & 1
//   P_AND, P_OR   pop two bits, push their conjunction / disjunction
//   P_NOT         negate the top bit
//   P_END k       pop invariant k's verdict (0 = violated)
//
// The stack is the low bits of one uint64_t (bit 0 = top).  pred_validate
// checks everything pred_eval relies on: at most KC_PRED_MAX_INSTR
// instructions, at most KC_PRED_MAX_DEPTH bits on the stack and never fewer
// than an instruction pops, word indices below the state's word count,
// shift + width <= 64, END 0, END 1, ... in order (at most KC_PRED_MAX_INV),
// the stack empty after each END and the program ending in one.
#pragma once
#include <stdint.h>

#include "kubeapi_spec.h"

#define KC_PRED_MAX_INSTR 128
#define KC_PRED_MAX_INV 8
#define KC_PRED_MAX_DEPTH 32

namespace kc {

enum PredOp : int {
  P_LEAF_CONST = 0, P_LEAF_SET, P_LEAF_FIELD, P_LEAF_POPC, P_PUSH, P_AND, P_OR, P_NOT, P_END, P_OP_COUNT
};
enum PredCmp : int { PC_EQ = 0, PC_NE, PC_LT, PC_LE, PC_GT, PC_GE, PC_CMP_COUNT };

struct PredInstr {
  uint64_t hdr, opnd;
};
static_assert(sizeof(PredInstr) == 16, "a predicate instruction is 16 bytes");

struct PredProgram {
  const PredInstr* code;
  int n;
};

KC_HD uint64_t pred_field(const uint64_t* w, uint64_t h) {
  return (w[(h >> 8) & 0xff] >> ((h >> 16) & 63)) & (~0ull >> (64 - ((h >> 22) & 127)));
}
KC_HD bool pred_cmp(unsigned c, uint64_t a, uint64_t b) {
  const bool eq = a == b, lt = a < b;
  bool r = eq;                       // PC_EQ
  r = c == PC_NE ? !eq : r;
  r = c == PC_LT ? lt : r;
  r = c == PC_LE ? (lt || eq) : r;
  r = c == PC_GT ? !(lt || eq) : r;
  r = c == PC_GE ? !lt : r;
  return r;
}

// The invariants `state_words` violates: bit k = invariant k is FALSE there.
// The program has passed pred_validate.
KC_HD uint32_t pred_eval(const uint64_t* state_words, const PredProgram& p) {
  uint64_t st = 0;
  uint32_t viol = 0;
  for (int i = 0; i < p.n; ++i) {
    const uint64_t h = p.code[i].hdr, x = p.code[i].opnd;
    const unsigned op = (unsigned)(h & 15), c = (unsigned)((h >> 4) & 7);
    if (op <= P_PUSH) {
      bool b;
      if (op == P_LEAF_POPC) {
        b = pred_cmp(c, (uint64_t)popc(state_words[(h >> 8) & 0xff] & x), (h >> 32) & 0xff);
      } else if (op == P_PUSH) {
        b = (x & 1) != 0;
      } else {
        const uint64_t a = pred_field(state_words, h);
        if (op == P_LEAF_FIELD) b = pred_cmp(c, a, pred_field(state_words, h >> 24));
        else if (op == P_LEAF_SET) b = a < 64 && ((x >> (a & 63)) & 1);
        else b = pred_cmp(c, a, x);
      }
      st = (st << 1) | (b ? 1u : 0u);
    } else if (op == P_AND) {
      st = (st >> 1) & (st | ~1ull);
    } else if (op == P_OR) {
      st = (st >> 1) | (st & 1);
    } else if (op == P_NOT) {
      st ^= 1;
    } else {                         // P_END
      viol |= (uint32_t)(~st & 1) << ((h >> 8) & 7);
      st >>= 1;
    }
  }
  return viol;
}

// The number of invariants of a program that pred_eval may run on states of
// `W` words, or -1 with *why set to what is wrong.
inline int pred_validate(const PredInstr* code, int n, int W, const char** why) {
  static const char* kWhy = nullptr;
  if (!why) why = &kWhy;
  if (n < 1 || n > KC_PRED_MAX_INSTR || !code) {
    *why = "a program has 1 to 128 instructions";
    return -1;
  }
  int depth = 0, inv = 0;
  auto field_ok = [&](uint64_t h) {
    const int word = (int)((h >> 8) & 0xff), shift = (int)((h >> 16) & 63), width = (int)((h >> 22) & 127);
    return word < W && width >= 1 && shift + width <= 64;
  };
  for (int i = 0; i < n; ++i) {
    const uint64_t h = code[i].hdr;
    const int op = (int)(h & 15), c = (int)((h >> 4) & 7);
    if (op >= P_OP_COUNT) { *why = "unknown opcode"; return -1; }
    if (op <= P_LEAF_POPC && op != P_LEAF_SET && c >= PC_CMP_COUNT) { *why = "unknown compare op"; return -1; }
    if (op <= P_PUSH) {
      if (op == P_LEAF_POPC) {
        if ((int)((h >> 8) & 0xff) >= W) { *why = "word index outside the state"; return -1; }
        if (((h >> 32) & 0xff) > 64) { *why = "a popcount is compared with 0..64"; return -1; }
      } else if (op != P_PUSH) {
        if (!field_ok(h) || (op == P_LEAF_FIELD && !field_ok(h >> 24))) {
          *why = "field outside the state (word index, or shift + width > 64)";
          return -1;
        }
      }
      if (++depth > KC_PRED_MAX_DEPTH) { *why = "nesting deeper than 32"; return -1; }
    } else if (op == P_AND || op == P_OR) {
      if (depth < 2) { *why = "AND / OR on fewer than two bits"; return -1; }
      --depth;
    } else if (op == P_NOT) {
      if (depth < 1) { *why = "NOT on an empty stack"; return -1; }
    } else {
      if (depth != 1) { *why = "END with other than one bit on the stack"; return -1; }
      if ((int)((h >> 8) & 0xff) != inv) { *why = "END k out of order"; return -1; }
      if (++inv > KC_PRED_MAX_INV) { *why = "more than 8 invariants"; return -1; }
      depth = 0;
    }
  }
  if ((code[n - 1].hdr & 15) != P_END) { *why = "the program does not end in END"; return -1; }
  return inv;
}

// k_pred's results, one block per launch sequence (a level):
//   [0]        min over the violating states of (state index << 8 | k), ~0 = none
//   [1]        states evaluated
//   [2 + k]    states violating invariant k
constexpr int PRED_OUT_WORDS = 2 + KC_PRED_MAX_INV;

// k_pred (pred.hip) over n packed states of W words on `stream` (a
// hipStream_t); state i counts as index base + i.  d_prog holds n_instr
// validated instructions in device memory.
int pred_launch(int W, const void* states, uint64_t n, uint64_t base, const PredInstr* d_prog, int n_instr,
                unsigned long long* d_out, void* stream);
// a result block as a level starts it: no key, every count zero (enqueued on `stream`)
int pred_reset(unsigned long long* d_out, void* stream);

}  // namespace kc
