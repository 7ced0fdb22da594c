// One operation of a plonky2_u32 / comparison gate row, from its inputs to every cell it owns (lcp2_u32_gate_rows).
//
// The generators of U32ArithmeticGate, U32AddManyGate, U32SubtractionGate, U32RangeCheckGate and ComparisonGate as ONE function:
// job in, (column, value) pairs out through a store callback.  k_u32_gate_rows (kernels_witness.hip) calls it with a store into
// the column-major witness matrix, lcp2_u32_gate_rows (witness_rows.hip) validates a host list with u32_job_problem, and
// tests/emu/emu_u32.cpp compiles the same text for the CPU.  Layouts and values are those of eth-lc-plonky2_amd/u32_gates.py (the docstrings of
// gate_u32_* / gate_comparison, the integer generators row_*); like them [RECALL], parity unpinned.
// Every value written is canonical: the inputs are u32, the outputs of the integer operations are below 2^34, and the two kinds
// of field element (the arithmetic gate's inverse, the comparison gate's signed differences) come from gl_inv / gl_neg.
#pragma once
#include "gl64.hpp"
#include "row_flag.hpp"

namespace lcp2 {

constexpr u32 U32_KIND_ARITHMETIC = 0, U32_KIND_ADD_MANY = 1, U32_KIND_SUBTRACTION = 2, U32_KIND_RANGE_CHECK = 3, U32_KIND_COMPARISON = 4,
              U32_KINDS = 5;
constexpr u32 U32_MAX = 0xFFFFFFFFu;
// operations per row, and the shape of each gate (u32_gates.py: U32_ARITH_OPS ... CMP_CHUNKS)
constexpr u32 U32_ARITH_OPS = 3, U32_ARITH_LIMBS = 32, U32_ADD_OPS = 5, U32_ADD_LIMBS = 18, U32_SUB_OPS = 6, U32_SUB_LIMBS = 16,
              U32_RANGE_OPS = 7, U32_RANGE_LIMBS = 16, U32_CMP_CHUNKS = 16;
constexpr u32 U32_ROW_COLUMNS = 126;  // one more than the highest column a job writes (U32SubtractionGate: 30 + 16 * 5 + 15)
constexpr u64 GL_INV_2 = 0x7FFFFFFF80000001ull, GL_INV_3 = 0xAAAAAAAA00000001ull;

struct U32JobDev {  // = lcp2_u32_job
  uint32_t row;
  uint16_t kind, op;
  uint32_t in[4];
};

LCP2_HD u32 u32_kind_ops(u32 kind) {
  return kind == U32_KIND_ARITHMETIC ? U32_ARITH_OPS : kind == U32_KIND_ADD_MANY ? U32_ADD_OPS : kind == U32_KIND_SUBTRACTION ? U32_SUB_OPS
       : kind == U32_KIND_RANGE_CHECK ? U32_RANGE_OPS : kind == U32_KIND_COMPARISON ? 1 : 0;
}

// 0: the job may run; otherwise why lcp2_u32_gate_rows refuses it (u32_problem_str)
LCP2_HD u32 u32_job_problem(const U32JobDev &j, u64 n) {
  if (j.row >= n) return 1;
  if (j.kind >= U32_KINDS) return 2;
  if (j.op >= u32_kind_ops(j.kind)) return 3;
  if (j.kind == U32_KIND_SUBTRACTION && j.in[2] > 1) return 4;
  return 0;
}
inline const char *u32_problem_str(u32 problem) {
  switch (problem) {
    case 1: return "row out of range";
    case 2: return "unknown kind";
    case 3: return "operation slot out of range for the gate";
    case 4: return "subtraction borrow above 1";
    default: return "ok";
  }
}

// `count` two-bit limbs of x, least significant first, on columns first ..
template <class Put>
LCP2_HD void u32_put_limbs(Put &put, u32 first, u64 x, u32 count) {
  for (u32 j = 0; j < count; j++) put(first + j, (x >> (2 * j)) & 3);
}

// a small signed integer (|v| < 4) as a field element, and the inverse of one as a field element (0 for 0)
LCP2_HD u64 u32_small_field(int v) { return v < 0 ? GL_P - (u64)(-v) : (u64)v; }
LCP2_HD u64 u32_small_inverse(int v) {
  const int a = v < 0 ? -v : v;
  const u64 inv = a == 1 ? 1 : a == 2 ? GL_INV_2 : a == 3 ? GL_INV_3 : 0;
  return v < 0 ? GL_P - inv : inv;
}

// every cell of a VALID job (u32_job_problem == 0): put(column, canonical value)
template <class Put>
LCP2_HD void u32_job_cells(const U32JobDev &j, Put put) {
  const u32 op = j.op;
  switch (j.kind) {
    case U32_KIND_ARITHMETIC: {  // multiplicand_0, multiplicand_1, addend, output_low, output_high, inverse; 32 limbs of the output
      const u64 out = (u64)j.in[0] * j.in[1] + j.in[2];  // < 2^64: (2^32 - 1)^2 + 2^32 - 1
      const u32 lo = (u32)out, hi = (u32)(out >> 32);
      const u32 w = 6 * op;
      put(w, j.in[0]); put(w + 1, j.in[1]); put(w + 2, j.in[2]); put(w + 3, lo); put(w + 4, hi);
      // output_high = 2^32 - 1 has no inverse to give: output_low is 0 then, which satisfies the canonicity constraint with any value
      put(w + 5, hi == U32_MAX ? 0 : gl_inv((u64)(U32_MAX - hi)));
      u32_put_limbs(put, 6 * U32_ARITH_OPS + U32_ARITH_LIMBS * op, out, U32_ARITH_LIMBS);
      break;
    }
    case U32_KIND_ADD_MANY: {  // addend_0..2, carry, output_result, output_carry; 16 limbs of the result, 2 of the carry
      const u64 total = (u64)j.in[0] + j.in[1] + j.in[2] + j.in[3];  // < 2^34
      const u32 w = 6 * op;
      put(w, j.in[0]); put(w + 1, j.in[1]); put(w + 2, j.in[2]); put(w + 3, j.in[3]); put(w + 4, (u32)total); put(w + 5, total >> 32);
      u32_put_limbs(put, 6 * U32_ADD_OPS + U32_ADD_LIMBS * op, total, U32_ADD_LIMBS);
      break;
    }
    case U32_KIND_SUBTRACTION: {  // x, y, borrow, output_result, output_borrow; 16 limbs of the result
      const u64 x = j.in[0], sub = (u64)j.in[1] + j.in[2];
      const u64 borrow = x < sub ? 1 : 0;
      const u64 res = x + (borrow << 32) - sub;  // < 2^32
      const u32 w = 5 * op;
      put(w, x); put(w + 1, j.in[1]); put(w + 2, j.in[2]); put(w + 3, res); put(w + 4, borrow);
      u32_put_limbs(put, 5 * U32_SUB_OPS + U32_SUB_LIMBS * op, res, U32_SUB_LIMBS);
      break;
    }
    case U32_KIND_RANGE_CHECK: {
      put(op, j.in[0]);
      u32_put_limbs(put, U32_RANGE_OPS + U32_RANGE_LIMBS * op, j.in[0], U32_RANGE_LIMBS);
      break;
    }
    case U32_KIND_COMPARISON: {  // first <= second: inputs, result, most significant difference, 5 x 16 chunk cells, 3 bits
      const u32 a = j.in[0], b = j.in[1], nc = U32_CMP_CHUNKS;
      put(0, a); put(1, b);
      int so_far = 0;  // the difference of the most significant chunk pair that differs so far, in (-4, 4)
      for (u32 i = 0; i < nc; i++) {
        const int fc = (a >> (2 * i)) & 3, sc = (b >> (2 * i)) & 3, diff = sc - fc;
        const bool eq = diff == 0;
        const int inter = eq ? so_far : 0;
        put(4 + i, (u64)fc); put(4 + nc + i, (u64)sc);
        put(4 + 2 * nc + i, u32_small_inverse(diff));  // difference * dummy = 1 - equal
        put(4 + 3 * nc + i, eq ? 1 : 0);
        put(4 + 4 * nc + i, u32_small_field(inter));
        so_far = eq ? inter : diff;
      }
      put(3, u32_small_field(so_far));
      const u32 total = (u32)(4 + so_far);  // in [1, 7]
      for (u32 i = 0; i < 3; i++) put(4 + 5 * nc + i, (total >> i) & 1);
      put(2, (total >> 2) & 1);
      break;
    }
    default: break;
  }
}

// lane i of k_u32_gate_rows.  Returns 0 when the job ran (or the lane had nothing to do), else the problem of job i, which then
// wrote nothing: the caller folds it into the flag word (row_flag.hpp)
LCP2_HD u32 u32_rows_lane(const U32JobDev *jobs, u64 njobs, u64 i, u64 *wires, u64 n) {
  if (i >= njobs) return 0;
  const U32JobDev job = jobs[i];
  if (const u32 problem = u32_job_problem(job, n)) return problem;
  u64 *W = wires + job.row;
  u32_job_cells(job, [&](u32 col, u64 v) { W[(u64)col * n] = v; });
  return 0;
}

}  // namespace lcp2
