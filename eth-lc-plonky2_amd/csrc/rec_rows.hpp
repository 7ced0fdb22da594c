// One operation of a recursion-gate row, from operands read out of the witness matrix to every cell it owns (lcp2_rec_gate_rows).
//
// SimpleGenerator::run_once of ArithmeticGate, BaseSumGate<2>, ArithmeticExtensionGate, MulExtensionGate, ReducingGate,
// ReducingExtensionGate, PoseidonMdsGate, RandomAccessGate, ExponentiationGate and CosetInterpolationGate as ONE function: job in,
// operands through a load callback, (column, value) pairs out through a store callback.  k_rec_gate_rows (kernels_witness.hip) calls
// it with loads from the operand list / the column-major witness matrix and stores into that matrix, the level runner of
// witness_rows.hip validates a host list with rec_lists_problem, and tests/emu/emu_rec.cpp (the per-job functions) and emu_plan.cpp
// (a level's launch) compile the same text for the CPU.
// Layouts and values are those of the gate programs and integer generators in eth-lc-plonky2_amd/recursion_gates.py,
// u32_gates.py (gate_coset_interpolation / row_coset_interpolation) and circuit.py (gate_arithmetic, gate_base_sum); like them the
// layout is [RECALL] of plonky2 0.1.4 and its parity is UNPINNED.
// Every operand is canonicalised when it is read and all arithmetic is the canonical arithmetic of gl64.hpp, so every value
// written is canonical.  The one exception on the input side: the two power words of an EXPONENTIATION job are bit strings, not
// field elements, and are taken as they arrive (an IMM word is not reduced; a CELL word was canonicalised by the load).
// The operands are streamed: a job never holds more than a few of them, so the long kinds (47 and 68 operands) need no array.
#pragma once
#include "gl64.hpp"
#include "row_flag.hpp"

namespace lcp2 {

constexpr u32 REC_ARITHMETIC = 0, REC_BASE_SUM = 1, REC_ARITHMETIC_EXT = 2, REC_MUL_EXT = 3, REC_REDUCING = 4, REC_REDUCING_EXT = 5,
              REC_POSEIDON_MDS = 6, REC_RANDOM_ACCESS = 7, REC_EXPONENTIATION = 8, REC_COSET_INTERPOLATION = 9, REC_KINDS = 10;
constexpr u32 REC_IMM = 0, REC_CELL = 1;
// the shape of each gate (circuit.py ARITH_OPS, BASE_SUM_LIMBS; recursion_gates.py ARITH_EXT_OPS ... ; u32_gates.py COSET_*)
constexpr u32 REC_ARITH_OPS = 20, REC_BASE_SUM_LIMBS = 63, REC_ARITH_EXT_OPS = 10, REC_MUL_EXT_OPS = 13, REC_REDUCING_COEFFS = 43,
              REC_REDUCING_EXT_COEFFS = 32, REC_RA_BITS = 4, REC_RA_COPIES = 4, REC_RA_ITEMS = 16, REC_RA_ROUTED = 18 * 4 + 2,
              REC_EXP_BITS = 66, REC_COSET_POINTS = 16, REC_COSET_DEGREE = 8;
constexpr u32 REC_ROW_COLUMNS = 135;  // lcp2_rec_gate_rows asks for ncols >= 135; the highest column a job writes is 133 (ExponentiationGate)

struct RecOperandDev {  // = lcp2_rec_operand
  uint64_t v;
  uint32_t col, src;
};
struct RecJobDev {  // = lcp2_rec_job
  uint32_t row;
  uint16_t kind, op;
  uint32_t first_operand, reserved;
};

LCP2_HD u32 rec_kind_ops(u32 kind) {
  return kind == REC_ARITHMETIC ? REC_ARITH_OPS : kind == REC_ARITHMETIC_EXT ? REC_ARITH_EXT_OPS : kind == REC_MUL_EXT ? REC_MUL_EXT_OPS
       : kind == REC_RANDOM_ACCESS ? REC_RA_COPIES + 1 : kind < REC_KINDS ? 1 : 0;
}
LCP2_HD u32 rec_kind_operands(u32 kind, u32 op) {
  switch (kind) {
    case REC_ARITHMETIC: return 5;
    case REC_BASE_SUM: return 1;
    case REC_ARITHMETIC_EXT: return 8;
    case REC_MUL_EXT: return 5;
    case REC_REDUCING: return 4 + REC_REDUCING_COEFFS;
    case REC_REDUCING_EXT: return 4 + 2 * REC_REDUCING_EXT_COEFFS;
    case REC_POSEIDON_MDS: return 24;
    case REC_RANDOM_ACCESS: return op < REC_RA_COPIES ? 1 + REC_RA_ITEMS : 2;
    case REC_EXPONENTIATION: return 3;
    case REC_COSET_INTERPOLATION: return 1 + 2 * REC_COSET_POINTS + 2;
    default: return 0;
  }
}

// Structure.  0: the job may read its operands and write its cells; otherwise why lcp2_rec_gate_rows refuses it (rec_problem_str)
LCP2_HD u32 rec_job_problem(const RecJobDev &j, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  if (j.row >= n) return 1;
  if (j.kind >= REC_KINDS) return 2;
  if (j.op >= rec_kind_ops(j.kind)) return 3;
  const u32 count = rec_kind_operands(j.kind, j.op);
  if ((u64)j.first_operand + count > noperands) return 4;
  for (u32 k = 0; k < count; k++) {
    const RecOperandDev &o = operands[(u64)j.first_operand + k];
    if (o.src > REC_CELL) return 5;
    if (o.src == REC_CELL && o.col >= ncols) return 6;
    if (o.src == REC_CELL && o.v >= n) return 7;
  }
  return 0;
}
// Values.  The operand of a job whose value can make the job refusable (-1: none), and the verdict on that value, canonical
LCP2_HD int rec_value_operand(u32 kind, u32 op) {
  return kind == REC_BASE_SUM || kind == REC_COSET_INTERPOLATION || (kind == REC_RANDOM_ACCESS && op < REC_RA_COPIES) ? 0
       : kind == REC_EXPONENTIATION ? 2 : -1;
}
LCP2_HD u32 rec_value_problem(u32 kind, u64 v) {
  if (kind == REC_BASE_SUM && v >> REC_BASE_SUM_LIMBS) return 8;
  if (kind == REC_RANDOM_ACCESS && v >= REC_RA_ITEMS) return 9;
  if (kind == REC_EXPONENTIATION && v > 3) return 10;
  if (kind == REC_COSET_INTERPOLATION && v == 0) return 11;
  return 0;
}
inline const char *rec_problem_str(u32 problem) {
  switch (problem) {
    case 1: return "row out of range";
    case 2: return "unknown kind";
    case 3: return "operation slot out of range for the gate";
    case 4: return "operands run past the end of the operand list";
    case 5: return "operand src above 1";
    case 6: return "cell operand column out of range";
    case 7: return "cell operand row out of range";
    case 8: return "base-sum value of 2^63 or more";
    case 9: return "random-access index of 16 or more";
    case 10: return "exponentiation high power word above 3";
    case 11: return "coset-interpolation shift is zero";
    default: return "ok";
  }
}
// A HOST list checked completely, as lcp2_rec_gate_rows and lcp2_witness_plan_rows do before they queue anything: the structure of
// every job, and the value condition of an operand that is IMM.  problem 0: nothing to refuse; otherwise the first refused job
struct RecListProblem {
  u32 problem;
  u64 job;
};
inline RecListProblem rec_lists_problem(const RecJobDev *jobs, u64 njobs, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  for (u64 i = 0; i < njobs; i++) {
    u32 problem = rec_job_problem(jobs[i], operands, noperands, ncols, n);
    const int checked = problem ? -1 : rec_value_operand(jobs[i].kind, jobs[i].op);
    if (checked >= 0 && operands[(u64)jobs[i].first_operand + checked].src == REC_IMM)
      problem = rec_value_problem(jobs[i].kind, gl_canon(operands[(u64)jobs[i].first_operand + checked].v));
    if (problem) return {problem, i};
  }
  return {0, 0};
}

// the subgroup H of order 16 (u32_gates._coset_domain) and its barycentric weights 1 / prod_{j != i} (x_i - x_j)
// (u32_gates._barycentric_weights); tests/test_rec_rows.py pins both tables to the Python functions
LCP2_HD u64 rec_coset_domain(u32 i) {
  constexpr u64 t[REC_COSET_POINTS] = {
      0x0000000000000001ull, 0xEFFFFFFF00000001ull, 0xFFFFFFFEFF000001ull, 0x000FFFFFFFF00000ull, 0x0001000000000000ull, 0x0000000000001000ull,
      0xFFFFFEFF00000101ull, 0xFFFFFFEF00000001ull, 0xFFFFFFFF00000000ull, 0x1000000000000000ull, 0x0000000001000000ull, 0xFFEFFFFF00100001ull,
      0xFFFEFFFF00000001ull, 0xFFFFFFFEFFFFF001ull, 0x000000FFFFFFFF00ull, 0x0000001000000000ull};
  return t[i];
}
LCP2_HD u64 rec_coset_weight(u32 i) {
  constexpr u64 t[REC_COSET_POINTS] = {
      0xEFFFFFFF10000001ull, 0xFEFFFFFF00000001ull, 0xFFFFFFFEFFF00001ull, 0x0000FFFFFFFF0000ull, 0x0000100000000000ull, 0x0000000000000100ull,
      0xFFFFFFEF00000011ull, 0xFFFFFFFE00000001ull, 0x0FFFFFFFF0000000ull, 0x0100000000000000ull, 0x0000000000100000ull, 0xFFFEFFFF00010001ull,
      0xFFFFEFFF00000001ull, 0xFFFFFFFEFFFFFF01ull, 0x0000000FFFFFFFF0ull, 0x0000000100000000ull};
  return t[i];
}

// one output of the Poseidon MDS layer over one component: sum_i s[(i + r) % 12] circ[i] + s[r] diag[r].  The coefficients sum
// to 264, so the halves of the operands are summed apart (each sum < 2^41) and the 73-bit total is reduced once
LCP2_HD u64 rec_mds_row(const u64 *s, u32 r) {
  constexpr u32 circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
  u64 lo = 0, hi = 0;
#pragma unroll
  for (u32 i = 0; i < 12; i++) {
    const u64 x = s[(i + r) % 12];
    lo += (x & GL_EPS) * circ[i];
    hi += (x >> 32) * circ[i];
  }
  if (r == 0) {  // MDS_DIAG = [8, 0, ..]
    lo += (s[0] & GL_EPS) * 8;
    hi += (s[0] >> 32) * 8;
  }
  const u64 low = lo + (hi << 32);
  return gl_reduce128(low, (hi >> 32) + (low < lo ? 1 : 0));
}

template <class Put>
LCP2_HD void rec_put2(Put &put, u32 col, gl2 v) {
  put(col, v.c0);
  put(col + 1, v.c1);
}

// every cell of a VALID job (rec_job_problem == 0, rec_value_problem == 0): get(k) is operand k as it arrives, put(column, canonical value)
template <class Get, class Put>
LCP2_HD void rec_job_cells(const RecJobDev &j, Get get, Put put) {
  const u32 op = j.op;
  auto in = [&](u32 k) -> u64 { return gl_canon(get(k)); };
  auto in2 = [&](u32 k) -> gl2 { return gl2_make(gl_canon(get(k)), gl_canon(get(k + 1))); };
  switch (j.kind) {
    case REC_ARITHMETIC: {  // multiplicand_0, multiplicand_1, addend, output = c0 m0 m1 + c1 addend
      const u64 c0 = in(0), c1 = in(1), m0 = in(2), m1 = in(3), addend = in(4);
      const u32 w = 4 * op;
      put(w, m0); put(w + 1, m1); put(w + 2, addend);
      put(w + 3, gl_add(gl_mul(gl_mul(m0, m1), c0), gl_mul(addend, c1)));
      break;
    }
    case REC_BASE_SUM: {  // the sum, then its 63 bits, least significant first
      const u64 v = in(0);
      put(0, v);
      for (u32 i = 0; i < REC_BASE_SUM_LIMBS; i++) put(1 + i, (v >> i) & 1);
      break;
    }
    case REC_ARITHMETIC_EXT: {
      const u64 c0 = in(0), c1 = in(1);
      const gl2 m0 = in2(2), m1 = in2(4), addend = in2(6);
      const u32 w = 8 * op;
      rec_put2(put, w, m0); rec_put2(put, w + 2, m1); rec_put2(put, w + 4, addend);
      rec_put2(put, w + 6, gl2_add(gl2_scale(gl2_mul(m0, m1), c0), gl2_scale(addend, c1)));
      break;
    }
    case REC_MUL_EXT: {
      const u64 c0 = in(0);
      const gl2 m0 = in2(1), m1 = in2(3);
      const u32 w = 6 * op;
      rec_put2(put, w, m0); rec_put2(put, w + 2, m1);
      rec_put2(put, w + 4, gl2_scale(gl2_mul(m0, m1), c0));
      break;
    }
    case REC_REDUCING: {  // output, alpha, old_acc, 43 coefficients, 42 accumulators: acc_i = acc_{i-1} alpha + coeff_i
      const gl2 alpha = in2(0);
      gl2 acc = in2(2);
      rec_put2(put, 2, alpha); rec_put2(put, 4, acc);
      for (u32 i = 0; i < REC_REDUCING_COEFFS; i++) {
        const u64 c = in(4 + i);
        put(6 + i, c);
        acc = gl2_add_base(gl2_mul(acc, alpha), c);
        rec_put2(put, i + 1 < REC_REDUCING_COEFFS ? 6 + REC_REDUCING_COEFFS + 2 * i : 0, acc);
      }
      break;
    }
    case REC_REDUCING_EXT: {
      const gl2 alpha = in2(0);
      gl2 acc = in2(2);
      rec_put2(put, 2, alpha); rec_put2(put, 4, acc);
      for (u32 i = 0; i < REC_REDUCING_EXT_COEFFS; i++) {
        const gl2 c = in2(4 + 2 * i);
        rec_put2(put, 6 + 2 * i, c);
        acc = gl2_add(gl2_mul(acc, alpha), c);
        rec_put2(put, i + 1 < REC_REDUCING_EXT_COEFFS ? 6 + 2 * REC_REDUCING_EXT_COEFFS + 2 * i : 0, acc);
      }
      break;
    }
    case REC_POSEIDON_MDS: {  // the layer is base-field linear: component by component
      for (u32 k = 0; k < 2; k++) {
        u64 s[12];
#pragma unroll
        for (u32 i = 0; i < 12; i++) {
          s[i] = in(2 * i + k);
          put(2 * i + k, s[i]);
        }
#pragma unroll
        for (u32 r = 0; r < 12; r++) put(24 + 2 * r + k, rec_mds_row(s, r));
      }
      break;
    }
    case REC_RANDOM_ACCESS: {
      if (op == REC_RA_COPIES) {  // the two extra constants
        put(18 * REC_RA_COPIES, in(0));
        put(18 * REC_RA_COPIES + 1, in(1));
        break;
      }
      const u64 index = in(0);
      const u32 base = 18 * op;
      u64 claimed = 0;
      put(base, index);
      for (u32 i = 0; i < REC_RA_ITEMS; i++) {
        const u64 item = in(1 + i);
        put(base + 2 + i, item);
        claimed = i == index ? item : claimed;
      }
      put(base + 1, claimed);
      for (u32 i = 0; i < REC_RA_BITS; i++) put(REC_RA_ROUTED + REC_RA_BITS * op + i, (index >> i) & 1);
      break;
    }
    case REC_EXPONENTIATION: {  // base, 66 power bits, output, 66 intermediates: square and multiply from the top bit down
      const u64 base = in(0), lo = get(1), hi = in(2);
      put(0, base);
      u64 cur = 1;
      for (u32 i = 0; i < REC_EXP_BITS; i++) {
        const u32 b = REC_EXP_BITS - 1 - i;
        const u64 bit = b < 64 ? (lo >> b) & 1 : (hi >> (b - 64)) & 1;
        if (i) cur = gl_sqr(cur);
        if (bit) cur = gl_mul(cur, base);
        put(1 + b, bit);
        put(2 + REC_EXP_BITS + i, cur);
      }
      put(1 + REC_EXP_BITS, cur);
      break;
    }
    case REC_COSET_INTERPOLATION: {  // barycentric evaluation in chunks of 8, 7 and 1 points (u32_gates.row_coset_interpolation)
      const u64 shift = in(0);
      const gl2 point = in2(1 + 2 * REC_COSET_POINTS);
      const gl2 x = gl2_scale(point, gl_inv(shift));
      put(0, shift);
      rec_put2(put, 33, point);
      gl2 ev = gl2_make(0, 0), pr = gl2_make(1, 0);
      u32 pinned = 0;
      for (u32 i = 0; i < REC_COSET_POINTS; i++) {
        const gl2 value = in2(1 + 2 * i);
        rec_put2(put, 1 + 2 * i, value);
        const gl2 term = gl2_sub_base(x, rec_coset_domain(i));
        ev = gl2_add(gl2_mul(ev, term), gl2_mul(gl2_scale(value, rec_coset_weight(i)), pr));
        pr = gl2_mul(pr, term);
        if (i + 1 == REC_COSET_DEGREE || i + 1 == 2 * REC_COSET_DEGREE - 1) {  // the intermediate (eval, prod) pairs
          rec_put2(put, 37 + 2 * pinned, ev);
          rec_put2(put, 41 + 2 * pinned, pr);
          pinned++;
        }
      }
      rec_put2(put, 35, ev);
      rec_put2(put, 45, x);
      break;
    }
    default: break;
  }
}

// Lane i of k_rec_gate_rows over the jobs [begin, end) of one level; jobs[0] is job `base` of the list.  Returns 0 when the job
// ran (or the lane had nothing to do), else the problem of job i, which then wrote nothing: the caller folds it into the flag word
// (row_flag.hpp), so the flag names the FIRST refused job.  A lane returns at once when the flag names a job
// of an earlier level: levels after a refused one write nothing.  check_structure = false: the list passed rec_job_problem already.
LCP2_HD u64 rec_rows_lane(const RecJobDev *jobs, u64 base, u64 begin, u64 end, u64 i, const RecOperandDev *operands, u64 noperands,
                          u64 *wires, u32 ncols, u64 n, const u64 *flag, bool check_structure) {
  if (i < begin || i >= end) return 0;
  if ((*flag >> 8) < begin) return 0;
  const RecJobDev job = jobs[i - base];
  if (check_structure)
    if (const u32 problem = rec_job_problem(job, operands, noperands, ncols, n)) return problem;
  const RecOperandDev *mine = operands + job.first_operand;
  auto get = [&](u32 k) -> u64 {
    const RecOperandDev o = mine[k];
    return o.src == REC_CELL ? gl_canon(wires[(u64)o.col * n + o.v]) : o.v;
  };
  const int checked = rec_value_operand(job.kind, job.op);
  if (checked >= 0)
    if (const u32 problem = rec_value_problem(job.kind, gl_canon(get((u32)checked)))) return problem;
  u64 *W = wires + job.row;
  rec_job_cells(job, get, [&](u32 col, u64 v) { W[(u64)col * n] = v; });
  return 0;
}

}  // namespace lcp2
