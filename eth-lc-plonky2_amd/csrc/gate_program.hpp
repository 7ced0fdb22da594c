// The gate-program format of include/lcp2.h in code, once, for every HOST reader of a program: the instruction, its checks, and
// the straight-line walk over an algebra (F_p^2 values at zeta: verifier.hip; extension targets: host/recursion.cpp; degree
// bounds: prover_build.hip).  Plain C++17 without HIP or field arithmetic, so that host/*.cpp and tools/gen/ include it too.
// K6 interprets the staged encoding (quotient_common.hpp) and the oracle restates the format independently; the one device reader of
// this text is the batch verifier's identity kernel (kernels_verify_head.hip), for which the instruction and the walk are marked
// GP_HD (host and device under hipcc, nothing elsewhere) and the registers are any type with operator[].
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/lcp2.h"

#if defined(__HIPCC__)
#define GP_HD __host__ __device__
#else
#define GP_HD
#endif
// unrolling is asked for in device code only (there it keeps the PMDS window in registers); every host build compiles the loops as written
#if defined(__HIP_DEVICE_COMPILE__)
#define GP_UNROLL _Pragma("unroll")
#else
#define GP_UNROLL
#endif

namespace gate_program {

enum : uint32_t { KIND_REG = 0, KIND_WIRE = 1, KIND_CONST = 2, KIND_IMM = 3, KIND_PI = 4 };
inline bool is_column(uint32_t kind) { return kind == KIND_WIRE || kind == KIND_CONST; }  // read from the trace, not from the program

// Poseidon MDS layer (LCP2_OP_PMDS): row r = sum_i x[(i + r) % 12] MDS_CIRC[i] + x[r] MDS_DIAG[r]
constexpr uint32_t MDS_WIDTH = 12;
inline constexpr uint64_t MDS_CIRC[MDS_WIDTH] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
inline constexpr uint64_t MDS_DIAG[MDS_WIDTH] = {8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// one instruction (two words): source k is of kind[k] at idx[k].  No reader looks at the bits outside these fields; encode() zeroes them.
struct Insn {
  uint32_t op, dst, kind[2], idx[2];
  GP_HD Insn(uint32_t w0, uint32_t w1) : op(w0 & 0xF), dst((w0 >> 8) & 0xFF), kind{(w0 >> 16) & 0xF, (w0 >> 20) & 0xF}, idx{w1 & 0xFFFF, w1 >> 16} {}
  void encode(uint32_t w[2]) const { w[0] = op | dst << 8 | kind[0] << 16 | kind[1] << 20; w[1] = idx[0] | idx[1] << 16; }
  GP_HD bool emits() const { return op == LCP2_OP_EMIT || op == LCP2_OP_EMITBOOL; }
  GP_HD bool pmds() const { return op == LCP2_OP_PMDS; }
  // operands that are single values of kind[k].  A PMDS has none: idx[0] is a window of 12 registers, idx[1] a block of 12 immediates.
  int nsrc() const { return pmds() ? 0 : (emits() || op == LCP2_OP_SBOX) ? 1 : 2; }
  // one past the highest register read or written
  uint32_t top_reg() const {
    if (pmds()) return (dst > idx[0] ? dst : idx[0]) + MDS_WIDTH;
    uint32_t top = emits() ? 0 : dst + 1;
    for (int k = 0; k < nsrc(); k++)
      if (kind[k] == KIND_REG && idx[k] + 1 > top) top = idx[k] + 1;
    return top;
  }
};

// what an operand index is checked against; UNCHECKED where the caller does not know the table
constexpr size_t UNCHECKED = ~(size_t)0;
struct Limits { size_t regs, wires = UNCHECKED, consts = UNCHECKED, imms = UNCHECKED, pis = UNCHECKED; };

// nullptr, or why no walker may run the instruction
inline const char *insn_problem(const Insn &in, const Limits &L) {
  if (in.op > LCP2_OP_PMDS) return "bad instruction";
  if (in.pmds()) {
    if ((size_t)in.dst + MDS_WIDTH > L.regs || (size_t)in.idx[0] + MDS_WIDTH > L.regs) return "PMDS window out of range";
    // its kind fields (no walker reads them) are held to REG, IMM together with the block of immediates
    if (L.imms != UNCHECKED && (in.kind[0] != KIND_REG || in.kind[1] != KIND_IMM || (size_t)in.idx[1] + MDS_WIDTH > L.imms)) return "PMDS window out of range";
    return nullptr;
  }
  if (!in.emits() && in.dst >= L.regs) return "bad instruction";
  for (int k = 0; k < in.nsrc(); k++) {
    const uint32_t kind = in.kind[k];
    const size_t lim = kind == KIND_REG ? L.regs : kind == KIND_WIRE ? L.wires : kind == KIND_CONST ? L.consts : kind == KIND_IMM ? L.imms : kind == KIND_PI ? L.pis : 0;
    if (in.idx[k] >= lim) return "operand out of range";
  }
  return nullptr;
}

// The straight-line walk of instructions [first, first + len) of `code` over an algebra:
//   Alg::V  a value, Alg::S a scalar of the base field (an MDS coefficient, a power of alpha)
//   V wire(i), gate_const(i), pi(i), imm(u64);  S scalar(u64), scalar_mul(S, S)
//   V add(a, b), sub(a, b), mul(a, b), mul_add(a, b, acc) = a b + acc, scale_add(x, s, acc) = x s + acc
// `imm` is the table of immediates, of either 64-bit unsigned type (null: every immediate reads as 0, for an algebra that ignores
// the values); regs (a pointer, or any type whose operator[] gives a V &) holds the registers the programs were validated for;
// on_emit(V) receives the constraints in program order.
// THE ORDER OF THE ALGEBRA CALLS IS PART OF THE CONTRACT: over targets every call adds gates to a circuit, and another order or
// an unfused mul + add where one mul_add stands gives another circuit with another digest (tests/cpp/test_gadgets.cpp pins them).
template <class Alg, class Word, class Regs, class Emit>
GP_HD void walk_program(Alg &A, const uint32_t *code, size_t first, size_t len, const Word *imm, Regs regs, Emit on_emit) {
  using V = typename Alg::V;
  auto immediate = [&](uint32_t i) { return A.imm(imm ? imm[i] : 0); };
  for (size_t pc = first; pc < first + len; pc++) {
    const Insn in(code[2 * pc], code[2 * pc + 1]);
    auto fetch = [&](int k) -> V {
      const uint32_t kind = in.kind[k], i = in.idx[k];
      return kind == KIND_REG ? regs[i] : kind == KIND_WIRE ? A.wire(i) : kind == KIND_CONST ? A.gate_const(i) : kind == KIND_IMM ? immediate(i) : A.pi(i);
    };
    if (in.pmds()) {
      V x[MDS_WIDTH];  // the two windows may be the same (unrolled: on the device x stays in registers)
      GP_UNROLL
      for (uint32_t i = 0; i < MDS_WIDTH; i++) x[i] = regs[in.idx[0] + i];
      GP_UNROLL
      for (uint32_t r = 0; r < MDS_WIDTH; r++) {
        V t = immediate(in.idx[1] + r);
        if (MDS_DIAG[r]) t = A.scale_add(x[r], A.scalar(MDS_DIAG[r]), t);
        GP_UNROLL
        for (uint32_t i = 0; i < MDS_WIDTH; i++) t = A.scale_add(x[(i + r) % MDS_WIDTH], A.scalar(MDS_CIRC[i]), t);
        regs[in.dst + r] = t;
      }
      continue;
    }
    const V a = fetch(0);
    if (in.op == LCP2_OP_EMIT) { on_emit(a); continue; }
    if (in.op == LCP2_OP_EMITBOOL) { on_emit(A.sub(A.mul(a, a), a)); continue; }
    if (in.op == LCP2_OP_SBOX) { const V x2 = A.mul(a, a), x4 = A.mul(x2, x2), x3 = A.mul(x2, a); regs[in.dst] = A.mul(x3, x4); continue; }
    const V b = fetch(1);
    switch (in.op) {
      case LCP2_OP_ADD: regs[in.dst] = A.add(a, b); break;
      case LCP2_OP_SUB: regs[in.dst] = A.sub(a, b); break;
      case LCP2_OP_MUL: regs[in.dst] = A.mul(a, b); break;
      case LCP2_OP_XOR: { const V ab = A.mul(a, b); regs[in.dst] = A.sub(A.sub(A.add(a, b), ab), ab); break; }
      case LCP2_OP_DBLADD: regs[in.dst] = A.add(A.add(a, a), b); break;
      default: regs[in.dst] = A.mul_add(a, b, regs[in.dst]); break;  // LCP2_OP_MULADD
    }
  }
}

// plonk/vanishing_poly.rs evaluate_gate_constraints at one point: out[k] = sum over the gates of filter * sum_i alphas[k]^i c_i.
// A forward-emitting gate takes its constraints with a running power of alpha, any other by a Horner step; the filter is the
// selector product of gates/selectors.rs, with the UNUSED_SELECTOR factor once there is more than one selector column.
// The algebra additionally supplies V selector(i), constants column i.
constexpr uint32_t MAX_REGS = 64, MAX_CHALLENGES = 4, UNUSED_SELECTOR = 0xFFFFFFFFu;
template <class Alg, class Word>
void eval_gates_filtered(Alg &A, const lcp2_gate *gates, size_t num_gates, const uint32_t *code, const Word *imm, uint32_t num_selectors,
                         const typename Alg::S *alphas, uint32_t num_challenges, typename Alg::V *out) {
  using V = typename Alg::V;
  const uint32_t CH = num_challenges;
  V regs[MAX_REGS];
  for (V &r : regs) r = A.imm(0);
  for (uint32_t k = 0; k < CH; k++) out[k] = A.imm(0);
  for (size_t g = 0; g < num_gates; g++) {
    const lcp2_gate &G = gates[g];
    const bool fwd = (G.flags & LCP2_GATE_EMIT_FORWARD) != 0;
    V acc[MAX_CHALLENGES];
    typename Alg::S apow[MAX_CHALLENGES];
    for (uint32_t k = 0; k < CH; k++) { acc[k] = A.imm(0); apow[k] = A.scalar(1); }
    walk_program(A, code, G.code_offset, G.code_len, imm, regs, [&](const V &a) {
      for (uint32_t k = 0; k < CH; k++) {
        if (fwd) { acc[k] = A.scale_add(a, apow[k], acc[k]); apow[k] = A.scalar_mul(apow[k], alphas[k]); }
        else acc[k] = A.scale_add(acc[k], alphas[k], a);
      }
    });
    const V s = A.selector(G.selector_index);
    V f = A.imm(1);
    for (uint32_t j = G.group_start; j < G.group_end; j++)
      if (j != G.selector_value) f = A.mul(f, A.sub(A.imm(j), s));
    if (num_selectors > 1) f = A.mul(f, A.sub(A.imm(UNUSED_SELECTOR), s));
    for (uint32_t k = 0; k < CH; k++) out[k] = A.mul_add(f, acc[k], out[k]);
  }
}

// Degree bound of a program's constraints in the column polynomials (each of degree < n): the program walked over degree bounds,
// where a sum has the larger degree of its terms and a product the sum of its factors', saturating at DEGREE_CAP.
constexpr uint32_t DEGREE_CAP = 1u << 20;
struct DegreeAlg {
  using V = uint32_t; using S = uint32_t;
  static V hi(V a, V b) { return a > b ? a : b; }
  V wire(uint32_t) { return 1; }    V gate_const(uint32_t) { return 1; }    V imm(uint64_t) { return 0; }    V pi(uint32_t) { return 0; }    S scalar(uint64_t) { return 0; }
  V add(V a, V b) { return hi(a, b); }    V sub(V a, V b) { return hi(a, b); }    V mul(V a, V b) { return a + b < DEGREE_CAP ? a + b : DEGREE_CAP; }
  V mul_add(V a, V b, V acc) { return hi(acc, mul(a, b)); }
  V scale_add(V x, S, V acc) { return hi(x, acc); }
};
inline uint32_t program_degree(const uint32_t *code, size_t first, size_t len, size_t nregs) {
  uint32_t reg[MAX_REGS + MDS_WIDTH] = {0};
  (void)nregs;  // validated against MAX_REGS by every caller
  DegreeAlg A;
  uint32_t deg = 0;
  walk_program(A, code, first, len, (const uint64_t *)nullptr, reg, [&](uint32_t d) { deg = d > deg ? d : deg; });
  return deg;
}

}  // namespace gate_program
