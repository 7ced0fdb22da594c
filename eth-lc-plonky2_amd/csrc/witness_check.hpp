// lcp2_check_witness as portable text: what the kernels of witness_check.hip run per row and per routed cell, what the entry point
// runs on the host for the one cell it names, and what tests/emu/emu_check.cpp runs on the CPU.
//
// Gate constraints.  The check needs every constraint of a row's own gate ON ITS OWN - no alpha, no filter - so it does not go
// through the evaluators of K6 (their result is sum_j alpha^j c_j): wc_walk walks the STAGED program (gate_staging.hpp: LDG,
// STAGE operands, PMDS, ...) instruction by instruction, like q_interpret does, over a memory `Mem` (registers, staging slots,
// columns, immediates: LDS and HBM on the device, arrays on the CPU) and hands each emitted value to a sink.  WcCount is the
// sink of the check: how many values were non-zero, and the smallest plonky2 constraint index among them.
//
// Copy constraints.  sigma_j(w^r) is the ID  k_j' w^r'  of the cell that follows (row r, wire j) in its cycle; wc_decode_cell
// finds (j', r') from the value alone: s^n = k_j'^n names the coset (the k_is lie in distinct cosets of H, so the n-th powers are
// distinct), and r' is the discrete logarithm of s / k_j' in H, bit by bit from the low end (Pohlig-Hellman in a 2-group).
#pragma once
#include "../../include/lcp2.h"
#include "gate_staging.hpp"
#include "gl64.hpp"
#include "ntt.hpp"

namespace lcp2 {

constexpr u32 WC_MAX_GATES = 1u << 16, WC_MAX_CONSTRAINTS = 1u << 16;  // what the packed key of a violation has room for
constexpr u32 WC_MAX_DEGREE_BITS = 28;                                  // lcp2_params_config's bound
constexpr u32 WC_NO_WIRE = 0xFFFFFFFFu;
constexpr u64 WC_NONE = ~0ull;

// ---- the first violation as one word, so that a minimum finds it: (row, gate, constraint) and (row, wire) order
LCP2_HD u64 wc_gate_key(u64 row, u32 gate, u32 constraint) { return row << 32 | (u64)gate << 16 | constraint; }
LCP2_HD u64 wc_copy_key(u64 row, u32 wire) { return row << 32 | wire; }

// ---- the counting sink.  A program without LCP2_GATE_EMIT_FORWARD lists its constraints last to first: plonky2's index of the
// e-th emitted value is then num_constraints - 1 - e.
struct WcCount {
  u32 count, first, emitted, last;
  bool forward;
  LCP2_HD void begin(u32 num_constraints, u32 gate_flags) {
    count = 0; first = WC_MAX_CONSTRAINTS; emitted = 0; last = num_constraints - 1;
    forward = (gate_flags & LCP2_GATE_EMIT_FORWARD) != 0;
  }
  LCP2_HD void operator()(u64 value /* canonical */) {
    const u32 index = forward ? emitted : last - emitted;
    emitted++;
    if (value != 0) { count++; if (index < first) first = index; }
  }
};

// ---- the walk of one staged program.  Mem:
//   u64 insn(pc)                       the two words of instruction pc (the code array is padded: pc + 1 is readable)
//   void stage(count, list_offset)     LDG: the listed columns of this row, canonical, into the staging slots
//   u64 operand(kind, idx)             REG, STAGE, IMM, PI (and WIRE / CONST of an unstaged program), canonical
//   u64 reg(r) / void set_reg(r, v)
//   void pmds(dst, src, imm_offset)    LCP2_OP_PMDS;   u64 sbox(x)   x^7
template <class Mem, class Sink>
LCP2_HD void wc_walk(Mem &m, u32 code_offset, u32 code_len, Sink &sink) {
  u64 nxt = m.insn(code_offset);  // one instruction ahead: the fetch overlaps the arithmetic of the current one
  for (u32 pc = code_offset; pc < code_offset + code_len; pc++) {
    const u32 w0 = (u32)nxt, w1 = (u32)(nxt >> 32);
    nxt = m.insn(pc + 1);
    const u32 op = w0 & 0xF, dst = (w0 >> 8) & 0xFF, ka = (w0 >> 16) & 0xF, kb = (w0 >> 20) & 0xF, ia = w1 & 0xFFFF, ib = w1 >> 16;
    if (op == QOP_LDG) { m.stage(dst, w1); continue; }
    if (op == LCP2_OP_PMDS) { m.pmds(dst, ia, ib); continue; }
    u64 x = m.operand(ka, ia);
    if (op == LCP2_OP_EMIT) { sink(x); continue; }
    if (op == LCP2_OP_EMITBOOL) { sink(gl_sub(gl_mul(x, x), x)); continue; }
    if (op == LCP2_OP_SBOX) { m.set_reg(dst, m.sbox(x)); continue; }
    const u64 y = m.operand(kb, ib);
    u64 r;
    switch (op) {
      case LCP2_OP_ADD: r = gl_add(x, y); break;
      case LCP2_OP_SUB: r = gl_sub(x, y); break;
      case LCP2_OP_MUL: r = gl_mul(x, y); break;
      case LCP2_OP_XOR: { const u64 xy = gl_mul(x, y); r = gl_sub(gl_sub(gl_add(x, y), xy), xy); break; }
      case LCP2_OP_DBLADD: r = gl_add(gl_add(x, x), y); break;
      default: r = gl_add(m.reg(dst), gl_mul(x, y)); break;  // LCP2_OP_MULADD
    }
    m.set_reg(dst, r);
  }
}

// ---- cell-id decoding
struct WcDecode {
  const u64 *kn;     // [num_routed] k_is[j]^n
  const u64 *kinv;   // [num_routed] 1 / k_is[j]
  TwoLevelTable roots;  // w_n^e, e < n (NttHost::root_table(degree_bits, false))
  u32 num_routed, degree_bits;
};
struct WcCell {
  u32 wire;  // WC_NO_WIRE: the value is the id of no cell
  u64 row;
};
// the cell (j', r') with s = k_is[j'] w^r'; s: any u64.  About 2 d squarings, d table values (one multiply each) and num_routed
// compares.  The d powers t^(2^k) of t = s / k_j' stay in registers: P[] is indexed by compile-time constants only (the powers sit
// at its top end, whatever d is), so no array goes to scratch.
LCP2_HD WcCell wc_decode_cell(const WcDecode &t, u64 s) {
  const u32 d = t.degree_bits;
  WcCell out;
  out.wire = WC_NO_WIRE; out.row = 0;
  s = gl_canon(s);
  u64 sn = s;
  for (u32 k = 0; k < d; k++) sn = gl_sqr(sn);
  u32 j = WC_NO_WIRE;
  for (u32 q = 0; q < t.num_routed; q++)
    if (t.kn[q] == sn) { j = q; break; }
  if (j == WC_NO_WIRE) return out;
  u64 P[WC_MAX_DEGREE_BITS];  // P[WC_MAX_DEGREE_BITS - d + k] = t^(2^k), k < d
  u64 cur = gl_mul(s, t.kinv[j]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (u32 m = 0; m < WC_MAX_DEGREE_BITS; m++) {
    P[m] = cur;
    if (m + d >= WC_MAX_DEGREE_BITS) cur = gl_sqr(cur);
  }
  // bit i of r': t^(2^(d-1-i)) = w^((r' mod 2^(i+1)) 2^(d-1-i)) is w^((r' mod 2^i) 2^(d-1-i)) when the bit is 0, minus that when it is 1
  u64 r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (u32 i = 0; i < WC_MAX_DEGREE_BITS; i++) {
    if (i < d) {
      const u64 w = two_level(t.roots, r << (d - 1 - i));
      if (P[WC_MAX_DEGREE_BITS - 1 - i] != w) r |= 1ull << i;
    }
  }
  out.wire = j; out.row = r;
  return out;
}
// host: the two small tables of WcDecode, kn then kinv, 2 * num_routed words
inline void wc_decode_tables(const u64 *k_is, u32 num_routed, u32 degree_bits, u64 *out) {
  for (u32 j = 0; j < num_routed; j++) {
    u64 v = gl_canon(k_is[j]);
    out[num_routed + j] = gl_inv(v);
    for (u32 k = 0; k < degree_bits; k++) v = gl_sqr(v);
    out[j] = v;
  }
}

// ---- one routed cell: is its copy constraint violated?  wires [>= num_routed][n] and sigmas [num_routed][n] column-major, any
// u64; own_id = k_is[wire] w^row.  A cell that is its own sigma image is tied to nothing and skips the decode.
LCP2_HD bool wc_copy_violated(const WcDecode &t, const u64 *wires, const u64 *sigmas, u64 n, u32 wire, u64 row, u64 own_id, WcCell *partner) {
  const u64 s = gl_canon(sigmas[(u64)wire * n + row]);
  if (s == own_id) { if (partner) { partner->wire = wire; partner->row = row; } return false; }
  const WcCell to = wc_decode_cell(t, s);
  if (partner) *partner = to;
  if (to.wire == WC_NO_WIRE) return true;
  return gl_canon(wires[(u64)wire * n + row]) != gl_canon(wires[(u64)to.wire * n + to.row]);
}

}  // namespace lcp2
