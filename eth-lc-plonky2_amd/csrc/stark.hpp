// AIR proofs over the bare-oracle openings (lcp2_stark_prove / lcp2_stark_verify, include/lcp2.h) as portable text: the refusals and
// the layout both sides derive their offsets from, the per-point text of the two kernels of stark.hip - operand fetch from a row and
// its successor, the three filters, the Horner combination (k_stark_quotient) and the per-row verdict (k_stark_check) - and the
// host verifier.  tests/emu/emu_stark.cpp compiles all of it for the CPU.
//
// The constraints of first_row, transition and last_row form one list c_0 .. c_{m-1}; per challenge alpha the vanishing polynomial is
// the Horner pass acc <- acc alpha + f(c_i) c_i with f = L_first, (X - g^-1), L_last, and the quotient is acc / Z_H.  On the coset
// the division is folded into the filters: L_first / Z_H = 1 / (n (x - 1)), L_last / Z_H = g^-1 / (n (x - g^-1)) and
// (x - g^-1) / Z_H, where Z_H takes 2^q values on 7 H_{2^q n} (a table) and the two denominators share one inversion per point.
//
// Permutation arguments (lcp2_stark_prove_perm / lcp2_stark_verify_perm): the staged table of instances, the per-row ratio text of
// k_stark_perm_ratio (four rows of a lane share one inversion), the closing check, and the constraints Z_z - 1 (first row) and
// Z_z(next) prod rhs - Z_z(local) prod lhs (all rows: on the coset its filter is the factor 1 / Z_H of the table zh_inv, in the
// verifier no factor) that continue the Horner pass of the quotient text and of the identity.  tests/emu/emu_stark_perm.cpp.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "fri_openings.hpp"
#include "gate_program.hpp"
#include "row_flag.hpp"

namespace lcp2 {

constexpr u32 ST_CHECK_CAP = 8, ST_CHECK_IDENTITY = 9;
constexpr u32 ST_MAX_WIDTH = 32767, ST_MAX_CH = 4, ST_MAX_REGS = gate_program::MAX_REGS, ST_MAX_Q = 256;  // Q = 2^q, q <= rate_bits <= 8
constexpr u32 ST_FIRST = 0, ST_TRANSITION = 1, ST_LAST = 2, ST_PERM = 3;  // kinds of a violation
constexpr u32 ST_PERM_MAX_PAIRS = 64, ST_PERM_MAX_COLUMN_PAIRS = 4096, ST_PERM_MAX_Z = 64, ST_PERM_ROWS = 4;

// the program tables are read through the constant address space in device code (scalar loads, as K6 reads them)
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> using st_konst = const T __attribute__((address_space(4))) *;
#define ST_KONST(T, p) ((st_konst<T>)(unsigned long long)(p))
#else
template <class T> using st_konst = const T *;
#define ST_KONST(T, p) (p)
#endif

// ---- the description: refusals shared by the word count, the prover and the verifier (host)
inline const lcp2_stark_program &st_program(const lcp2_stark_desc &d, u32 kind) { return kind == ST_FIRST ? d.first_row : kind == ST_TRANSITION ? d.transition : d.last_row; }

// the instance the opening layer is handed: oracle 0 the trace, oracle 1 the quotient chunks; zeta: both, g zeta: the trace.  With
// numZ permutation columns they are oracle 1 and the quotient is oracle 2; zeta: all three, g zeta: the trace and the Z columns
struct StInstance {
  lcp2_fri_range at_zeta[3], at_next[2];
  u32 cols[3], num_oracles;
  lcp2_fri_instance inst;
  StInstance(const StInstance &) = delete;  // inst points into this object
  explicit StInstance(const lcp2_stark_desc &d, u32 numZ = 0) {
    const u32 quot = d.num_challenges << d.quotient_degree_bits, hasZ = numZ ? 1 : 0;
    num_oracles = 2 + hasZ;
    cols[0] = d.width; cols[1] = numZ; cols[1 + hasZ] = quot;
    at_zeta[0] = {0, 0, d.width}; at_zeta[1] = {1, 0, numZ}; at_zeta[1 + hasZ] = {1 + hasZ, 0, quot};
    at_next[0] = {0, 0, d.width}; at_next[1] = {1, 0, numZ};
    inst = {};
    inst.num_oracles = num_oracles; inst.num_points = 2;
    inst.num_ranges[0] = 2 + hasZ; inst.ranges[0] = at_zeta;
    inst.num_ranges[1] = 1 + hasZ; inst.ranges[1] = at_next;
  }
};
inline bool st_perm_on(const lcp2_stark_perm *perm) { return perm && perm->num_pairs; }
// true (why says why) for a permutation description no call takes, of a description that has passed the checks of st_desc_problem
// up to the instance; *numZ receives the number of Z columns
inline bool st_perm_problem(const lcp2_stark_desc &d, const lcp2_stark_perm &perm, u32 *numZ, std::string &why) {
  if (perm.num_pairs > ST_PERM_MAX_PAIRS) { why = "perm: num_pairs above 64"; return true; }
  if (perm.num_column_pairs > ST_PERM_MAX_COLUMN_PAIRS) { why = "perm: num_column_pairs above 4096"; return true; }
  if (!perm.pairs || !perm.columns) { why = "perm: null pairs or columns"; return true; }
  for (u32 p = 0; p < perm.num_pairs; p++) {
    if (perm.pairs[p].count == 0) { why = "perm: pair " + std::to_string(p) + " has no columns"; return true; }
    if ((u64)perm.pairs[p].first + perm.pairs[p].count > perm.num_column_pairs) { why = "perm: pair " + std::to_string(p) + " lies outside columns"; return true; }
  }
  for (size_t j = 0; j < 2 * perm.num_column_pairs; j++)
    if (perm.columns[j] >= d.width) { why = "perm: column pair " + std::to_string(j / 2) + ": column not below width"; return true; }
  if (perm.batch_size < 1 || perm.batch_size > (1u << d.quotient_degree_bits)) { why = "perm: batch_size outside [1, 2^quotient_degree_bits]"; return true; }
  const u32 z = (perm.num_pairs * d.num_challenges + perm.batch_size - 1) / perm.batch_size;
  if (z > ST_PERM_MAX_Z) { why = "perm: more than 64 Z columns"; return true; }
  *numZ = z;
  return false;
}

// true (why says why) for a description no call takes; point_polys[FO_MAX_POINTS] receives the batch sizes of the instance.  With a
// permutation (st_perm_on) its refusals come behind the description's and before the opening layer's; *numZ is 0 without one
inline bool st_desc_problem(const lcp2_stark_desc *d, u32 *point_polys, std::string &why, const lcp2_stark_perm *perm = nullptr, u32 *numZ = nullptr) {
  namespace gp = gate_program;
  if (!d) { why = "null description"; return true; }
  if (d->width < 1 || d->width > ST_MAX_WIDTH) { why = "width outside [1, 32767]"; return true; }
  if (d->num_challenges < 1 || d->num_challenges > ST_MAX_CH) { why = "num_challenges outside [1, 4]"; return true; }
  if (const char *w = fo_config_problem(d->fri, d->log_n)) { why = w; return true; }
  if (d->quotient_degree_bits > d->fri.rate_bits) { why = "quotient_degree_bits exceeds rate_bits"; return true; }
  if (d->num_regs > ST_MAX_REGS) { why = "num_regs above 64"; return true; }
  if ((d->code_words & 1) || (d->code_words && !d->code) || (d->num_imm && !d->imm)) { why = "bad code or immediate table"; return true; }
  const gp::Limits lim{d->num_regs, 2 * (size_t)d->width, 0, d->num_imm, d->num_public_inputs};
  const u32 Q = 1u << d->quotient_degree_bits;
  static const char *const names[3] = {"first_row", "transition", "last_row"};
  for (u32 kind = 0; kind < 3; kind++) {
    const lcp2_stark_program &p = st_program(*d, kind);
    if ((u64)p.code_offset + p.code_len > d->code_words / 2) { why = std::string(names[kind]) + ": program outside the code"; return true; }
    u32 emits = 0;
    for (u32 pc = p.code_offset; pc < p.code_offset + p.code_len; pc++) {
      const gp::Insn in(d->code[2 * pc], d->code[2 * pc + 1]);
      if (const char *w = gp::insn_problem(in, lim)) { why = std::string(names[kind]) + ": instruction " + std::to_string(pc - p.code_offset) + ": " + w; return true; }
      emits += in.emits();
    }
    if (emits != p.num_constraints) { why = std::string(names[kind]) + ": num_constraints does not match the program"; return true; }
    // deg (n - 1) + deg(filter) - n < Q n:  the transition filter has degree 1, a boundary filter n - 1
    if (p.code_len && gp::program_degree(d->code, p.code_offset, p.code_len, d->num_regs) > Q) {
      why = std::string(names[kind]) + ": constraint degree above 2^quotient_degree_bits"; return true;
    }
  }
  u32 z = 0;
  if (st_perm_on(perm) && st_perm_problem(*d, *perm, &z, why)) return true;
  if (numZ) *numZ = z;
  const StInstance I(*d, z);
  return fo_shape_problem(&d->fri, d->log_n, I.cols, &I.inst, point_polys, why);
}

// ---- the layout: trace cap, (Z cap,) quotient cap, then the words of lcp2_fri_openings_words for the instance
struct StLayout {
  u64 total;
  u32 capw, trace_cap, z_cap, quot_cap, openings;   // word offsets (z_cap only with numZ != 0)
  u32 op_local, op_z, op_quotient, op_next, op_z_next;  // inside the proof: the openings at zeta (trace, Z, chunks) and at g zeta (trace, Z)
  u32 Q, quot_cols, numZ, num_oracles;
  FoLayout fo;
};
inline StLayout st_make_layout(const lcp2_stark_desc &d, const u32 *point_polys, u32 numZ = 0) {
  StLayout L = {};
  const StInstance I(d, numZ);
  L.numZ = numZ; L.num_oracles = I.num_oracles;
  L.fo = fo_make_layout(d.fri, d.log_n, I.cols, I.num_oracles, point_polys, 2);
  L.capw = L.fo.capw; L.trace_cap = 0; L.z_cap = L.capw; L.quot_cap = (I.num_oracles - 1) * L.capw; L.openings = I.num_oracles * L.capw;
  L.Q = 1u << d.quotient_degree_bits; L.quot_cols = I.cols[I.num_oracles - 1];
  L.op_local = L.openings + L.fo.point_off[0]; L.op_z = L.op_local + 2 * d.width; L.op_quotient = L.op_z + 2 * numZ;
  L.op_next = L.openings + L.fo.point_off[1]; L.op_z_next = L.op_next + 2 * d.width;
  L.total = L.openings + L.fo.total;
  return L;
}

// ---- the staged permutation: what the ratio text and the quotient text read, through the constant address space like the
// programs.  Instance t = pair * num_challenges + challenge holds three words at tab[3 t]: beta, gamma, first | count << 32 of its run
// of column pairs; column pair j is the word tab[cols_off + j] = lhs | rhs << 32.  Z number z multiplies the instances
// [z batch, min((z + 1) batch, num_inst)).
struct StPerm {
  const u64 *tab;
  u32 num_inst, numZ, batch, cols_off;
};
inline u32 st_perm_draws(const lcp2_stark_desc &d, const lcp2_stark_perm &perm) { return 2 * perm.batch_size * d.num_challenges; }
// draws[2 (i CH + c)], draws[2 (i CH + c) + 1]: beta and gamma of pair c of challenge set i, in the order they were drawn
inline std::vector<u64> st_perm_stage(const lcp2_stark_desc &d, const lcp2_stark_perm &perm, const u64 *draws, StPerm *view) {
  const u32 CH = d.num_challenges, num_inst = perm.num_pairs * CH;
  std::vector<u64> tab(3 * (size_t)num_inst + perm.num_column_pairs + 1, 0);
  for (u32 t = 0; t < num_inst; t++) {
    const u32 p = t / CH, c = t % CH, i = t % perm.batch_size;
    tab[3 * t] = draws[2 * (i * CH + c)]; tab[3 * t + 1] = draws[2 * (i * CH + c) + 1];
    tab[3 * t + 2] = perm.pairs[p].first | (u64)perm.pairs[p].count << 32;
  }
  for (size_t j = 0; j < perm.num_column_pairs; j++) tab[3 * (size_t)num_inst + j] = perm.columns[2 * j] | (u64)perm.columns[2 * j + 1] << 32;
  view->tab = tab.data(); view->num_inst = num_inst; view->batch = perm.batch_size; view->cols_off = 3 * num_inst;
  view->numZ = (num_inst + perm.batch_size - 1) / perm.batch_size;
  return tab;
}
// prod_i lhs_i and prod_i rhs_i over the instances of Z number z; cell(column): the canonical value of that trace column on the row
template <class Cell>
LCP2_HD void st_perm_products(const StPerm &Pm, u32 z, Cell cell, u64 &num, u64 &den) {
  st_konst<u64> tab = ST_KONST(u64, Pm.tab);
  num = 1; den = 1;
  const u32 t0 = z * Pm.batch, t1 = t0 + Pm.batch < Pm.num_inst ? t0 + Pm.batch : Pm.num_inst;
  for (u32 t = t0; t < t1; t++) {
    const u64 beta = tab[3 * t], gamma = tab[3 * t + 1], run = tab[3 * t + 2];
    const u32 first = (u32)run, count = (u32)(run >> 32);
    u64 lhs = 0, rhs = 0;
    for (u32 j = count; j-- > 0;) {  // Horner from the highest power of beta down
      const u64 lr = tab[Pm.cols_off + first + j];
      lhs = gl_add(gl_mul(lhs, beta), cell((u32)lr));
      rhs = gl_add(gl_mul(rhs, beta), cell((u32)(lr >> 32)));
    }
    num = gl_mul(num, gl_add(lhs, gamma));
    den = gl_mul(den, gl_add(rhs, gamma));
  }
}
// ratio[z n + row] = prod lhs / prod rhs for the rows row0 + k step, k < ST_PERM_ROWS (those below n), of the trace as given
// ([width][n], any u64): Montgomery's trick, one inversion for the four denominators.  A zero denominator gives the ratio 0 (the
// inverse of 0 is 0) and stands in the shared product as 1.
LCP2_HD void st_perm_ratio_rows(const StPerm &Pm, const u64 *trace, u64 n, u64 row0, u64 step, u32 z, u64 *ratio) {
  u64 num[ST_PERM_ROWS], den[ST_PERM_ROWS], pre[ST_PERM_ROWS];
  u64 run = 1;
#pragma unroll
  for (u32 k = 0; k < ST_PERM_ROWS; k++) {
    const u64 row = row0 + k * step;
    num[k] = 0; den[k] = 0;
    if (row < n) st_perm_products(Pm, z, [&](u32 col) { return gl_canon(trace[(u64)col * n + row]); }, num[k], den[k]);
    pre[k] = run;
    run = gl_mul(run, den[k] ? den[k] : 1);
  }
  u64 inv = gl_inv(run);
#pragma unroll
  for (u32 k = ST_PERM_ROWS; k-- > 0;) {
    const u64 row = row0 + k * step;
    if (row < n) ratio[(u64)z * n + row] = den[k] ? gl_mul(num[k], gl_mul(inv, pre[k])) : 0;
    inv = gl_mul(inv, den[k] ? den[k] : 1);
  }
}
// the running product closes: Z_z[n - 1] ratio_z[n - 1] == 1 (zs the exclusive prefix products of the ratios, both [numZ][n])
LCP2_HD bool st_perm_closes(const u64 *zs, const u64 *ratio, u64 n, u32 z) { return gl_canon(gl_mul(zs[(u64)z * n + n - 1], ratio[(u64)z * n + n - 1])) == 1; }

// ---- the staged programs: what the per-point text reads.  One instruction per 64-bit word (w0 | w1 << 32), padded by one so that
// the walk may fetch one instruction ahead; immediates and public inputs canonical.
struct StPrograms {
  const u64 *code, *imm, *pis;
  u32 first[3], len[3], ncons[3];
  u32 width, num_regs, num_challenges;
};
struct StStaged {
  std::vector<u64> code, imm, pis;  // imm and pis never empty
  StPrograms view(const lcp2_stark_desc &d) const {
    StPrograms P = {};
    P.code = code.data(); P.imm = imm.data(); P.pis = pis.data();
    for (u32 k = 0; k < 3; k++) { P.first[k] = st_program(d, k).code_offset; P.len[k] = st_program(d, k).code_len; P.ncons[k] = st_program(d, k).num_constraints; }
    P.width = d.width; P.num_regs = d.num_regs; P.num_challenges = d.num_challenges;
    return P;
  }
};
inline StStaged st_stage(const lcp2_stark_desc &d, const u64 *public_inputs) {
  StStaged S;
  S.code.assign(d.code_words / 2 + 1, 0);
  for (size_t pc = 0; pc < d.code_words / 2; pc++) S.code[pc] = d.code[2 * pc] | (u64)d.code[2 * pc + 1] << 32;
  S.imm.assign(d.num_imm + 1, 0);
  for (size_t i = 0; i < d.num_imm; i++) S.imm[i] = d.imm[i] % GL_P;
  S.pis.assign(d.num_public_inputs + 1, 0);
  for (u32 i = 0; i < d.num_public_inputs; i++) S.pis[i] = public_inputs[i] % GL_P;
  return S;
}

// ---- the per-point text
// the leaf that holds the successor of leaf i's row: x -> g x on the LDE coset of 2^lgN leaves (leaf order is bit-reversed)
LCP2_HD u64 st_next_leaf(u64 i, u32 lgN, u32 rate_bits) {
  return bitrev32((bitrev32((u32)i, lgN) + (1u << rate_bits)) & ((1u << lgN) - 1), lgN);
}

// One program over the base field.  column(idx): operand WIRE idx (idx < width: the local row, else the next row), canonical;
// regs: num_regs registers (operator[] gives a u64 &), cleared here; emit(value) receives the constraints in program order.
template <class Column, class Regs, class Emit>
LCP2_HD void st_walk(const StPrograms &P, u32 kind, Column column, Regs regs, Emit emit) {
  namespace gp = gate_program;
  st_konst<u64> code = ST_KONST(u64, P.code), imm = ST_KONST(u64, P.imm), pis = ST_KONST(u64, P.pis);
  for (u32 r = 0; r < P.num_regs; r++) regs[r] = 0;
  const u32 first = P.first[kind], end = first + P.len[kind];
  u64 nxt = code[first];
  for (u32 pc = first; pc < end; pc++) {
    const u32 w0 = (u32)nxt, w1 = (u32)(nxt >> 32);
    nxt = code[pc + 1];  // wave-uniform: the scalar load overlaps the arithmetic of this instruction
    const u32 op = w0 & 0xF, dst = (w0 >> 8) & 0xFF, ka = (w0 >> 16) & 0xF, kb = (w0 >> 20) & 0xF, ia = w1 & 0xFFFF, ib = w1 >> 16;
    auto operand = [&](u32 k, u32 i) -> u64 { return k == gp::KIND_REG ? regs[i] : k == gp::KIND_WIRE ? column(i) : k == gp::KIND_IMM ? imm[i] : pis[i]; };
    if (op == LCP2_OP_PMDS) {  // 32-bit halves times the small constants, one reduction per element
      u64 x[gp::MDS_WIDTH];
      GP_UNROLL
      for (u32 j = 0; j < gp::MDS_WIDTH; j++) x[j] = regs[ia + j];
      GP_UNROLL
      for (u32 r = 0; r < gp::MDS_WIDTH; r++) {
        u64 lo = (x[r] & GL_EPS) * gp::MDS_DIAG[r], hi = (x[r] >> 32) * gp::MDS_DIAG[r];
        GP_UNROLL
        for (u32 j = 0; j < gp::MDS_WIDTH; j++) { const u64 v = x[(j + r) % gp::MDS_WIDTH]; lo += (v & GL_EPS) * gp::MDS_CIRC[j]; hi += (v >> 32) * gp::MDS_CIRC[j]; }
        const u64 l = lo + (hi << 32);
        regs[dst + r] = gl_add(gl_reduce128(l, (hi >> 32) + (l < lo ? 1 : 0)), imm[ib + r]);
      }
      continue;
    }
    const u64 a = operand(ka, ia);
    if (op == LCP2_OP_EMIT) { emit(a); continue; }
    if (op == LCP2_OP_EMITBOOL) { emit(gl_sub(gl_mul(a, a), a)); continue; }
    if (op == LCP2_OP_SBOX) { const u64 a2 = gl_mul(a, a), a4 = gl_mul(a2, a2); regs[dst] = gl_mul(gl_mul(a2, a), a4); continue; }
    const u64 b = operand(kb, ib);
    u64 r;
    switch (op) {
      case LCP2_OP_ADD: r = gl_add(a, b); break;
      case LCP2_OP_SUB: r = gl_sub(a, b); break;
      case LCP2_OP_MUL: r = gl_mul(a, b); break;
      case LCP2_OP_XOR: { const u64 ab = gl_mul(a, b); r = gl_sub(gl_sub(gl_add(a, b), ab), ab); break; }
      case LCP2_OP_DBLADD: r = gl_add(gl_add(a, a), b); break;
      default: r = gl_add(regs[dst], gl_mul(a, b)); break;  // LCP2_OP_MULADD
    }
    regs[dst] = r;
  }
}

// the quotient coset 7 H_M, M = 2^(log_n + q), in leaf order: x_i = 7 w_M^bitrev(i) from a two-level table of the powers of w_M
struct StCoset {
  const u64 *x_lo, *x_hi;   // 7 w^j (j < 2^lo_bits); w^(j << lo_bits)
  u32 log_n, lgM, lo_bits;
  u64 n_inv, g_inv;
  u64 zh_inv[ST_MAX_Q];     // 1 / Z_H(x_i), by i >> log_n
};
LCP2_HD u32 st_lo_bits(u32 lgM) { return (lgM + 1) / 2; }
inline u64 st_coset_lo(u32 lgM, u64 j) { return gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(lgM), j)); }
inline u64 st_coset_hi(u32 lgM, u64 j) { return gl_pow(gl_root_of_unity(lgM), j << st_lo_bits(lgM)); }
// everything of the coset but its two tables (host)
inline StCoset st_make_coset(u32 log_n, u32 q) {
  StCoset C = {};
  C.log_n = log_n; C.lgM = log_n + q; C.lo_bits = st_lo_bits(C.lgM);
  C.n_inv = gl_inv((1ull << log_n) % GL_P);
  C.g_inv = gl_inv(gl_root_of_unity(log_n));
  const u64 shift_n = gl_pow(GL_GENERATOR, 1ull << log_n);  // x^n = 7^n w_Q^bitrev_q(i >> log_n)
  for (u32 t = 0; t < (1u << q); t++) C.zh_inv[t] = gl_inv(gl_sub(gl_mul(shift_n, gl_pow(gl_root_of_unity(q), bitrev32(t, q))), 1));
  return C;
}
// f[kind] = filter_kind(x_i) / Z_H(x_i)
LCP2_HD void st_filters(const StCoset &C, u64 i, u64 f[3]) {
  const u32 e = bitrev32((u32)i, C.lgM);
  const u64 x = gl_mul(C.x_lo[e & ((1u << C.lo_bits) - 1)], C.x_hi[e >> C.lo_bits]);
  const u64 d_first = gl_sub(x, 1), d_last = gl_sub(x, C.g_inv);  // never 0: the coset does not meet H
  const u64 inv = gl_inv(gl_mul(d_first, d_last));
  f[ST_FIRST] = gl_mul(C.n_inv, gl_mul(inv, d_last));
  f[ST_TRANSITION] = gl_mul(d_last, C.zh_inv[i >> C.log_n]);
  f[ST_LAST] = gl_mul(gl_mul(C.n_inv, C.g_inv), gl_mul(inv, d_first));
}
// acc[c] <- the Horner pass over the whole list with the filters f, per challenge
template <class Column, class Regs>
LCP2_HD void st_combine(const StPrograms &P, const u64 f[3], const u64 *alphas, Column column, Regs regs, u64 acc[ST_MAX_CH]) {
#pragma unroll
  for (u32 c = 0; c < ST_MAX_CH; c++) acc[c] = 0;
  for (u32 kind = 0; kind < 3; kind++)
    st_walk(P, kind, column, regs, [&](u64 v) {
      const u64 fv = gl_mul(f[kind], v);
#pragma unroll
      for (u32 c = 0; c < ST_MAX_CH; c++)
        if (c < P.num_challenges) acc[c] = gl_add(gl_mul(acc[c], alphas[c]), fv);
    });
}
// the permutation constraints continue the pass: Z_z - 1 under the first-row filter for every z, then the all-rows constraint of
// every z under f_all.  local(column): the trace on the row; z_local(z), z_next(z): Z_z on the row and on its successor
template <class Local, class ZLocal, class ZNext>
LCP2_HD void st_perm_combine(const StPerm &Pm, u32 num_challenges, u64 f_first, u64 f_all, const u64 *alphas, Local local, ZLocal z_local, ZNext z_next,
                             u64 acc[ST_MAX_CH]) {
  auto push = [&](u64 fv) {
#pragma unroll
    for (u32 c = 0; c < ST_MAX_CH; c++)
      if (c < num_challenges) acc[c] = gl_add(gl_mul(acc[c], alphas[c]), fv);
  };
  for (u32 z = 0; z < Pm.numZ; z++) push(gl_mul(f_first, gl_sub(z_local(z), 1)));
  for (u32 z = 0; z < Pm.numZ; z++) {
    u64 num, den;
    st_perm_products(Pm, z, local, num, den);
    push(gl_mul(f_all, gl_sub(gl_mul(z_next(z), den), gl_mul(z_local(z), num))));
  }
}
// the quotient values of point i (leaf i of the trace LDE [width][stride]) into out[c * M + i]; PERM: with the permutation
// constraints of Pm over the LDE z_lde [numZ][stride] of the Z columns
template <bool PERM = false, class Regs>
LCP2_HD void st_quotient_point(const StPrograms &P, const StCoset &C, const u64 *lde, u64 stride, u32 lgN, u32 rate_bits, const u64 *alphas, u64 i, Regs regs,
                               u64 *out, const StPerm *Pm = nullptr, const u64 *z_lde = nullptr) {
  u64 f[3], acc[ST_MAX_CH];
  st_filters(C, i, f);
  const u64 next = st_next_leaf(i, lgN, rate_bits);
  const u32 width = P.width;
  st_combine(P, f, alphas, [&](u32 idx) { return idx < width ? lde[(u64)idx * stride + i] : lde[(u64)(idx - width) * stride + next]; }, regs, acc);
  if constexpr (PERM)
    st_perm_combine(*Pm, P.num_challenges, f[ST_FIRST], C.zh_inv[i >> C.log_n], alphas, [&](u32 col) { return lde[(u64)col * stride + i]; },
                    [&](u32 z) { return z_lde[(u64)z * stride + i]; }, [&](u32 z) { return z_lde[(u64)z * stride + next]; }, acc);
#pragma unroll
  for (u32 c = 0; c < ST_MAX_CH; c++)
    if (c < P.num_challenges) out[((u64)c << C.lgM) + i] = acc[c];
}

// the witness check of row `row` of the trace as given ([width][n], any u64): ROW_NO_PROBLEM, or st_violation_key of the first
// violated constraint of the list.  First-row constraints hold on row 0, last-row constraints on row n - 1, transition constraints
// on every row but the last; the next row of row i is row (i + 1) mod n.
LCP2_HD u64 st_violation_key(u64 row, u32 list_index) { return row << 32 | list_index; }
template <class Regs>
LCP2_HD u64 st_check_row(const StPrograms &P, const u64 *trace, u64 n, u64 row, Regs regs) {
  u64 key = ROW_NO_PROBLEM;
  u32 index = 0;
  const u64 next = row + 1 == n ? 0 : row + 1;
  const u32 width = P.width;
  for (u32 kind = 0; kind < 3; kind++) {
    const bool active = kind == ST_FIRST ? row == 0 : kind == ST_TRANSITION ? row + 1 != n : row + 1 == n;
    if (active)
      st_walk(P, kind, [&](u32 idx) { return gl_canon(idx < width ? trace[(u64)idx * n + row] : trace[(u64)(idx - width) * n + next]); }, regs, [&](u64 v) {
        if (v != 0 && key == ROW_NO_PROBLEM) key = st_violation_key(row, index);
        index++;
      });
    else index += P.ncons[kind];
  }
  return key;
}
inline lcp2_stark_violation st_violation_of(const StPrograms &P, u64 key) {
  u32 index = (u32)key, kind = 0;
  while (kind < 2 && index >= P.ncons[kind]) index -= P.ncons[kind++];
  return lcp2_stark_violation{kind, index, key >> 32};
}

// ---- the verifier (host).  The programs over F_p^2 at the openings, through the walker every host reader of a program uses
struct StZetaAlg {
  using V = gl2; using S = u64;
  const u64 *local, *next, *pis; u32 width;
  V wire(u32 i) { return i < width ? vq_rd2(local + 2 * i) : vq_rd2(next + 2 * (i - width)); }
  V gate_const(u32) { return gl2_make(0, 0); }  // refused by st_desc_problem
  V imm(u64 x) { return gl2_make(x % GL_P, 0); }
  V pi(u32 i) { return gl2_make(pis[i], 0); }
  S scalar(u64 x) { return x; }
  S scalar_mul(S a, S b) { return gl_mul(a, b); }
  V add(V a, V b) { return gl2_add(a, b); }
  V sub(V a, V b) { return gl2_sub(a, b); }
  V mul(V a, V b) { return gl2_mul(a, b); }
  V mul_add(V a, V b, V acc) { return gl2_add(acc, gl2_mul(a, b)); }
  V scale_add(V x, S s, V acc) { return gl2_add(acc, gl2_scale(x, s)); }
};
// vanishing_c(zeta) == Z_H(zeta) sum_k chunk_{c,k}(zeta) zeta^(n k) for every challenge
// (with Pm: over the list extended by the permutation constraints, the all-rows ones without a filter)
inline bool st_identity_holds(const lcp2_stark_desc &d, const StLayout &L, const u64 *pis, const u64 *alphas, gl2 zeta, const u64 *proof,
                              const StPerm *Pm = nullptr) {
  const u64 n = 1ull << d.log_n;
  const u64 g_inv = gl_inv(gl_root_of_unity(d.log_n)), n_inv = gl_inv(n % GL_P);
  const gl2 zeta_n = gl2_pow(zeta, n), zh = gl2_sub_base(zeta_n, 1);
  const gl2 d_first = gl2_sub_base(zeta, 1), d_last = gl2_sub_base(zeta, g_inv);
  const gl2 f[3] = {gl2_scale(gl2_mul(zh, gl2_inv(d_first)), n_inv), d_last, gl2_scale(gl2_mul(zh, gl2_inv(d_last)), gl_mul(n_inv, g_inv))};
  StZetaAlg A{proof + L.op_local, proof + L.op_next, pis, d.width};
  gl2 acc[ST_MAX_CH] = {};
  for (u32 kind = 0; kind < 3; kind++) {
    gl2 regs[ST_MAX_REGS + gate_program::MDS_WIDTH] = {};
    gate_program::walk_program(A, d.code, st_program(d, kind).code_offset, st_program(d, kind).code_len, d.imm, regs, [&](const gl2 &v) {
      const gl2 fv = gl2_mul(f[kind], v);
      for (u32 c = 0; c < d.num_challenges; c++) acc[c] = gl2_add(gl2_scale(acc[c], alphas[c]), fv);
    });
  }
  if (Pm) {
    auto push = [&](const gl2 &fv) {
      for (u32 c = 0; c < d.num_challenges; c++) acc[c] = gl2_add(gl2_scale(acc[c], alphas[c]), fv);
    };
    for (u32 z = 0; z < Pm->numZ; z++) push(gl2_mul(f[ST_FIRST], gl2_sub_base(vq_rd2(proof + L.op_z + 2 * z), 1)));
    for (u32 z = 0; z < Pm->numZ; z++) {
      gl2 num = gl2_make(1, 0), den = gl2_make(1, 0);
      const u32 t0 = z * Pm->batch, t1 = std::min(t0 + Pm->batch, Pm->num_inst);
      for (u32 t = t0; t < t1; t++) {
        const u64 beta = Pm->tab[3 * t], gamma = Pm->tab[3 * t + 1], run = Pm->tab[3 * t + 2];
        gl2 lhs = gl2_make(0, 0), rhs = gl2_make(0, 0);
        for (u32 j = (u32)(run >> 32); j-- > 0;) {
          const u64 lr = Pm->tab[Pm->cols_off + (u32)run + j];
          lhs = gl2_add(gl2_scale(lhs, beta), A.wire((u32)lr));
          rhs = gl2_add(gl2_scale(rhs, beta), A.wire((u32)(lr >> 32)));
        }
        num = gl2_mul(num, gl2_add(lhs, gl2_make(gamma, 0)));
        den = gl2_mul(den, gl2_add(rhs, gl2_make(gamma, 0)));
      }
      push(gl2_sub(gl2_mul(vq_rd2(proof + L.op_z_next + 2 * z), den), gl2_mul(vq_rd2(proof + L.op_z + 2 * z), num)));
    }
  }
  for (u32 c = 0; c < d.num_challenges; c++) {
    gl2 sum = gl2_make(0, 0);
    for (u32 k = L.Q; k-- > 0;) sum = gl2_add(gl2_mul(sum, zeta_n), vq_rd2(proof + L.op_quotient + 2 * (c * L.Q + k)));
    if (!gl2_eq(acc[c], gl2_mul(zh, sum))) return false;
  }
  return true;
}
// the transcript up to zeta, the prover's and the verifier's alike: public inputs, trace cap, (the permutation's betas and gammas,
// Z cap,) alphas; quotient cap, zeta
inline void st_observe_statement(HostChallenger &ch, const StStaged &S, u32 num_public_inputs, const u64 *trace_cap, u32 capw) {
  ch.observe_n(S.pis.data(), num_public_inputs);
  ch.observe_n(trace_cap, capw);
}
inline std::vector<u64> st_draw_perm(HostChallenger &ch, u32 draws) {
  std::vector<u64> out(draws);
  for (u64 &v : out) v = ch.get();
  return out;
}
inline void st_draw_alphas(HostChallenger &ch, const u64 *z_cap /* null without a permutation */, u32 capw, u32 num_challenges, u64 *alphas) {
  if (z_cap) ch.observe_n(z_cap, capw);
  for (u32 c = 0; c < num_challenges; c++) alphas[c] = ch.get();
}
inline gl2 st_draw_zeta(HostChallenger &ch, const u64 *quot_cap, u32 capw) {
  ch.observe_n(quot_cap, capw);
  return ch.get_ext();
}
// the two points of the instance: zeta and g zeta
inline void st_points(gl2 zeta, u32 log_n, u64 points[4]) {
  const u64 g = gl_root_of_unity(log_n);
  points[0] = zeta.c0; points[1] = zeta.c1; points[2] = gl_mul(zeta.c0, g); points[3] = gl_mul(zeta.c1, g);
}

// lcp2_stark_verify / lcp2_stark_verify_perm without their ABI dress: LCP2_OK / LCP2_E_VERIFY / LCP2_E_INVALID (why says why).  Order
// of the checks: 8, the opening layer's 1 and 2, 9, then the opening layer's queries.
inline int st_verify(const lcp2_stark_desc *d, const u64 *public_inputs, lcp2_challenger *chs, const u64 *proof, size_t proof_words, int32_t *failed_check,
                     std::string &why, const lcp2_stark_perm *perm = nullptr) {
  if (failed_check) *failed_check = 0;
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  if (st_desc_problem(d, point_polys, why, perm, &numZ)) return LCP2_E_INVALID;
  if (!chs || !proof || (d->num_public_inputs && !public_inputs)) { why = "null argument"; return LCP2_E_INVALID; }
  if (chs->input_len >= 8 || chs->output_len > 8) { why = "broken challenger state"; return LCP2_E_INVALID; }
  const StLayout L = st_make_layout(*d, point_polys, numZ);
  if (proof_words != L.total) { why = "proof_words is not lcp2_stark_proof_words"; return LCP2_E_INVALID; }
  for (u32 w = 0; w < L.openings; w++)
    if (proof[w] >= GL_P) { if (failed_check) *failed_check = (int32_t)ST_CHECK_CAP; return LCP2_E_VERIFY; }
  const StStaged S = st_stage(*d, public_inputs);
  HostChallenger ch;
  ch.load((const u64 *)chs->sponge, (const u64 *)chs->input, chs->input_len, (const u64 *)chs->output, chs->output_len);
  u64 alphas[ST_MAX_CH] = {0}, points[4];
  st_observe_statement(ch, S, d->num_public_inputs, proof + L.trace_cap, L.capw);
  StPerm Pm = {};
  std::vector<u64> perm_tab;
  if (numZ) perm_tab = st_perm_stage(*d, *perm, st_draw_perm(ch, st_perm_draws(*d, *perm)).data(), &Pm);
  st_draw_alphas(ch, numZ ? proof + L.z_cap : nullptr, L.capw, d->num_challenges, alphas);
  const gl2 zeta = st_draw_zeta(ch, proof + L.quot_cap, L.capw);
  st_points(zeta, d->log_n, points);
  ch.save((u64 *)chs->sponge, (u64 *)chs->input, chs->input_len, (u64 *)chs->output, chs->output_len);
  const StInstance I(*d, numZ);
  const u64 *caps[3] = {proof + L.trace_cap, proof + (numZ ? L.z_cap : L.quot_cap), proof + L.quot_cap};
  return fo_verify_openings(caps, I.cols, d->log_n, &I.inst, points, &d->fri, chs, proof + L.openings, (size_t)L.fo.total, failed_check, why,
                            [&](const FoLayout &) { return st_identity_holds(*d, L, S.pis.data(), alphas, zeta, proof, numZ ? &Pm : nullptr) ? 0u : ST_CHECK_IDENTITY; });
}

}  // namespace lcp2
