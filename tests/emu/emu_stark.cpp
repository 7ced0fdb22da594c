// TEST HARNESS (not product code): csrc/stark.hpp compiled for the CPU - the per-point text of k_stark_quotient and k_stark_check as
// loops over the points and the rows (registers in a plain array where the kernels keep them in LDS), the next-leaf index, the
// word count and the verifier of lcp2_stark_verify.  Built by tests/test_stark_emu.py with g++ and included by
// tests/emu/sanitize_stark_main.cpp; never loaded by the package.
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/stark.hpp"

using namespace lcp2;

extern "C" {

unsigned long long emu_stark_words(const lcp2_stark_desc *d) {
  u32 point_polys[FO_MAX_POINTS] = {0};
  std::string why;
  if (st_desc_problem(d, point_polys, why)) return 0;
  return st_make_layout(*d, point_polys).total;
}

unsigned long long emu_stark_next_leaf(unsigned long long i, unsigned lgN, unsigned rate_bits) { return st_next_leaf(i, lgN, rate_bits); }

// the quotient values of every point of the coset: lde = the trace LDE [width][n << rate_bits] in leaf order, out = [num_challenges][n << q];
// returns 0, or 1 for a refused description
int emu_stark_quotient(const lcp2_stark_desc *d, const unsigned long long *public_inputs, const unsigned long long *lde, const unsigned long long *alphas,
                       unsigned long long *out) {
  u32 point_polys[FO_MAX_POINTS] = {0};
  std::string why;
  if (st_desc_problem(d, point_polys, why)) return 1;
  const StStaged S = st_stage(*d, public_inputs);
  const StPrograms P = S.view(*d);
  StCoset C = st_make_coset(d->log_n, d->quotient_degree_bits);
  std::vector<u64> lo(1ull << C.lo_bits), hi(1ull << (C.lgM - C.lo_bits));
  for (u64 j = 0; j < lo.size(); j++) lo[j] = st_coset_lo(C.lgM, j);
  for (u64 j = 0; j < hi.size(); j++) hi[j] = st_coset_hi(C.lgM, j);
  C.x_lo = lo.data(); C.x_hi = hi.data();
  u64 regs[ST_MAX_REGS + 1];
  const u32 lgN = d->log_n + d->fri.rate_bits;
  for (u64 i = 0; i < (1ull << C.lgM); i++) st_quotient_point(P, C, lde, 1ull << lgN, lgN, d->fri.rate_bits, alphas, i, regs, out);
  return 0;
}

// the witness check over all rows, the minimum taken as atomicMin takes it: 0 satisfied (v untouched), 1 violated, 2 refused description
int emu_stark_check(const lcp2_stark_desc *d, const unsigned long long *public_inputs, const unsigned long long *trace, lcp2_stark_violation *v) {
  u32 point_polys[FO_MAX_POINTS] = {0};
  std::string why;
  if (st_desc_problem(d, point_polys, why)) return 2;
  const StStaged S = st_stage(*d, public_inputs);
  const StPrograms P = S.view(*d);
  u64 regs[ST_MAX_REGS + 1], flag = ROW_NO_PROBLEM;
  const u64 n = 1ull << d->log_n;
  for (u64 row = n; row-- > 0;) {  // (any order gives the same minimum)
    const u64 key = st_check_row(P, trace, n, row, regs);
    if (key < flag) flag = key;
  }
  if (flag == ROW_NO_PROBLEM) return 0;
  *v = st_violation_of(P, flag);
  return 1;
}

int emu_stark_verify(const lcp2_stark_desc *d, const unsigned long long *public_inputs, lcp2_challenger *ch, const unsigned long long *proof,
                     unsigned long long proof_words, int *failed_check) {
  std::string why;
  return st_verify(d, public_inputs, ch, proof, (size_t)proof_words, failed_check, why);
}

}  // extern "C"
