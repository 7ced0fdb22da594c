// TEST HARNESS (not product code): the permutation-argument text of csrc/stark.hpp compiled for the CPU - the refusals with their
// reasons, the word count, the per-row ratio text of k_stark_perm_ratio as loops over the lanes (a lane's ST_PERM_ROWS rows `threads`
// apart, as in the kernel), the running product as a plain loop where the device runs launch_scan, the closing verdict, the per-point
// text of the PERM quotient kernel, and the verifier of lcp2_stark_verify_perm.  Built by tests/stark_perm_cases.py with g++ and
// included by tests/emu/sanitize_stark_perm_main.cpp; never loaded by the package.
#include <cstring>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/stark.hpp"

using namespace lcp2;

extern "C" {

unsigned long long emu_stark_perm_words(const lcp2_stark_desc *d, const lcp2_stark_perm *perm) {
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  std::string why;
  if (st_desc_problem(d, point_polys, why, perm, &numZ)) return 0;
  return st_make_layout(*d, point_polys, numZ).total;
}

// 0, or 1 with the reason (cut to len - 1 characters) in `reason`
int emu_stark_perm_problem(const lcp2_stark_desc *d, const lcp2_stark_perm *perm, char *reason, unsigned len) {
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  std::string why;
  if (!st_desc_problem(d, point_polys, why, perm, &numZ)) return 0;
  if (len) { std::strncpy(reason, why.c_str(), len - 1); reason[len - 1] = 0; }
  return 1;
}

// draws: 2 * batch_size * num_challenges words in the order they are drawn.  ratio, zs: [numZ][n].  Returns the smallest z whose
// product does not close, -1 if all close, -2 for a refused description
int emu_stark_perm_columns(const lcp2_stark_desc *d, const lcp2_stark_perm *perm, const unsigned long long *draws, const unsigned long long *trace,
                           unsigned threads, unsigned long long *ratio, unsigned long long *zs) {
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  std::string why;
  if (st_desc_problem(d, point_polys, why, perm, &numZ) || !numZ || !threads) return -2;
  StPerm Pm = {};
  const std::vector<u64> tab = st_perm_stage(*d, *perm, draws, &Pm);
  const u64 n = 1ull << d->log_n;
  for (u32 z = 0; z < numZ; z++)
    for (u64 block = 0; block * threads * ST_PERM_ROWS < n; block++)
      for (u32 t = 0; t < threads; t++) {
        const u64 row0 = block * threads * ST_PERM_ROWS + t;
        if (row0 < n) st_perm_ratio_rows(Pm, trace, n, row0, threads, z, ratio);
      }
  for (u32 z = 0; z < numZ; z++) {
    u64 acc = 1;
    for (u64 r = 0; r < n; r++) { zs[z * n + r] = acc; acc = gl_mul(acc, ratio[z * n + r]); }
  }
  for (u32 z = 0; z < numZ; z++)
    if (!st_perm_closes(zs, ratio, n, z)) return (int)z;
  return -1;
}

// the quotient values of every point: lde, z_lde = the LDEs [width][N] and [numZ][N] in leaf order, out = [num_challenges][n << q]
int emu_stark_perm_quotient(const lcp2_stark_desc *d, const lcp2_stark_perm *perm, const unsigned long long *draws, const unsigned long long *public_inputs,
                            const unsigned long long *lde, const unsigned long long *z_lde, const unsigned long long *alphas, unsigned long long *out) {
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  std::string why;
  if (st_desc_problem(d, point_polys, why, perm, &numZ) || !numZ) return 1;
  const StStaged S = st_stage(*d, public_inputs);
  const StPrograms P = S.view(*d);
  StPerm Pm = {};
  const std::vector<u64> tab = st_perm_stage(*d, *perm, draws, &Pm);
  StCoset C = st_make_coset(d->log_n, d->quotient_degree_bits);
  std::vector<u64> lo(1ull << C.lo_bits), hi(1ull << (C.lgM - C.lo_bits));
  for (u64 j = 0; j < lo.size(); j++) lo[j] = st_coset_lo(C.lgM, j);
  for (u64 j = 0; j < hi.size(); j++) hi[j] = st_coset_hi(C.lgM, j);
  C.x_lo = lo.data(); C.x_hi = hi.data();
  u64 regs[ST_MAX_REGS + 1];
  const u32 lgN = d->log_n + d->fri.rate_bits;
  for (u64 i = 0; i < (1ull << C.lgM); i++) st_quotient_point<true>(P, C, lde, 1ull << lgN, lgN, d->fri.rate_bits, alphas, i, regs, out, &Pm, z_lde);
  return 0;
}

int emu_stark_perm_verify(const lcp2_stark_desc *d, const lcp2_stark_perm *perm, const unsigned long long *public_inputs, lcp2_challenger *ch,
                          const unsigned long long *proof, unsigned long long proof_words, int *failed_check) {
  std::string why;
  return st_verify(d, public_inputs, ch, proof, (size_t)proof_words, failed_check, why, perm);
}

}  // extern "C"
