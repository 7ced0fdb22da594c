// TEST HARNESS (not product code): csrc/fri_openings.hpp compiled for the CPU - the layout, the composition and division the
// k_open_* kernels run per coefficient (as loops over the coefficients, with the reversed exclusive scan between them done here),
// the verifier of lcp2_fri_verify_openings, and the combination formula of verify_query.hpp for the two batches of a Plonk proof.
// Built by tests/test_fri_openings_emu.py with g++ and included by tests/emu/sanitize_openings_main.cpp; never loaded by the package.
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/fri_openings.hpp"

using namespace lcp2;

extern "C" {

// out[48]: total, fri_caps, queries, query_words, final_poly, pow_witness, final_len, init_sib, then point_off[4], init_off[8],
// step_off[8], step_sib[8], point_polys[4], init_cols[8]; returns 0, or 1 for a refused shape
int emu_open_layout(const lcp2_fri_config *cfg, unsigned log_n, const unsigned *oracle_cols, const lcp2_fri_instance *inst, unsigned long long *out) {
  u32 point_polys[FO_MAX_POINTS] = {0};
  std::string why;
  if (fo_shape_problem(cfg, log_n, oracle_cols, inst, point_polys, why)) return 1;
  const FoLayout L = fo_make_layout(*cfg, log_n, oracle_cols, inst->num_oracles, point_polys, inst->num_points);
  u64 *o = out;
  *o++ = L.total; *o++ = L.fri_caps; *o++ = L.queries; *o++ = L.query_words; *o++ = L.final_poly; *o++ = L.pow_witness; *o++ = L.final_len; *o++ = L.init_sib;
  for (u32 i = 0; i < 4; i++) *o++ = L.point_off[i];
  for (u32 i = 0; i < 8; i++) *o++ = L.init_off[i];
  for (u32 i = 0; i < 8; i++) *o++ = L.step_off[i];
  for (u32 i = 0; i < 8; i++) *o++ = L.step_sib[i];
  for (u32 i = 0; i < 4; i++) *o++ = L.point_polys[i];
  for (u32 i = 0; i < 8; i++) *o++ = L.init_cols[i];
  return 0;
}

// the committed polynomial of an instance: coeffs[o] = [oracle_cols[o]][n] canonical coefficients; out0 / out1: its n coefficients
int emu_open_compose(const lcp2_fri_instance *inst, const unsigned *oracle_cols, const unsigned long long *const *coeffs, unsigned log_n,
                     const unsigned long long *alpha, const unsigned long long *points, unsigned long long *out0, unsigned long long *out1) {
  gl2 z[FO_MAX_POINTS];
  std::string why;
  if (fo_points_problem(points, inst->num_points, z, why)) return 1;
  const u64 n = 1ull << log_n;
  FoCompose a = {};
  std::vector<u64> weights;
  std::vector<u32> mask;
  fo_make_weights(*inst, oracle_cols, gl2_make(alpha[0], alpha[1]), weights, mask, a.shift);
  a.zh = (log_n + 1) / 2; a.hi_count = (n >> a.zh) + 1;
  const u64 per_point = 2 * ((1ull << a.zh) + a.hi_count);
  std::vector<u64> tables(inst->num_points * fo_table_words(a.zh, a.hi_count)), planes(2 * inst->num_points * n);
  for (u32 b = 0; b < inst->num_points; b++)
    for (u64 j = 0; j < per_point; j++) {
      const gl2 v = fo_table_entry(z[b], a.zh, a.hi_count, j);
      tables[2 * (b * per_point + j)] = v.c0; tables[2 * (b * per_point + j) + 1] = v.c1;
    }
  for (u32 o = 0; o < inst->num_oracles; o++) { a.coeffs[o] = coeffs[o]; a.ncols[o] = oracle_cols[o]; }
  a.num_oracles = inst->num_oracles; a.num_points = inst->num_points; a.n = n;
  a.weights = weights.data(); a.mask = mask.data(); a.tables = tables.data(); a.planes = planes.data();
  for (u64 i = 0; i < n; i++) fo_compose_coeff(a, i);
  for (u32 p = 0; p < 2 * inst->num_points; p++) {  // launch_scan(add, reverse, exclusive)
    u64 run = 0;
    for (u64 i = n; i-- > 0;) { const u64 t = planes[p * n + i]; planes[p * n + i] = run; run = gl_add(run, t); }
  }
  for (u64 i = 0; i < n; i++) fo_divide_coeff(a, i, out0, out1);
  return 0;
}

// vq_combine_initial of verify_query.hpp for leaves of cols[0..3] columns laid out back to back in `leaves`: out[2]
void emu_open_vq_combine(const unsigned *cols, unsigned num_challenges, const unsigned long long *leaves, const unsigned long long *alpha,
                         const unsigned long long *zeta, const unsigned long long *g_zeta, const unsigned long long *red0,
                         const unsigned long long *red1, unsigned long long x, unsigned long long *out) {
  VqLayout V = {};
  VqChallenge c = {};
  u32 off = 0;
  for (u32 o = 0; o < 4; o++) { V.tree[o].leaf_off = off; V.tree[o].leaf_len = cols[o]; off += cols[o]; }
  V.zs_leaf_off = V.tree[2].leaf_off; V.num_challenges = num_challenges;
  c.fri_alpha = gl2_make(alpha[0], alpha[1]); c.zeta = gl2_make(zeta[0], zeta[1]); c.g_zeta = gl2_make(g_zeta[0], g_zeta[1]);
  c.red0 = gl2_make(red0[0], red0[1]); c.red1 = gl2_make(red1[0], red1[1]);
  c.alpha_ch = gl2_pow(c.fri_alpha, num_challenges);
  const gl2 r = vq_combine_initial(V, c, leaves, x);
  out[0] = r.c0; out[1] = r.c1;
}

unsigned long long emu_open_words(const lcp2_fri_config *cfg, unsigned log_n, const unsigned *oracle_cols, const lcp2_fri_instance *inst) {
  u32 point_polys[FO_MAX_POINTS] = {0};
  std::string why;
  if (fo_shape_problem(cfg, log_n, oracle_cols, inst, point_polys, why)) return 0;
  return fo_make_layout(*cfg, log_n, oracle_cols, inst->num_oracles, point_polys, inst->num_points).total;
}

int emu_open_verify(const unsigned long long *const *caps, const unsigned *oracle_cols, unsigned log_n, const lcp2_fri_instance *inst,
                    const unsigned long long *points, const lcp2_fri_config *cfg, lcp2_challenger *ch, const unsigned long long *proof,
                    unsigned long long proof_words, int *failed_check) {
  std::string why;
  return fo_verify_openings(caps, oracle_cols, log_n, inst, points, cfg, ch, proof, (size_t)proof_words, failed_check, why);
}

}  // extern "C"
