// Openings of bare oracles (lcp2_fri_prove_openings / lcp2_fri_verify_openings) as portable text, the way verify_query.hpp holds the
// query phase of a Plonk proof: the layout both sides derive their offsets from, the composition and division the k_open_* kernels
// of fri_openings.hip run per coefficient, and the whole verifier - its head on the host, its per-query text written for host and
// device alike.  tests/emu/emu_openings.cpp compiles all of it for the CPU.
//
// The committed polynomial is plonky2's batch combination in coefficient form.  With C_b = sum_j alpha^j f_j over the polynomials
// of batch b in order and k_b their number,
//     F = sum_b alpha^(k_{b+1} + .. + k_last) (C_b - C_b(zeta_b)) / (X - zeta_b),
// and coefficient i of (C - C(z)) / (X - z) is  z^-(i+1) sum_{j > i} c_j z^j:  fo_compose_coeff writes t_b[i] = c_b[i] zeta_b^i,
// a reversed exclusive scan makes the suffix sums, fo_divide_coeff multiplies by the inverse powers and the shifts and adds the
// batches.  A column is loaded ONCE however many points list it: per column the table holds one extension weight per point (the sum
// of alpha^position over its appearances in that batch) and a mask of the points that list it.
#pragma once
#include <string>
#include <vector>
#include "host_protocol.hpp"
#include "verify_query.hpp"

namespace lcp2 {

constexpr u32 FO_CHECK_CANON = 1, FO_CHECK_POW = 2, FO_CHECK_INITIAL_PATH = 3, FO_CHECK_LAYER_PATH = 4, FO_CHECK_FOLD = 5,
              FO_CHECK_FINAL_POLY = 6, FO_CHECK_POINT = 7;
constexpr u32 FO_MAX_ORACLES = LCP2_FRI_MAX_ORACLES, FO_MAX_POINTS = LCP2_FRI_MAX_POINTS;

// ---- the layout: every offset in words, from the config and the shape alone
struct FoLayout {
  u64 total, fri_caps, queries, query_words, final_poly, pow_witness;
  u32 num_oracles, num_points, num_layers, num_queries, log_n, lgN, cap_height, capw, final_len, init_sib, pow_bits, total_polys;
  u32 point_off[FO_MAX_POINTS], point_polys[FO_MAX_POINTS];   // openings of point b: 2 * point_polys[b] words at point_off[b]
  u32 init_off[FO_MAX_ORACLES], init_cols[FO_MAX_ORACLES];    // inside a query round: leaf of oracle o, then 4 * init_sib sibling words
  u32 arity_bits[LCP2_MAX_FRI_LAYERS], step_off[LCP2_MAX_FRI_LAYERS], step_sib[LCP2_MAX_FRI_LAYERS];
};
// point_polys[b]: the polynomials of batch b (the sum of its ranges' num_polys).  The shape must have passed fo_shape_problem.
LCP2_HD FoLayout fo_make_layout(const lcp2_fri_config &cfg, u32 log_n, const u32 *oracle_cols, u32 num_oracles, const u32 *point_polys,
                                u32 num_points) {
  FoLayout L = {};
  L.num_oracles = num_oracles; L.num_points = num_points; L.num_layers = cfg.num_fri_layers; L.num_queries = cfg.num_query_rounds;
  L.log_n = log_n; L.lgN = log_n + cfg.rate_bits; L.cap_height = cfg.cap_height; L.capw = 4u << cfg.cap_height; L.pow_bits = cfg.proof_of_work_bits;
  u64 o = 0;
  for (u32 b = 0; b < num_points; b++) { L.point_off[b] = (u32)o; L.point_polys[b] = point_polys[b]; L.total_polys += point_polys[b]; o += 2ull * point_polys[b]; }
  L.fri_caps = o; o += (u64)cfg.num_fri_layers * L.capw;
  L.init_sib = L.lgN - cfg.cap_height;
  u32 q = 0;
  for (u32 i = 0; i < num_oracles; i++) { L.init_off[i] = q; L.init_cols[i] = oracle_cols[i]; q += oracle_cols[i] + 4 * L.init_sib; }
  u32 lg = L.lgN, fl = log_n;
  for (u32 l = 0; l < cfg.num_fri_layers; l++) {
    const u32 ab = cfg.fri_arity_bits[l];
    lg -= ab; fl -= ab;
    L.arity_bits[l] = ab; L.step_off[l] = q; L.step_sib[l] = lg - cfg.cap_height;
    q += (2u << ab) + 4 * L.step_sib[l];
  }
  L.query_words = q;
  L.queries = o; o += (u64)q * cfg.num_query_rounds;
  L.final_len = 1u << fl;
  L.final_poly = o; o += 2ull * L.final_len;
  L.pow_witness = o; o += 1;
  L.total = o;
  return L;
}

// ---- refusals shared by the word count, the prover and the verifier (host).  nullptr, or the reason
inline const char *fo_config_problem(const lcp2_fri_config &c, u32 log_n) {
  if (log_n < 1 || c.rate_bits < 1 || c.rate_bits > 8 || log_n + c.rate_bits > 30) return "log_n / rate_bits out of range";
  if (c.cap_height > log_n + c.rate_bits) return "cap_height exceeds the LDE tree";
  if (c.num_query_rounds < 1 || c.num_query_rounds > VQ_MAX_QUERIES || c.num_fri_layers > LCP2_MAX_FRI_LAYERS) return "too many queries / layers";
  if (c.proof_of_work_bits > 40) return "proof_of_work_bits out of range";
  u32 lg = log_n + c.rate_bits, d = log_n;
  for (u32 l = 0; l < c.num_fri_layers; l++) {
    const u32 ab = c.fri_arity_bits[l];
    if (ab < 1 || ab > 5 || ab > d || lg - ab < c.cap_height) return "bad FRI arity schedule";
    lg -= ab; d -= ab;
  }
  return nullptr;
}
// the instance against the column counts of its oracles; point_polys[FO_MAX_POINTS] receives the batch sizes
inline bool fo_shape_problem(const lcp2_fri_config *cfg, u32 log_n, const u32 *oracle_cols, const lcp2_fri_instance *inst, u32 *point_polys,
                             std::string &why) {
  if (!cfg || !oracle_cols || !inst) { why = "null argument"; return true; }
  if (const char *w = fo_config_problem(*cfg, log_n)) { why = w; return true; }
  if (inst->num_oracles < 1 || inst->num_oracles > FO_MAX_ORACLES) { why = "num_oracles outside [1, LCP2_FRI_MAX_ORACLES]"; return true; }
  if (inst->num_points < 1 || inst->num_points > FO_MAX_POINTS) { why = "num_points outside [1, LCP2_FRI_MAX_POINTS]"; return true; }
  for (u32 o = 0; o < inst->num_oracles; o++)
    if (oracle_cols[o] < 1 || oracle_cols[o] > 65535) { why = "oracle " + std::to_string(o) + ": bad column count"; return true; }
  for (u32 b = 0; b < inst->num_points; b++) {
    if (inst->num_ranges[b] < 1 || !inst->ranges[b]) { why = "point " + std::to_string(b) + " has no range"; return true; }
    u64 polys = 0;
    for (u32 r = 0; r < inst->num_ranges[b]; r++) {
      const lcp2_fri_range &g = inst->ranges[b][r];
      if (g.oracle >= inst->num_oracles || g.num_polys < 1 || (u64)g.first_poly + g.num_polys > oracle_cols[g.oracle]) {
        why = "point " + std::to_string(b) + " range " + std::to_string(r) + " does not lie inside its oracle";
        return true;
      }
      polys += g.num_polys;
    }
    if (polys > (1u << 24)) { why = "point " + std::to_string(b) + ": too many polynomials"; return true; }
    point_polys[b] = (u32)polys;
  }
  return false;
}
// the points, reduced; zeta = 0 has no inverse powers
inline bool fo_points_problem(const u64 *points, u32 num_points, gl2 *z, std::string &why) {
  if (!points) { why = "null points"; return true; }
  for (u32 b = 0; b < num_points; b++) {
    z[b] = gl2_make(points[2 * b] % GL_P, points[2 * b + 1] % GL_P);
    if ((z[b].c0 | z[b].c1) == 0) { why = "point " + std::to_string(b) + " is 0 (the opening divides by powers of the point)"; return true; }
  }
  return false;
}
// the ranges of all points back to back, as the per-query text and the weight table read them
struct FoRanges {
  std::vector<lcp2_fri_range> list;
  u32 first[FO_MAX_POINTS + 1] = {0};
};
inline FoRanges fo_flatten(const lcp2_fri_instance &inst) {
  FoRanges R;
  for (u32 b = 0; b < inst.num_points; b++) {
    R.first[b] = (u32)R.list.size();
    R.list.insert(R.list.end(), inst.ranges[b], inst.ranges[b] + inst.num_ranges[b]);
  }
  for (u32 b = inst.num_points; b <= FO_MAX_POINTS; b++) R.first[b] = (u32)R.list.size();
  return R;
}

// ---- composition and division per coefficient (k_open_compose / k_open_divide)
struct FoCompose {
  const u64 *coeffs[FO_MAX_ORACLES];  // [ncols][n] each, canonical
  u32 ncols[FO_MAX_ORACLES];
  u32 num_oracles, num_points;
  u64 n;
  const u64 *weights;   // [total columns][FO_MAX_POINTS][2]: the extension weight of the column in each batch
  const u32 *mask;      // [total columns]: bit b set iff batch b lists the column
  const u64 *tables;    // per point: zeta^j (j < 2^zh), zeta^(j << zh) (j < hi_count), then the same of 1 / zeta; extension elements
  u32 zh;
  u64 hi_count;
  u64 shift[FO_MAX_POINTS][2];  // alpha^(polynomials of the batches after b)
  u64 *planes;          // [num_points][2][n]: t_b, then (scanned in place) the exclusive suffix sums
};
LCP2_HD u64 fo_table_words(u32 zh, u64 hi_count) { return 4 * ((1ull << zh) + hi_count); }  // per point
// entry j of point z's table: j < per: a power of z, else of 1 / z (per = 2^zh + hi_count entries each)
LCP2_HD gl2 fo_table_entry(gl2 z, u32 zh, u64 hi_count, u64 j) {
  const u64 per = (1ull << zh) + hi_count;
  if (j >= per) { z = gl2_inv(z); j -= per; }
  return j < (1ull << zh) ? gl2_pow(z, j) : gl2_pow(z, (j - (1ull << zh)) << zh);
}
// z_b^e (inverse = false) or z_b^-e from the two-level tables, e <= n
LCP2_HD gl2 fo_point_pow(const FoCompose &a, u32 b, u64 e, bool inverse) {
  const u64 per = (1ull << a.zh) + a.hi_count;
  const u64 *T = a.tables + (u64)b * fo_table_words(a.zh, a.hi_count) + (inverse ? 2 * per : 0);
  const u64 lo = e & ((1ull << a.zh) - 1), hi = (1ull << a.zh) + (e >> a.zh);
  return gl2_mul(gl2_make(T[2 * lo], T[2 * lo + 1]), gl2_make(T[2 * hi], T[2 * hi + 1]));
}
// planes[b][.][i] = zeta_b^i sum_columns weight_b[column] f_column[i]
LCP2_HD void fo_compose_coeff(const FoCompose &a, u64 i) {
  gl2 acc[FO_MAX_POINTS];
  for (u32 b = 0; b < FO_MAX_POINTS; b++) acc[b] = gl2_make(0, 0);
  u32 g = 0;
  for (u32 o = 0; o < a.num_oracles; o++) {
    const u64 *cf = a.coeffs[o] + i;
    for (u32 c = 0; c < a.ncols[o]; c++, g++) {
      const u32 m = a.mask[g];
      if (!m) continue;
      const u64 v = cf[(u64)c * a.n];
      const u64 *w = a.weights + (u64)g * 2 * FO_MAX_POINTS;
#pragma unroll
      for (u32 b = 0; b < FO_MAX_POINTS; b++)
        if (m >> b & 1) { acc[b].c0 = gl_add(acc[b].c0, gl_mul(w[2 * b], v)); acc[b].c1 = gl_add(acc[b].c1, gl_mul(w[2 * b + 1], v)); }
    }
  }
#pragma unroll
  for (u32 b = 0; b < FO_MAX_POINTS; b++)
    if (b < a.num_points) {
      const gl2 t = gl2_mul(acc[b], fo_point_pow(a, b, i, false));
      a.planes[(2ull * b) * a.n + i] = t.c0; a.planes[(2ull * b + 1) * a.n + i] = t.c1;
    }
}
// the planes hold the exclusive suffix sums S_b[i] = sum_{j > i} t_b[j]:  F_i = sum_b shift_b zeta_b^-(i+1) S_b[i]
LCP2_HD void fo_divide_coeff(const FoCompose &a, u64 i, u64 *out0, u64 *out1) {
  gl2 r = gl2_make(0, 0);
  for (u32 b = 0; b < a.num_points; b++) {
    const gl2 s = gl2_make(a.planes[(2ull * b) * a.n + i], a.planes[(2ull * b + 1) * a.n + i]);
    r = gl2_add(r, gl2_mul(gl2_mul(s, fo_point_pow(a, b, i + 1, true)), gl2_make(a.shift[b][0], a.shift[b][1])));
  }
  out0[i] = r.c0; out1[i] = r.c1;
}
// host: the weight table, the masks and the shifts of an instance for one alpha.  col_base[o]: the first table row of oracle o
inline void fo_make_weights(const lcp2_fri_instance &inst, const u32 *oracle_cols, gl2 alpha, std::vector<u64> &weights, std::vector<u32> &mask,
                            u64 shift[FO_MAX_POINTS][2]) {
  u32 base[FO_MAX_ORACLES + 1] = {0};
  for (u32 o = 0; o < inst.num_oracles; o++) base[o + 1] = base[o] + oracle_cols[o];
  weights.assign((size_t)base[inst.num_oracles] * 2 * FO_MAX_POINTS, 0);
  mask.assign(base[inst.num_oracles], 0);
  gl2 after = gl2_make(1, 0);  // alpha^(polynomials of the batches after b), from the last batch down
  for (u32 b = inst.num_points; b-- > 0;) {
    shift[b][0] = after.c0; shift[b][1] = after.c1;
    gl2 w = gl2_make(1, 0);
    for (u32 r = 0; r < inst.num_ranges[b]; r++)
      for (u32 j = 0; j < inst.ranges[b][r].num_polys; j++) {
        const u32 g = base[inst.ranges[b][r].oracle] + inst.ranges[b][r].first_poly + j;
        u64 *e = &weights[((size_t)g * FO_MAX_POINTS + b) * 2];
        e[0] = gl_add(e[0], w.c0); e[1] = gl_add(e[1], w.c1);
        mask[g] |= 1u << b;
        w = gl2_mul(w, alpha);
      }
    after = gl2_mul(after, w);  // w = alpha^(polynomials of batch b)
  }
}

// ---- the verifier.  What its head leaves for the queries:
struct FoChallenge {
  gl2 alpha, point[FO_MAX_POINTS], reduced[FO_MAX_POINTS], batch_shift[FO_MAX_POINTS];  // batch_shift[b] = alpha^(polynomials of batch b)
  gl2 betas[LCP2_MAX_FRI_LAYERS];
  u32 x_index[VQ_MAX_QUERIES];
};
// Query q: 0, or the first check that fails.  ranges: the flattened ranges, range_first[b] .. range_first[b + 1] those of point b;
// caps[o]: the cap of oracle o; rc: the 360 round constants.  Every offset comes from L; x_index < 2^lgN.
LCP2_HD u32 fo_verify_query(const FoLayout &L, const FoChallenge &c, const lcp2_fri_range *ranges, const u32 *range_first, const u64 *proof,
                            const u64 *const *caps, u32 q, const u64 *rc) {
  const u64 *R = proof + L.queries + (u64)q * L.query_words;
  u64 xi = c.x_index[q];
  for (u32 o = 0; o < L.num_oracles; o++) {
    const u64 *leaf = R + L.init_off[o];
    if (!vq_merkle_path(leaf, L.init_cols[o], xi, leaf + L.init_cols[o], L.init_sib, caps[o], rc)) return FO_CHECK_INITIAL_PATH;
  }
  u64 subgroup_x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(L.lgN), bitrev32((u32)xi, L.lgN)));
  const gl2 x = gl2_make(subgroup_x, 0);
  gl2 eval = gl2_make(0, 0);
  for (u32 b = 0; b < L.num_points; b++) {
    const gl2 den = gl2_sub(x, c.point[b]);
    if ((den.c0 | den.c1) == 0) return FO_CHECK_POINT;
    gl2 r = gl2_make(0, 0);
    for (u32 k = range_first[b + 1]; k-- > range_first[b];) {
      const u64 *leaf = R + L.init_off[ranges[k].oracle] + ranges[k].first_poly;
      for (u32 j = ranges[k].num_polys; j-- > 0;) r = gl2_add_base(gl2_mul(r, c.alpha), leaf[j]);
    }
    eval = gl2_add(gl2_mul(eval, c.batch_shift[b]), gl2_mul(gl2_sub(r, c.reduced[b]), gl2_inv(den)));
  }
  for (u32 l = 0; l < L.num_layers; l++) {
    const u32 ab = L.arity_bits[l], within = (u32)xi & ((1u << ab) - 1);
    const u64 *evals = R + L.step_off[l];
    if (!gl2_eq(vq_rd2(evals + 2 * within), eval)) return FO_CHECK_FOLD;
    xi >>= ab;
    if (!vq_merkle_path(evals, 2u << ab, xi, evals + (2u << ab), L.step_sib[l], proof + L.fri_caps + (u64)l * L.capw, rc)) return FO_CHECK_LAYER_PATH;
    eval = vq_compute_evaluation(subgroup_x, within, ab, evals, c.betas[l]);
    for (u32 i = 0; i < ab; i++) subgroup_x = gl_sqr(subgroup_x);
  }
  gl2 fv = gl2_make(0, 0);
  for (u32 j = L.final_len; j-- > 0;) fv = gl2_add(gl2_mul(fv, gl2_make(subgroup_x, 0)), vq_rd2(proof + L.final_poly + 2 * j));
  return gl2_eq(fv, eval) ? 0 : FO_CHECK_FINAL_POLY;
}

// the transcript of the opening after the openings were observed is the prover's and the verifier's alike; what differs is where the
// caps and the final polynomial come from.  The verifier's head (host): canonical words, transcript, proof of work, reduced openings.
// Returns 0 or the failed check; ch is left in the state after the query indices unless check 1 fails.
inline u32 fo_verify_head(const FoLayout &L, const gl2 *points, const u64 *proof, HostChallenger &ch, FoChallenge &c) {
  for (u64 w = 0; w < L.total; w++)
    if (proof[w] >= GL_P) return FO_CHECK_CANON;
  ch.observe_n(proof, 2 * (size_t)L.total_polys);
  c.alpha = ch.get_ext();
  for (u32 b = 0; b < L.num_points; b++) {
    c.point[b] = points[b];
    gl2 r = gl2_make(0, 0);
    for (u32 j = L.point_polys[b]; j-- > 0;) r = gl2_add(gl2_mul(r, c.alpha), vq_rd2(proof + L.point_off[b] + 2 * j));
    c.reduced[b] = r;
    c.batch_shift[b] = gl2_pow(c.alpha, L.point_polys[b]);
  }
  for (u32 l = 0; l < L.num_layers; l++) {
    ch.observe_n(proof + L.fri_caps + (u64)l * L.capw, L.capw);
    c.betas[l] = ch.get_ext();
  }
  ch.observe_n(proof + L.final_poly, 2 * (size_t)L.final_len);
  ch.observe(proof[L.pow_witness]);
  const u64 response = ch.get();
  const bool pow_ok = L.pow_bits == 0 || (response >> (64 - L.pow_bits)) == 0;
  for (u32 q = 0; q < L.num_queries; q++) c.x_index[q] = (u32)(ch.get() & ((1ull << L.lgN) - 1));
  return pow_ok ? 0 : FO_CHECK_POW;
}

// lcp2_fri_verify_openings without its ABI dress: LCP2_OK / LCP2_E_VERIFY / LCP2_E_INVALID (why says why).  after_head(L): a check
// of the caller's between checks 1 and 2 and the queries (0, or the number it reports): the STARK verifier's identity (stark.hpp).
template <class AfterHead>
inline int fo_verify_openings(const u64 *const *caps, const u32 *oracle_cols, u32 log_n, const lcp2_fri_instance *inst, const u64 *points,
                              const lcp2_fri_config *cfg, lcp2_challenger *chs, const u64 *proof, size_t proof_words, int32_t *failed_check,
                              std::string &why, AfterHead after_head) {
  if (failed_check) *failed_check = 0;
  u32 point_polys[FO_MAX_POINTS] = {0};
  gl2 z[FO_MAX_POINTS];
  if (!caps || !chs || !proof) { why = "null argument"; return LCP2_E_INVALID; }
  if (fo_shape_problem(cfg, log_n, oracle_cols, inst, point_polys, why) || fo_points_problem(points, inst->num_points, z, why)) return LCP2_E_INVALID;
  for (u32 o = 0; o < inst->num_oracles; o++)
    if (!caps[o]) { why = "null cap"; return LCP2_E_INVALID; }
  if (chs->input_len >= 8 || chs->output_len > 8) { why = "broken challenger state"; return LCP2_E_INVALID; }
  const FoLayout L = fo_make_layout(*cfg, log_n, oracle_cols, inst->num_oracles, point_polys, inst->num_points);
  if (proof_words != L.total) { why = "proof_words is not lcp2_fri_openings_words"; return LCP2_E_INVALID; }
  HostChallenger ch;
  ch.load((const u64 *)chs->sponge, (const u64 *)chs->input, chs->input_len, (const u64 *)chs->output, chs->output_len);
  FoChallenge c = {};
  u32 failed = fo_verify_head(L, z, proof, ch, c);
  if (failed != FO_CHECK_CANON) ch.save((u64 *)chs->sponge, (u64 *)chs->input, chs->input_len, (u64 *)chs->output, chs->output_len);
  if (!failed) failed = after_head(L);
  if (!failed) {
    // the caps enter the paths as field elements: reduced copies
    std::vector<u64> cap_words((size_t)inst->num_oracles * L.capw);
    const u64 *cap_of[FO_MAX_ORACLES];
    for (u32 o = 0; o < inst->num_oracles; o++) {
      for (u32 i = 0; i < L.capw; i++) cap_words[(size_t)o * L.capw + i] = caps[o][i] % GL_P;
      cap_of[o] = cap_words.data() + (size_t)o * L.capw;
    }
    const FoRanges F = fo_flatten(*inst);
    for (u32 q = 0; q < L.num_queries && !failed; q++)
      failed = fo_verify_query(L, c, F.list.data(), F.first, proof, cap_of, q, HostPoseidon::get().round_constants());
  }
  if (failed_check) *failed_check = (int32_t)failed;
  return failed ? LCP2_E_VERIFY : LCP2_OK;
}
inline int fo_verify_openings(const u64 *const *caps, const u32 *oracle_cols, u32 log_n, const lcp2_fri_instance *inst, const u64 *points,
                              const lcp2_fri_config *cfg, lcp2_challenger *chs, const u64 *proof, size_t proof_words, int32_t *failed_check,
                              std::string &why) {
  return fo_verify_openings(caps, oracle_cols, log_n, inst, points, cfg, chs, proof, proof_words, failed_check, why, [](const FoLayout &) { return 0u; });
}

}  // namespace lcp2
