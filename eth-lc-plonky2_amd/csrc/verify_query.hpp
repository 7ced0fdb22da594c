// The query phase of data.verify(proof) - checks 4 to 7 of lcp2_verify - as portable text: what the host verifier (verifier.hip)
// runs query by query, what lcp2_verify_batch (verify_batch.hip, kernels_verify.hip) runs for every query of every proof at once on
// the device, and what tests/emu/emu_verify.cpp runs on the CPU.
//
// A proof is read only through VqLayout, the circuit's ProofLayout restated in words a kernel can take by value: every offset,
// leaf length and sibling count comes from the circuit's parameters and none from the proof, and the query indices are reduced mod
// N by the host, so no proof content moves a read outside the proof's own words.
//
// The work of one proof is  num_queries x num_trees  Merkle paths (tree t < 4: initial oracle t; tree 4 + l: FRI layer l) and
// num_queries FRI queries.  vq_merkle_path is one path walked by ONE lane, the reference form of what a 16-lane group of
// k_verify_paths does; vq_fri_query is the text a lane of k_verify_fri runs.  Each reports into the status word of its
// (proof, query) by minimum of  ordinal << 8 | check,  the ordinals in the order in which the host verifier meets the checks inside
// a query; the verdict of a proof is the status of its first query that has one (vq_reduce_statuses).
#pragma once
#include "../../include/lcp2.h"
#include "poseidon.hpp"

namespace lcp2 {

constexpr u32 VQ_MAX_QUERIES = 64;
constexpr u32 VQ_MAX_TREES = 4 + LCP2_MAX_FRI_LAYERS;
constexpr u32 VQ_CHECK_INITIAL_PATH = 4, VQ_CHECK_CONSISTENCY = 5, VQ_CHECK_LAYER_PATH = 6, VQ_CHECK_FINAL_POLY = 7;

// ---- status word of one (proof, query)
constexpr u32 VQ_STATUS_NONE = 0xFFFFFFFFu;
LCP2_HD u32 vq_status(u32 ordinal, u32 check) { return ordinal << 8 | check; }
LCP2_HD u32 vq_ord_initial(u32 oracle) { return oracle; }
LCP2_HD u32 vq_ord_consistency(u32 layer) { return 4 + 2 * layer; }
LCP2_HD u32 vq_ord_layer_path(u32 layer) { return 5 + 2 * layer; }
LCP2_HD u32 vq_ord_final(u32 num_layers) { return 4 + 2 * num_layers; }
// the failed check of a proof from the statuses of its queries: the first query that has one, 0 if none has
LCP2_HD u32 vq_reduce_statuses(const u32 *status, u32 num_queries) {
  for (u32 q = 0; q < num_queries; q++)
    if (status[q] != VQ_STATUS_NONE) return status[q] & 0xFF;
  return 0;
}

// ---- what the host derives from the words of a proof outside its query section (transcript, reduced openings), one per proof
struct VqChallenge {
  gl2 zeta, g_zeta, fri_alpha, alpha_ch, red0, red1;
  gl2 fri_betas[LCP2_MAX_FRI_LAYERS];
  u32 x_index[VQ_MAX_QUERIES];  // < N
  u32 live, pad;                // 0: a check before the queries has failed already and no job of this proof runs
};

struct VqTree {
  u32 leaf_off, leaf_len, nsib;  // inside a query: the leaf, then 4 * nsib sibling words
  u32 cap_off;                   // of the tree's cap inside the proof (tree 0: unused, its cap is the circuit's)
  u32 index_shift;               // leaf index = x_index >> index_shift
  u32 status;                    // what a failed path reports
};
struct VqLayout {
  u64 proof_words, queries, query_words, final_poly;
  u32 num_queries, num_trees, num_layers, lgN, final_len, num_challenges, capw, zs_leaf_off;
  u32 arity_bits[LCP2_MAX_FRI_LAYERS];
  VqTree tree[VQ_MAX_TREES];
};
// L: host_protocol.hpp ProofLayout of p
template <class Layout>
inline VqLayout vq_make_layout(const Layout &L, const lcp2_params &p) {
  VqLayout V = {};
  V.proof_words = L.total; V.queries = L.queries; V.query_words = L.query_words; V.final_poly = L.final_poly;
  V.num_queries = p.num_query_rounds; V.num_layers = p.num_fri_layers; V.num_trees = 4 + p.num_fri_layers;
  V.lgN = p.degree_bits + p.rate_bits; V.final_len = (u32)L.final_len; V.num_challenges = p.num_challenges; V.capw = (u32)L.capw;
  V.zs_leaf_off = (u32)L.q_init_off[2];
  const size_t caps[4] = {0, L.wires_cap, L.zs_cap, L.quot_cap};
  for (u32 o = 0; o < 4; o++)
    V.tree[o] = {(u32)L.q_init_off[o], (u32)L.q_init_cols[o], (u32)L.q_init_sib, (u32)caps[o], 0, vq_status(vq_ord_initial(o), VQ_CHECK_INITIAL_PATH)};
  u32 shift = 0;
  for (u32 l = 0; l < p.num_fri_layers; l++) {
    V.arity_bits[l] = p.fri_arity_bits[l];
    shift += p.fri_arity_bits[l];
    V.tree[4 + l] = {(u32)L.q_step_off[l], 2u << p.fri_arity_bits[l], (u32)L.q_step_sib[l], (u32)(L.fri_caps + l * L.capw), shift,
                     vq_status(vq_ord_layer_path(l), VQ_CHECK_LAYER_PATH)};
  }
  return V;
}

// ---- Merkle paths (plonky2 hash/merkle_proofs.rs verify_merkle_proof_to_cap), one lane.  rc: the 360 round constants
LCP2_HD void vq_hash_or_noop(const u64 *in, u32 len, u64 out[4], const u64 *rc) {
  u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (len <= 4) {
    for (u32 i = 0; i < len; i++) s[i] = gl_canon(in[i]);
  } else {
    for (u32 off = 0; off < len; off += 8) {
      for (u32 i = 0; i < 8 && off + i < len; i++) s[i] = gl_canon(in[off + i]);
      pos_permute(s, rc);
    }
  }
  for (u32 i = 0; i < 4; i++) out[i] = s[i];
}
LCP2_HD bool vq_merkle_path(const u64 *leaf, u32 leaf_len, u64 index, const u64 *siblings, u32 nsib, const u64 *cap, const u64 *rc) {
  u64 cur[4];
  vq_hash_or_noop(leaf, leaf_len, cur, rc);
  for (u32 k = 0; k < nsib; k++) {
    const u64 *sib = siblings + 4 * k;
    u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (u32 i = 0; i < 4; i++) { s[i] = (index & 1) ? sib[i] : cur[i]; s[4 + i] = (index & 1) ? cur[i] : sib[i]; }
    pos_permute(s, rc);
    for (u32 i = 0; i < 4; i++) cur[i] = s[i];
    index >>= 1;
  }
  bool same = true;
  for (u32 i = 0; i < 4; i++) same = same && cur[i] == cap[4 * index + i];
  return same;
}
// where path (q, t) of a proof lies; cs_cap: the circuit's constants_sigmas cap
struct VqPath {
  const u64 *leaf, *siblings, *cap;
  u32 leaf_len, nsib, status;
  u64 index;
};
LCP2_HD VqPath vq_path_of(const VqLayout &V, const VqChallenge &c, const u64 *proof, const u64 *cs_cap, u32 q, u32 t) {
  const VqTree T = V.tree[t];
  VqPath p;
  p.leaf = proof + V.queries + (u64)q * V.query_words + T.leaf_off;
  p.siblings = p.leaf + T.leaf_len;
  p.cap = t == 0 ? cs_cap : proof + T.cap_off;
  p.leaf_len = T.leaf_len; p.nsib = T.nsib; p.status = T.status;
  p.index = c.x_index[q] >> T.index_shift;
  return p;
}
// VQ_STATUS_NONE, or the status of the failed path
LCP2_HD u32 vq_path_job(const VqLayout &V, const VqChallenge &c, const u64 *proof, const u64 *cs_cap, u32 q, u32 t, const u64 *rc) {
  const VqPath p = vq_path_of(V, c, proof, cs_cap, q, t);
  return vq_merkle_path(p.leaf, p.leaf_len, p.index, p.siblings, p.nsib, p.cap, rc) ? VQ_STATUS_NONE : p.status;
}

// ---- FRI queries (plonky2 fri/verifier.rs)
LCP2_HD gl2 vq_rd2(const u64 *p) { return gl2_make(p[0], p[1]); }
LCP2_HD u64 vq_subgroup_x(const VqLayout &V, u32 x_index) {
  return gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(V.lgN), bitrev32(x_index, V.lgN)));
}
// fri_combine_initial: the alpha-reduction over the four leaves of query R, divided by x - zeta, and that of the Z columns by x - g zeta
LCP2_HD gl2 vq_combine_initial(const VqLayout &V, const VqChallenge &c, const u64 *R, u64 subgroup_x) {
  const gl2 x = gl2_make(subgroup_x, 0);
  gl2 r0 = gl2_make(0, 0);
  for (int o = 3; o >= 0; o--) {
    const u64 *leaf = R + V.tree[o].leaf_off;
    for (u32 j = V.tree[o].leaf_len; j-- > 0;) r0 = gl2_add_base(gl2_mul(r0, c.fri_alpha), leaf[j]);
  }
  gl2 sum = gl2_mul(gl2_sub(r0, c.red0), gl2_inv(gl2_sub(x, c.zeta)));
  gl2 r1 = gl2_make(0, 0);
  for (u32 j = V.num_challenges; j-- > 0;) r1 = gl2_add_base(gl2_mul(r1, c.fri_alpha), R[V.zs_leaf_off + j]);
  return gl2_add(gl2_mul(sum, c.alpha_ch), gl2_mul(gl2_sub(r1, c.red1), gl2_inv(gl2_sub(x, c.g_zeta))));
}
// compute_evaluation: the value at beta of the interpolant of degree < arity through the coset of x; evals: the layer's leaf (arity
// extension elements in bit-reversed order), within: the position of x in it.  With g of order arity and the points p_i = s g^i
// (s = x g^(arity - rev(within))), the Lagrange denominator prod_{j != i} (p_i - p_j) is arity p_i^(arity - 1) (the product of
// 1 - g^k over k = 1 .. arity - 1 is arity), whose inverse is K g^i with K = 1 / (arity s^(arity - 1)): one inversion per layer, no
// table of points, and the evals are read where they lie.
LCP2_HD gl2 vq_compute_evaluation(u64 x, u32 within, u32 arity_bits, const u64 *evals, gl2 beta) {
  const u32 arity = 1u << arity_bits;
  const u64 g = gl_root_of_unity(arity_bits);
  const u64 s = gl_mul(x, gl_pow(g, arity - bitrev32(within, arity_bits)));
  const u64 K = gl_inv(gl_mul(arity, gl_pow(s, arity - 1)));
  gl2 acc = gl2_make(0, 0);
  u64 gi = 1;
  for (u32 i = 0; i < arity; i++) {
    gl2 num = gl2_make(1, 0);
    u64 pj = s;
    for (u32 j = 0; j < arity; j++) {
      if (j != i) num = gl2_mul(num, gl2_sub_base(beta, pj));
      pj = gl_mul(pj, g);
    }
    acc = gl2_add(acc, gl2_mul(vq_rd2(evals + 2 * bitrev32(i, arity_bits)), gl2_scale(num, gl_mul(K, gi))));
    gi = gl_mul(gi, g);
  }
  return acc;
}
// One layer of the fold chain of query R: false when evals[within] is not the value carried so far (check 5); otherwise eval becomes
// the folded value and (xi, subgroup_x) move to the next layer's domain.
LCP2_HD bool vq_fold_layer(const VqLayout &V, const VqChallenge &c, const u64 *R, u32 l, u64 &xi, u64 &subgroup_x, gl2 &eval) {
  const u32 ab = V.arity_bits[l];
  const u64 *evals = R + V.tree[4 + l].leaf_off;
  const u32 within = (u32)xi & ((1u << ab) - 1);
  if (!gl2_eq(vq_rd2(evals + 2 * within), eval)) return false;
  eval = vq_compute_evaluation(subgroup_x, within, ab, evals, c.fri_betas[l]);
  for (u32 i = 0; i < ab; i++) subgroup_x = gl_sqr(subgroup_x);
  xi >>= ab;
  return true;
}
LCP2_HD bool vq_final_poly_holds(const VqLayout &V, const u64 *final_poly, u64 subgroup_x, gl2 eval) {
  gl2 fv = gl2_make(0, 0);
  for (u32 j = V.final_len; j-- > 0;) fv = gl2_add(gl2_mul(fv, gl2_make(subgroup_x, 0)), vq_rd2(final_poly + 2 * j));
  return gl2_eq(fv, eval);
}
// Query q of a proof without its Merkle paths: VQ_STATUS_NONE, or the first of its consistency checks / its final-polynomial check
// that fails.  final_poly: the proof's final polynomial (proof + V.final_poly).
LCP2_HD u32 vq_fri_query(const VqLayout &V, const VqChallenge &c, const u64 *proof, const u64 *final_poly, u32 q) {
  const u64 *R = proof + V.queries + (u64)q * V.query_words;
  u64 xi = c.x_index[q], subgroup_x = vq_subgroup_x(V, c.x_index[q]);
  gl2 eval = vq_combine_initial(V, c, R, subgroup_x);
  for (u32 l = 0; l < V.num_layers; l++)
    if (!vq_fold_layer(V, c, R, l, xi, subgroup_x, eval)) return vq_status(vq_ord_consistency(l), VQ_CHECK_CONSISTENCY);
  return vq_final_poly_holds(V, final_poly, subgroup_x, eval) ? VQ_STATUS_NONE : vq_status(vq_ord_final(V.num_layers), VQ_CHECK_FINAL_POLY);
}

}  // namespace lcp2
