// The head of data.verify(proof): public-input hash, transcript (plonky2 plonk/get_challenges.rs), proof of work, the vanishing
// identity at zeta (plonk/vanishing_poly.rs eval_vanishing_poly) and the reduced openings of the FRI verifier.  Host text, shared by
// lcp2_verify (verifier.hip), lcp2_verify_batch (verify_batch.hip) and the CPU harness tests/emu/emu_verify.cpp.
#pragma once
#include <vector>
#include "gate_program.hpp"
#include "host_protocol.hpp"

namespace lcp2 {
inline gl2 rd2(const u64 *p) { return gl2_make(p[0], p[1]); }
inline gl2 base2(u64 x) { return gl2_make(x, 0); }

// gate programs over the extension field (evaluation at zeta): the algebra gate_program.hpp walks them with.  mul_add and scale_add
// are a multiplication and an addition here (the field element is the same either way; over targets they are one gate)
struct ZetaAlg {
  using V = gl2; using S = u64;
  const gl2 *wires, *consts; const u64 *pis; u32 num_selectors;
  V wire(u32 i) { return wires[i]; }    V selector(u32 i) { return consts[i]; }    V gate_const(u32 i) { return consts[num_selectors + i]; }
  V imm(u64 x) { return base2(x); }     V pi(u32 i) { return base2(pis[i]); }
  S scalar(u64 x) { return x; }         S scalar_mul(S a, S b) { return gl_mul(a, b); }
  V add(V a, V b) { return gl2_add(a, b); }    V sub(V a, V b) { return gl2_sub(a, b); }    V mul(V a, V b) { return gl2_mul(a, b); }
  V mul_add(V a, V b, V acc) { return gl2_add(acc, gl2_mul(a, b)); }
  V scale_add(V x, S s, V acc) { return gl2_add(acc, gl2_scale(x, s)); }
};

// Checks 2 and 3 of data.verify(proof) and everything its query phase needs, from the words of a proof OUTSIDE its query section:
// proof = the words [0, L.queries) (nothing at or beyond L.queries is read through it), tail = the words [L.final_poly, L.total)
// (final polynomial, PoW witness).  Returns 0, 2 or 3; on 0 `out` holds the challenges, the reduced openings and the query indices.
// Every word must be canonical (check 1 comes first).
inline int verify_head(const VerifierView &v, const ProofLayout &L, const u64 *proof, const u64 *tail, const u64 *pis_in, VqChallenge &out) {
  const lcp2_params &p = *v.p;
  const u64 n = 1ull << p.degree_bits, N = n << p.rate_bits;
  const u32 W = p.num_wires, NR = p.num_routed_wires, NC = p.num_constants, CH = p.num_challenges, Q = p.quotient_degree_factor;
  const u32 nchunks = (NR + Q - 1) / Q, npp = nchunks - 1;
  const HostPoseidon &H = HostPoseidon::get();
  std::vector<u64> pis(std::max<u32>(v.npi, 1), 0);
  for (u32 i = 0; i < v.npi; i++) pis[i] = gl_canon(pis_in[i]);
  u64 pi_hash[4];
  H.hash_no_pad(pis.data(), v.npi, pi_hash);

  // ---- get_challenges
  HostChallenger ch;
  ch.observe_n(v.digest, 4);
  ch.observe_n(pi_hash, 4);
  ch.observe_n(proof + L.wires_cap, L.capw);
  u64 betas[4], gammas[4], alphas[4];
  for (u32 k = 0; k < CH; k++) betas[k] = ch.get();
  for (u32 k = 0; k < CH; k++) gammas[k] = ch.get();
  ch.observe_n(proof + L.zs_cap, L.capw);
  for (u32 k = 0; k < CH; k++) alphas[k] = ch.get();
  ch.observe_n(proof + L.quot_cap, L.capw);
  const gl2 zeta = ch.get_ext();
  ch.observe_n(proof + L.op_constants, 2 * (NC + NR + W));
  ch.observe_n(proof + L.op_zs, 2 * CH);
  ch.observe_n(proof + L.op_pp, 2 * CH * npp);
  ch.observe_n(proof + L.op_quot, 2 * CH * Q);
  ch.observe_n(proof + L.op_zs_next, 2 * CH);
  const gl2 fri_alpha = ch.get_ext();
  gl2 fri_betas[LCP2_MAX_FRI_LAYERS];
  for (u32 l = 0; l < p.num_fri_layers; l++) { ch.observe_n(proof + L.fri_caps + l * L.capw, L.capw); fri_betas[l] = ch.get_ext(); }
  ch.observe_n(tail, 2 * L.final_len);
  ch.observe(tail[L.pow_witness - L.final_poly]);
  if ((ch.get() >> (64 - p.proof_of_work_bits)) != 0) return 2;

  // ---- vanishing(zeta) = Z_H(zeta) * t(zeta)
  std::vector<gl2> ow(W), oc(NC + NR);
  for (u32 j = 0; j < W; j++) ow[j] = rd2(proof + L.op_wires + 2 * j);
  for (u32 j = 0; j < NC + NR; j++) oc[j] = rd2(proof + L.op_constants + 2 * j);
  gl2 zeta_n = zeta;
  for (u32 i = 0; i < p.degree_bits; i++) zeta_n = gl2_mul(zeta_n, zeta_n);
  const gl2 one = base2(1);
  const gl2 zh = gl2_sub(zeta_n, one);
  {
    const gl2 l0 = gl2_eq(zeta, one) ? one : gl2_mul(zh, gl2_inv(gl2_scale(gl2_sub(zeta, one), n % GL_P)));
    std::vector<gl2> terms;
    for (u32 k = 0; k < CH; k++) terms.push_back(gl2_mul(l0, gl2_sub(rd2(proof + L.op_zs + 2 * k), one)));
    for (u32 k = 0; k < CH; k++) {
      gl2 prev = rd2(proof + L.op_zs + 2 * k);
      for (u32 c = 0; c < nchunks; c++) {
        gl2 pn = one, pd = one;
        for (u32 j = c * Q; j < NR && j < (c + 1) * Q; j++) {
          pn = gl2_mul(pn, gl2_add_base(gl2_add(ow[j], gl2_scale(gl2_scale(zeta, v.k_is[j]), betas[k])), gammas[k]));
          pd = gl2_mul(pd, gl2_add_base(gl2_add(ow[j], gl2_scale(oc[NC + j], betas[k])), gammas[k]));
        }
        gl2 next = c < npp ? rd2(proof + L.op_pp + 2 * (k * npp + c)) : rd2(proof + L.op_zs_next + 2 * k);
        terms.push_back(gl2_sub(gl2_mul(prev, pn), gl2_mul(next, pd)));
        prev = next;
      }
    }
    gl2 gates[4];
    ZetaAlg at_zeta{ow.data(), oc.data(), pi_hash, v.num_selectors};
    gate_program::eval_gates_filtered(at_zeta, v.gates, v.num_gates, v.code, v.imm, v.num_selectors, alphas, CH, gates);
    for (u32 k = 0; k < CH; k++) {
      gl2 acc = gates[k];
      for (size_t t = terms.size(); t-- > 0;) acc = gl2_add(gl2_scale(acc, alphas[k]), terms[t]);
      gl2 tq = base2(0);
      for (u32 j = Q; j-- > 0;) tq = gl2_add(gl2_mul(tq, zeta_n), rd2(proof + L.op_quot + 2 * (k * Q + j)));
      if (!gl2_eq(acc, gl2_mul(zh, tq))) return 3;
    }
  }
  // ---- FRI
  gl2 red0 = base2(0), red1 = base2(0);
  {
    std::vector<gl2> vals;
    for (u32 j = 0; j < NC + NR + W; j++) vals.push_back(rd2(proof + L.op_constants + 2 * j));
    for (u32 j = 0; j < CH; j++) vals.push_back(rd2(proof + L.op_zs + 2 * j));
    for (u32 j = 0; j < CH * npp; j++) vals.push_back(rd2(proof + L.op_pp + 2 * j));
    for (u32 j = 0; j < CH * Q; j++) vals.push_back(rd2(proof + L.op_quot + 2 * j));
    for (size_t j = vals.size(); j-- > 0;) red0 = gl2_add(gl2_mul(red0, fri_alpha), vals[j]);
    for (u32 j = CH; j-- > 0;) red1 = gl2_add(gl2_mul(red1, fri_alpha), rd2(proof + L.op_zs_next + 2 * j));
  }
  out.zeta = zeta; out.g_zeta = gl2_scale(zeta, gl_root_of_unity(p.degree_bits));
  out.fri_alpha = fri_alpha; out.alpha_ch = gl2_pow(fri_alpha, CH);
  out.red0 = red0; out.red1 = red1;
  for (u32 l = 0; l < LCP2_MAX_FRI_LAYERS; l++) out.fri_betas[l] = l < p.num_fri_layers ? fri_betas[l] : base2(0);
  for (u32 q = 0; q < VQ_MAX_QUERIES; q++) out.x_index[q] = q < p.num_query_rounds ? (u32)(ch.get() % N) : 0;
  out.live = 1; out.pad = 0;
  return 0;
}

}  // namespace lcp2
