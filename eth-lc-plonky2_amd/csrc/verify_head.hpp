// The head of data.verify(proof): public-input hash, transcript (plonky2 plonk/get_challenges.rs), proof of work, the vanishing
// identity at zeta (plonk/vanishing_poly.rs eval_vanishing_poly) and the reduced openings of the FRI verifier - as portable text, the
// way verify_query.hpp holds the query phase: what verify_head() below runs on one host thread for lcp2_verify (verifier.hip) and
// for lcp2_verify_batch with the host head (verify_batch.hip), what the kernels of kernels_verify_head.hip run for the device head,
// and what tests/emu/emu_verify_head.cpp runs on the CPU in the kernels' decomposition:
//   head_transcript   one sponge per proof (host: the one-lane permutation; device: a 16-lane group, state word j in lane j)
//   head_gate_slot    one gate's filtered constraint sums under every alpha, from the openings of one proof
//   head_terms        the L_0 and permutation terms under every alpha
//   head_finish       sums and terms against Z_H(zeta) t(zeta), reduced openings, the rest of the challenge block
// The arithmetic is exact, so the host's single Horner chain over (terms, gates) is regrouped here:  for challenge k and nt terms
//   sum_t alpha^t term_t + alpha^nt sum_g filter_g sum_i alpha^i c_{g,i}.
// A proof is read only through HeadLayout (offsets and counts of the circuit, none taken from the proof).
#pragma once
#include <vector>
#include "gate_program.hpp"
#include "host_protocol.hpp"

namespace lcp2 {
LCP2_HD gl2 rd2(const u64 *p) { return gl2_make(p[0], p[1]); }
LCP2_HD gl2 base2(u64 x) { return gl2_make(x, 0); }

constexpr u32 HEAD_MAX_CHALLENGES = gate_program::MAX_CHALLENGES;

// the circuit's ProofLayout outside the query section, and its shape, in words a kernel takes by value
struct HeadLayout {
  u64 final_poly, pow_witness;
  u32 degree_bits, lgN, W, NR, NC, CH, Q, nchunks, npp, num_layers, num_queries, pow_bits, npi, capw, final_len;
  u32 num_selectors, num_gates, num_regs;
  u32 wires_cap, zs_cap, quot_cap, op_constants, op_wires, op_zs, op_zs_next, op_pp, op_quot, fri_caps;
};
// num_regs: the registers head_gate_slot clears before a gate's program runs (the circuit's; the host passes its whole file)
inline HeadLayout head_make_layout(const VerifierView &v, const ProofLayout &L, u32 num_regs) {
  const lcp2_params &p = *v.p;
  HeadLayout H = {};
  H.final_poly = L.final_poly; H.pow_witness = L.pow_witness;
  H.degree_bits = p.degree_bits; H.lgN = p.degree_bits + p.rate_bits; H.W = p.num_wires; H.NR = p.num_routed_wires; H.NC = p.num_constants;
  H.CH = p.num_challenges; H.Q = p.quotient_degree_factor; H.nchunks = (H.NR + H.Q - 1) / H.Q; H.npp = H.nchunks - 1;
  H.num_layers = p.num_fri_layers; H.num_queries = p.num_query_rounds; H.pow_bits = p.proof_of_work_bits; H.npi = v.npi;
  H.capw = (u32)L.capw; H.final_len = (u32)L.final_len;
  H.num_selectors = v.num_selectors; H.num_gates = v.num_gates; H.num_regs = num_regs;
  H.wires_cap = (u32)L.wires_cap; H.zs_cap = (u32)L.zs_cap; H.quot_cap = (u32)L.quot_cap; H.op_constants = (u32)L.op_constants;
  H.op_wires = (u32)L.op_wires; H.op_zs = (u32)L.op_zs; H.op_zs_next = (u32)L.op_zs_next; H.op_pp = (u32)L.op_pp; H.op_quot = (u32)L.op_quot;
  H.fri_caps = (u32)L.fri_caps;
  return H;
}

// what the transcript leaves for the identity besides the challenge block: one per proof
struct HeadChallenges {
  u64 pi_hash[4], betas[HEAD_MAX_CHALLENGES], gammas[HEAD_MAX_CHALLENGES], alphas[HEAD_MAX_CHALLENGES];
};
// per proof: (num_gates + 1) slots of HEAD_MAX_CHALLENGES sums each; slot g < num_gates is gate g's, slot num_gates the terms'
LCP2_HD u64 head_part_index(const HeadLayout &H, u64 proof, u32 slot) { return (proof * (H.num_gates + 1) + slot) * HEAD_MAX_CHALLENGES; }

// ---- transcript.  A sponge provider Sp holds one Poseidon state and up to 8 staged input words:
//   reset()                 the zero state
//   stage(x, at, k)         staged words at .. at + k - 1 <- gl_canon(x[0 .. k - 1])          (at + k <= 8)
//   stage_value(at, v)      staged word at <- v (canonical, known to every lane)
//   duplex(m)               state words 0 .. m - 1 <- the staged words, then one permutation   (overwrite mode)
//   word(j)                 state word j
//   writer()                whether this lane stores results (every lane computes the same ones)
// The one-lane provider of the host:
struct OneLaneSponge {
  const u64 *rc;  // the 360 round constants
  u64 s[12], in[8];
  void reset() { for (u64 &w : s) w = 0; }
  void stage(const u64 *x, u32 at, u32 k) { for (u32 i = 0; i < k; i++) in[at + i] = gl_canon(x[i]); }
  void stage_value(u32 at, u64 v) { in[at] = v; }
  void duplex(u32 m) { for (u32 i = 0; i < m; i++) s[i] = in[i]; pos_permute(s, rc); }
  u64 word(u32 j) const { return s[j]; }
  bool writer() const { return true; }
};
// Challenger<F, PoseidonHash> (iop/challenger.rs) over a provider: rate 8, challenges popped from the back of the output
template <class Sp>
struct HeadChallenger {
  Sp &sp;
  u32 nin, nout;
  LCP2_HD void duplex() { sp.duplex(nin); nin = 0; nout = 8; }
  LCP2_HD void observe_n(const u64 *x, u32 n) {
    while (n) {
      const u32 k = n < 8 - nin ? n : 8 - nin;
      sp.stage(x, nin, k);
      nin += k; x += k; n -= k; nout = 0;
      if (nin == 8) duplex();
    }
  }
  LCP2_HD void observe_value(u64 v) {
    sp.stage_value(nin, v);
    nin++; nout = 0;
    if (nin == 8) duplex();
  }
  LCP2_HD u64 get() {
    if (nin || !nout) duplex();
    return sp.word(--nout);
  }
  LCP2_HD gl2 get_ext() { const u64 a = get(), b = get(); return gl2_make(a, b); }
};
LCP2_HD bool head_pow_fails(u64 response, u32 pow_bits) { return (response >> (64 - pow_bits)) != 0; }

// hash_no_pad of the canonicalised public inputs, then the observe / get sequence of get_challenges in its order, the proof-of-work
// test and the query indices.  proof: the words [0, queries) of a proof, tail: its words [final_poly, total).  Returns 0 or 2; on 0
// hc is complete and out holds zeta, fri_alpha, fri_betas and x_index (every index below N).
template <class Sp>
LCP2_HD int head_transcript(Sp &sp, const HeadLayout &H, const u64 *proof, const u64 *tail, const u64 *pis, const u64 *digest, HeadChallenges &hc,
                            VqChallenge &out) {
  sp.reset();
  for (u32 off = 0; off < H.npi; off += 8) {
    const u32 c = H.npi - off < 8 ? H.npi - off : 8;
    sp.stage(pis + off, 0, c);
    sp.duplex(c);
  }
  u64 h[4];
#pragma unroll
  for (u32 i = 0; i < 4; i++) h[i] = sp.word(i);
  if (sp.writer())
    for (u32 i = 0; i < 4; i++) hc.pi_hash[i] = h[i];
  sp.reset();
  HeadChallenger<Sp> ch{sp, 0, 0};
  ch.observe_n(digest, 4);
#pragma unroll
  for (u32 i = 0; i < 4; i++) ch.observe_value(h[i]);
  ch.observe_n(proof + H.wires_cap, H.capw);
  for (u32 k = 0; k < H.CH; k++) { const u64 b = ch.get(); if (sp.writer()) hc.betas[k] = b; }
  for (u32 k = 0; k < H.CH; k++) { const u64 g = ch.get(); if (sp.writer()) hc.gammas[k] = g; }
  ch.observe_n(proof + H.zs_cap, H.capw);
  for (u32 k = 0; k < H.CH; k++) { const u64 a = ch.get(); if (sp.writer()) hc.alphas[k] = a; }
  ch.observe_n(proof + H.quot_cap, H.capw);
  const gl2 zeta = ch.get_ext();
  ch.observe_n(proof + H.op_constants, 2 * (H.NC + H.NR + H.W));
  ch.observe_n(proof + H.op_zs, 2 * H.CH);
  ch.observe_n(proof + H.op_pp, 2 * H.CH * H.npp);
  ch.observe_n(proof + H.op_quot, 2 * H.CH * H.Q);
  ch.observe_n(proof + H.op_zs_next, 2 * H.CH);
  const gl2 fri_alpha = ch.get_ext();
  if (sp.writer()) { out.zeta = zeta; out.fri_alpha = fri_alpha; }
  for (u32 l = 0; l < LCP2_MAX_FRI_LAYERS; l++) {
    gl2 beta = base2(0);
    if (l < H.num_layers) { ch.observe_n(proof + H.fri_caps + l * H.capw, H.capw); beta = ch.get_ext(); }
    if (sp.writer()) out.fri_betas[l] = beta;
  }
  ch.observe_n(tail, 2 * H.final_len);
  ch.observe_n(tail + (H.pow_witness - H.final_poly), 1);
  if (head_pow_fails(ch.get(), H.pow_bits)) return 2;
  const u64 N = 1ull << H.lgN;
  for (u32 q = 0; q < VQ_MAX_QUERIES; q++) {
    const u32 x = q < H.num_queries ? (u32)(ch.get() % N) : 0;
    if (sp.writer()) out.x_index[q] = x;
  }
  return 0;
}

// ---- identity.  Gate programs over the extension field (evaluation at zeta): the algebra gate_program.hpp walks them with, on the
// openings where they lie in the proof.  mul_add and scale_add are a multiplication and an addition here (the field element is the
// same either way; over targets they are one gate)
struct ZetaAlg {
  using V = gl2; using S = u64;
  const u64 *wires, *consts, *pis; u32 num_selectors;  // op_wires, op_constants of the proof; the public-input hash
  LCP2_HD V wire(u32 i) { return rd2(wires + 2 * i); }
  LCP2_HD V selector(u32 i) { return rd2(consts + 2 * i); }
  LCP2_HD V gate_const(u32 i) { return rd2(consts + 2 * (num_selectors + i)); }
  LCP2_HD V imm(u64 x) { return base2(x); }
  LCP2_HD V pi(u32 i) { return base2(pis[i]); }
  LCP2_HD S scalar(u64 x) { return x; }
  LCP2_HD S scalar_mul(S a, S b) { return gl_mul(a, b); }
  LCP2_HD V add(V a, V b) { return gl2_add(a, b); }
  LCP2_HD V sub(V a, V b) { return gl2_sub(a, b); }
  LCP2_HD V mul(V a, V b) { return gl2_mul(a, b); }
  LCP2_HD V mul_add(V a, V b, V acc) { return gl2_add(acc, gl2_mul(a, b)); }
  LCP2_HD V scale_add(V x, S s, V acc) { return gl2_add(acc, gl2_scale(x, s)); }
};

// out[k] = filter_g(zeta) * sum_i alphas[k]^i c_i  for gate G, k < CH: what gate_program::eval_gates_filtered adds for this gate.
// regs: H.num_regs registers (operator[] gives a gl2 &), cleared here.  The loops over k are unrolled to HEAD_MAX_CHALLENGES so that
// the sums stay in registers on the device.
template <class Regs>
LCP2_HD void head_gate_slot(const HeadLayout &H, const lcp2_gate &G, const uint32_t *code, const u64 *imm, const u64 *proof, const HeadChallenges &hc,
                            Regs regs, gl2 *out) {
  ZetaAlg A{proof + H.op_wires, proof + H.op_constants, hc.pi_hash, H.num_selectors};
  for (u32 r = 0; r < H.num_regs; r++) regs[r] = base2(0);
  const bool fwd = (G.flags & LCP2_GATE_EMIT_FORWARD) != 0;
  const u32 CH = H.CH;
  gl2 acc[HEAD_MAX_CHALLENGES];
  u64 apow[HEAD_MAX_CHALLENGES], alpha[HEAD_MAX_CHALLENGES];
#pragma unroll
  for (u32 k = 0; k < HEAD_MAX_CHALLENGES; k++) { acc[k] = base2(0); apow[k] = 1; alpha[k] = k < CH ? hc.alphas[k] : 0; }
  gate_program::walk_program(A, code, G.code_offset, G.code_len, imm, regs, [&](const gl2 &a) {
#pragma unroll
    for (u32 k = 0; k < HEAD_MAX_CHALLENGES; k++) {
      if (k >= CH) continue;
      if (fwd) { acc[k] = A.scale_add(a, apow[k], acc[k]); apow[k] = A.scalar_mul(apow[k], alpha[k]); }
      else acc[k] = A.scale_add(acc[k], alpha[k], a);
    }
  });
  const gl2 s = A.selector(G.selector_index);
  gl2 f = base2(1);
  for (u32 j = G.group_start; j < G.group_end; j++)
    if (j != G.selector_value) f = gl2_mul(f, gl2_sub(base2(j), s));
  if (H.num_selectors > 1) f = gl2_mul(f, gl2_sub(base2(gate_program::UNUSED_SELECTOR), s));
#pragma unroll
  for (u32 k = 0; k < HEAD_MAX_CHALLENGES; k++)
    if (k < CH) out[k] = gl2_mul(f, acc[k]);
}

LCP2_HD gl2 head_zeta_n(const HeadLayout &H, gl2 zeta) {
  gl2 zeta_n = zeta;
  for (u32 i = 0; i < H.degree_bits; i++) zeta_n = gl2_mul(zeta_n, zeta_n);
  return zeta_n;
}
LCP2_HD u32 head_num_terms(const HeadLayout &H) { return H.CH + H.CH * H.nchunks; }

// out[k] = sum_t alphas[k]^t term_t, k < CH, over the terms of eval_vanishing_poly in its order: L_0(zeta) (Z_c(zeta) - 1) for every
// challenge c, then per challenge the chunked permutation products.  k_is: the circuit's coset shifts.
LCP2_HD void head_terms(const HeadLayout &H, const u64 *proof, const u64 *k_is, const HeadChallenges &hc, gl2 zeta, gl2 *out) {
  const u32 CH = H.CH;
  const u64 n = 1ull << H.degree_bits;
  const gl2 one = base2(1);
  const gl2 zh = gl2_sub(head_zeta_n(H, zeta), one);
  const gl2 l0 = gl2_eq(zeta, one) ? one : gl2_mul(zh, gl2_inv(gl2_scale(gl2_sub(zeta, one), n % GL_P)));
  gl2 sum[HEAD_MAX_CHALLENGES];
  u64 apow[HEAD_MAX_CHALLENGES], alpha[HEAD_MAX_CHALLENGES];
#pragma unroll
  for (u32 k = 0; k < HEAD_MAX_CHALLENGES; k++) { sum[k] = base2(0); apow[k] = 1; alpha[k] = k < CH ? hc.alphas[k] : 0; }
  auto term = [&](gl2 t) {
#pragma unroll
    for (u32 k = 0; k < HEAD_MAX_CHALLENGES; k++) {
      if (k >= CH) continue;
      sum[k] = gl2_add(sum[k], gl2_scale(t, apow[k]));
      apow[k] = gl_mul(apow[k], alpha[k]);
    }
  };
  for (u32 c = 0; c < CH; c++) term(gl2_mul(l0, gl2_sub(rd2(proof + H.op_zs + 2 * c), one)));
  for (u32 c = 0; c < CH; c++) {
    const u64 beta = hc.betas[c], gamma = hc.gammas[c];
    gl2 prev = rd2(proof + H.op_zs + 2 * c);
    for (u32 chunk = 0; chunk < H.nchunks; chunk++) {
      gl2 pn = one, pd = one;
      for (u32 j = chunk * H.Q; j < H.NR && j < (chunk + 1) * H.Q; j++) {
        const gl2 w = rd2(proof + H.op_wires + 2 * j), sigma = rd2(proof + H.op_constants + 2 * (H.NC + j));
        pn = gl2_mul(pn, gl2_add_base(gl2_add(w, gl2_scale(gl2_scale(zeta, k_is[j]), beta)), gamma));
        pd = gl2_mul(pd, gl2_add_base(gl2_add(w, gl2_scale(sigma, beta)), gamma));
      }
      const gl2 next = chunk < H.npp ? rd2(proof + H.op_pp + 2 * (c * H.npp + chunk)) : rd2(proof + H.op_zs_next + 2 * c);
      term(gl2_sub(gl2_mul(prev, pn), gl2_mul(next, pd)));
      prev = next;
    }
  }
#pragma unroll
  for (u32 k = 0; k < HEAD_MAX_CHALLENGES; k++)
    if (k < CH) out[k] = sum[k];
}

// acc <- acc * x + v over the extension elements words[2 * (count - 1)], ..., words[0]
LCP2_HD gl2 head_horner_down(gl2 acc, gl2 x, const u64 *words, u32 count) {
  for (u32 j = count; j-- > 0;) acc = gl2_add(gl2_mul(acc, x), rd2(words + 2 * j));
  return acc;
}
// The identity and the rest of the challenge block from the sums of one proof (parts: its (num_gates + 1) slots, head_part_index)
// and out.zeta, out.fri_alpha as head_transcript left them.  Returns 0 or 3; on 0 out is complete and live.
LCP2_HD int head_finish(const HeadLayout &H, const u64 *proof, const HeadChallenges &hc, const gl2 *parts, VqChallenge &out) {
  const gl2 zeta = out.zeta, fri_alpha = out.fri_alpha;
  const gl2 zeta_n = head_zeta_n(H, zeta), zh = gl2_sub(zeta_n, base2(1));
  const u32 nt = head_num_terms(H);
  for (u32 k = 0; k < H.CH; k++) {
    gl2 gates = base2(0);
    for (u32 g = 0; g < H.num_gates; g++) gates = gl2_add(gates, parts[g * HEAD_MAX_CHALLENGES + k]);
    const gl2 acc = gl2_add(gl2_scale(gates, gl_pow(hc.alphas[k], nt)), parts[H.num_gates * HEAD_MAX_CHALLENGES + k]);
    const gl2 tq = head_horner_down(base2(0), zeta_n, proof + H.op_quot + 2 * k * H.Q, H.Q);
    if (!gl2_eq(acc, gl2_mul(zh, tq))) return 3;
  }
  // fri/verifier.rs: the openings at zeta reduced under alpha in the order constants, sigmas, wires, zs, partial products, quotient
  gl2 red0 = head_horner_down(base2(0), fri_alpha, proof + H.op_quot, H.CH * H.Q);
  red0 = head_horner_down(red0, fri_alpha, proof + H.op_pp, H.CH * H.npp);
  red0 = head_horner_down(red0, fri_alpha, proof + H.op_zs, H.CH);
  red0 = head_horner_down(red0, fri_alpha, proof + H.op_constants, H.NC + H.NR + H.W);
  out.red0 = red0;
  out.red1 = head_horner_down(base2(0), fri_alpha, proof + H.op_zs_next, H.CH);
  out.g_zeta = gl2_scale(zeta, gl_root_of_unity(H.degree_bits));
  out.alpha_ch = gl2_pow(fri_alpha, H.CH);
  out.live = 1; out.pad = 0;
  return 0;
}

// ---- the host's head: the four parts above on one thread.
// Checks 2 and 3 of data.verify(proof) and everything its query phase needs, from the words of a proof OUTSIDE its query section:
// proof = the words [0, L.queries) (nothing at or beyond L.queries is read through it), tail = the words [L.final_poly, L.total)
// (final polynomial, PoW witness).  Returns 0, 2 or 3; on 0 `out` holds the challenges, the reduced openings and the query indices.
// Every word must be canonical (check 1 comes first).
inline int verify_head(const VerifierView &v, const ProofLayout &L, const u64 *proof, const u64 *tail, const u64 *pis_in, VqChallenge &out) {
  const HeadLayout H = head_make_layout(v, L, gate_program::MAX_REGS);
  OneLaneSponge sp;
  sp.rc = HostPoseidon::get().round_constants();
  HeadChallenges hc = {};
  if (const int rc = head_transcript(sp, H, proof, tail, pis_in, v.digest, hc, out)) return rc;
  std::vector<gl2> parts((size_t)(v.num_gates + 1) * HEAD_MAX_CHALLENGES, base2(0));
  gl2 regs[gate_program::MAX_REGS];
  for (u32 g = 0; g < v.num_gates; g++) head_gate_slot(H, v.gates[g], v.code, v.imm, proof, hc, regs, &parts[(size_t)g * HEAD_MAX_CHALLENGES]);
  head_terms(H, proof, v.k_is, hc, out.zeta, &parts[(size_t)v.num_gates * HEAD_MAX_CHALLENGES]);
  return head_finish(H, proof, hc, parts.data(), out);
}

}  // namespace lcp2
