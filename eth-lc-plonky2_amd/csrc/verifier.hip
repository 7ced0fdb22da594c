// data.verify(proof): host-only verifier (reference call site eth-lc-plonky2/src/main.rs:233,
// src/unit_tests.rs:34).  Restates plonky2 0.1.4 plonk/verifier.rs::verify_with_challenges,
// plonk/vanishing_poly.rs::eval_vanishing_poly, plonk/get_challenges.rs and fri/verifier.rs
// (verify_fri_proof, fri_combine_initial, compute_evaluation).  Milliseconds of scalar work: it stays
// on the host exactly as in the reference; no device call is made here.
#include <vector>
#include "internal.hpp"
#include "verify_head.hpp"

namespace lcp2 {
VerifierView verifier_view(const lcp2_circuit *c);
}
using namespace lcp2;

namespace {
// the queries one after another, each check where plonky2's verifier meets it (verify_query.hpp holds the text of every step)
int verify_impl(const VerifierView &v, const u64 *proof, const u64 *pis_in) {
  const lcp2_params &p = *v.p;
  const ProofLayout L(p);
  const HostPoseidon &H = HostPoseidon::get();
  for (size_t i = 0; i < L.total; i++)
    if (proof[i] >= GL_P) return 1;
  VqChallenge c;
  if (const int rc = verify_head(v, L, proof, proof + L.final_poly, pis_in, c)) return rc;
  const VqLayout V = vq_make_layout(L, p);
  const u64 *caps[4] = {v.cs_cap, proof + L.wires_cap, proof + L.zs_cap, proof + L.quot_cap};
  for (u32 q = 0; q < p.num_query_rounds; q++) {
    const u64 x_index = c.x_index[q];
    const u64 *R = proof + L.queries + (size_t)q * L.query_words;
    for (int o = 0; o < 4; o++)
      if (!H.merkle_verify(R + L.q_init_off[o], L.q_init_cols[o], x_index, R + L.q_init_off[o] + L.q_init_cols[o], (u32)L.q_init_sib, caps[o]))
        return 4;
    u64 subgroup_x = vq_subgroup_x(V, (u32)x_index), xi = x_index;
    gl2 eval = vq_combine_initial(V, c, R, subgroup_x);
    for (u32 l = 0; l < p.num_fri_layers; l++) {
      const u32 arity = 1u << p.fri_arity_bits[l];
      if (!vq_fold_layer(V, c, R, l, xi, subgroup_x, eval)) return 5;  // xi is the coset index from here on
      if (!H.merkle_verify(R + L.q_step_off[l], 2 * arity, xi, R + L.q_step_off[l] + 2 * arity, (u32)L.q_step_sib[l],
                           proof + L.fri_caps + l * L.capw))
        return 6;
    }
    if (!vq_final_poly_holds(V, proof + L.final_poly, subgroup_x, eval)) return 7;
  }
  return 0;
}
}  // namespace

extern "C" int lcp2_verify(const lcp2_circuit *c, const uint64_t *proof, size_t proof_words, const uint64_t *public_inputs,
                           size_t num_public_inputs, int *failed_check) {
  if (!c || !proof) return LCP2_E_INVALID;
  VerifierView v = verifier_view(c);
  if (v.npi && !public_inputs) return LCP2_E_INVALID;
  // an untrusted proof is only ever read through the layout of THIS circuit: refuse any other length up front
  if (proof_words != ProofLayout(*v.p).total || num_public_inputs != v.npi) return LCP2_E_INVALID;
  int rc = verify_impl(v, (const u64 *)proof, (const u64 *)public_inputs);
  if (failed_check) *failed_check = rc;
  return rc == 0 ? LCP2_OK : LCP2_E_VERIFY;
}

// ------------------------------------------------------------------ proof <-> bytes (plonky2 util/serialization.rs, [RECALL])
namespace {
// walks the flat proof in field order; `word` sees every field element slot, `count` every MerkleProof sibling-count byte
template <class Word, class Count>
bool walk_proof(const lcp2_params &p, Word &&word, Count &&count) {
  const ProofLayout L(p);
  const size_t CH = p.num_challenges, NR = p.num_routed_wires, NC = p.num_constants, W = p.num_wires, Q = p.quotient_degree_factor;
  const size_t npp = (NR + Q - 1) / Q - 1;
  auto run = [&](size_t off, size_t n) { for (size_t i = 0; i < n; i++) if (!word(off + i)) return false; return true; };
  if (!run(L.wires_cap, 3 * L.capw)) return false;
  // OpeningSet: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next, partial_products, quotient_polys (the flat layout's order)
  if (!run(L.op_constants, 2 * (NC + NR + W)) || !run(L.op_zs, 2 * CH) || !run(L.op_zs_next, 2 * CH) || !run(L.op_pp, 2 * CH * npp) || !run(L.op_quot, 2 * CH * Q)) return false;
  if (!run(L.fri_caps, p.num_fri_layers * L.capw)) return false;
  for (u32 q = 0; q < p.num_query_rounds; q++) {
    const size_t R = L.queries + (size_t)q * L.query_words;
    for (int o = 0; o < 4; o++) {
      if (!run(R + L.q_init_off[o], L.q_init_cols[o])) return false;
      if (!count(L.q_init_sib)) return false;
      if (!run(R + L.q_init_off[o] + L.q_init_cols[o], 4 * L.q_init_sib)) return false;
    }
    for (u32 l = 0; l < p.num_fri_layers; l++) {
      const size_t ev = (size_t)2 << p.fri_arity_bits[l];
      if (!run(R + L.q_step_off[l], ev)) return false;
      if (!count(L.q_step_sib[l])) return false;
      if (!run(R + L.q_step_off[l] + ev, 4 * L.q_step_sib[l])) return false;
    }
  }
  return run(L.final_poly, 2 * L.final_len) && run(L.pow_witness, 1);
}
// the full shape check of build(): ProofLayout subtracts the FRI arities from the LDE height in unsigned arithmetic, so a schedule that
// does not fit (a single arity of 31, a sum above degree_bits) must be refused before any layout is computed
bool params_ok(const lcp2_params *p) {
  bool unsupported;
  return p && !params_problem(*p, &unsupported) && p->degree_bits >= 1 && p->degree_bits + p->rate_bits <= 30 && p->cap_height <= p->degree_bits + p->rate_bits &&
         p->num_fri_layers <= LCP2_MAX_FRI_LAYERS && p->num_query_rounds <= 64 && p->quotient_degree_factor >= 1 && p->num_routed_wires >= 1 &&
         p->num_routed_wires <= p->num_wires && p->num_wires <= 65535 && p->num_constants <= 65535 && p->num_challenges >= 1 && p->num_challenges <= 4;
}
inline void put64(uint8_t *o, u64 v) { for (int i = 0; i < 8; i++) o[i] = (uint8_t)(v >> (8 * i)); }
inline u64 get64(const uint8_t *o) { u64 v = 0; for (int i = 0; i < 8; i++) v |= (u64)o[i] << (8 * i); return v; }
}  // namespace

extern "C" int lcp2_proof_layout_of(const lcp2_params *p, lcp2_proof_layout *o) {
  if (!params_ok(p) || !o) return LCP2_E_INVALID;
  const ProofLayout L(*p);
  memset(o, 0, sizeof *o);
  o->cap_words = L.capw; o->wires_cap = L.wires_cap; o->zs_cap = L.zs_cap; o->quot_cap = L.quot_cap;
  o->op_constants = L.op_constants; o->op_sigmas = L.op_sigmas; o->op_wires = L.op_wires; o->op_zs = L.op_zs; o->op_zs_next = L.op_zs_next;
  o->op_partial_products = L.op_pp; o->op_quotient = L.op_quot;
  o->fri_caps = L.fri_caps; o->queries = L.queries; o->query_words = L.query_words; o->q_init_sib = L.q_init_sib;
  for (int i = 0; i < 4; i++) { o->q_init_off[i] = L.q_init_off[i]; o->q_init_cols[i] = L.q_init_cols[i]; }
  for (int l = 0; l < LCP2_MAX_FRI_LAYERS; l++) { o->q_step_off[l] = L.q_step_off[l]; o->q_step_sib[l] = L.q_step_sib[l]; }
  o->final_poly = L.final_poly; o->final_len = L.final_len; o->pow_witness = L.pow_witness; o->total = L.total;
  return LCP2_OK;
}

extern "C" size_t lcp2_proof_bytes(const lcp2_params *p, size_t npi, uint32_t flags) {
  if (!params_ok(p)) return 0;
  size_t n = 0;
  walk_proof(*p, [&](size_t) { n += 8; return true; }, [&](size_t) { n += 1; return true; });
  return n + 8 * npi + ((flags & LCP2_SER_PUBLIC_INPUT_COUNT) ? 8 : 0);
}
extern "C" int lcp2_proof_to_bytes(const lcp2_params *p, const uint64_t *proof, size_t proof_words, const uint64_t *pis, size_t npi, uint32_t flags,
                                   uint8_t *out, size_t out_len) {
  if (!params_ok(p) || !proof || !out || (npi && !pis)) return LCP2_E_INVALID;
  if (proof_words != ProofLayout(*p).total || out_len != lcp2_proof_bytes(p, npi, flags)) return LCP2_E_INVALID;
  size_t pos = 0;
  bool ok = walk_proof(*p, [&](size_t w) { if (proof[w] >= GL_P) return false; put64(out + pos, proof[w]); pos += 8; return true; },
                       [&](size_t nsib) { if (nsib > 255) return false; out[pos++] = (uint8_t)nsib; return true; });
  if (!ok) return LCP2_E_INVALID;
  if (flags & LCP2_SER_PUBLIC_INPUT_COUNT) { put64(out + pos, npi); pos += 8; }
  for (size_t i = 0; i < npi; i++) { put64(out + pos, gl_canon(pis[i])); pos += 8; }
  return pos == out_len ? LCP2_OK : LCP2_E_INVALID;
}
extern "C" int lcp2_proof_from_bytes(const lcp2_params *p, const uint8_t *bytes, size_t len, uint32_t flags, uint64_t *proof, size_t proof_words,
                                     uint64_t *pis, size_t npi) {
  if (!params_ok(p) || !bytes || !proof || (npi && !pis)) return LCP2_E_INVALID;
  if (proof_words != ProofLayout(*p).total || len != lcp2_proof_bytes(p, npi, flags)) return LCP2_E_INVALID;  // nothing is read past `len`
  size_t pos = 0;
  bool ok = walk_proof(*p, [&](size_t w) { const u64 v = get64(bytes + pos); pos += 8; if (v >= GL_P) return false; proof[w] = v; return true; },
                       [&](size_t nsib) { return bytes[pos++] == (uint8_t)nsib && nsib <= 255; });
  if (!ok) return LCP2_E_INVALID;
  if (flags & LCP2_SER_PUBLIC_INPUT_COUNT) { if (get64(bytes + pos) != npi) return LCP2_E_INVALID; pos += 8; }
  for (size_t i = 0; i < npi; i++) { const u64 v = get64(bytes + pos); pos += 8; if (v >= GL_P) return LCP2_E_INVALID; pis[i] = v; }
  return LCP2_OK;
}
extern "C" int lcp2_verifier_data_to_bytes(const lcp2_circuit *c, uint8_t *out, size_t out_len) {
  if (!c || !out) return LCP2_E_INVALID;
  const VerifierView v = verifier_view(c);
  const size_t capw = (size_t)4 << v.p->cap_height;
  if (out_len != (capw + 4) * 8) return LCP2_E_INVALID;
  for (size_t i = 0; i < capw; i++) put64(out + 8 * i, v.cs_cap[i]);
  for (size_t i = 0; i < 4; i++) put64(out + 8 * (capw + i), v.digest[i]);
  return LCP2_OK;
}
