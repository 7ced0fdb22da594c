// TEST HARNESS (not product code): csrc/proof_compress.hpp compiled for the CPU - the predicates, the word count, the compression of
// a full-layout proof and the level-by-level reconstruction that a workgroup of k_decompress_paths is held to, all over query
// indices the caller passes in; and the query indices of a proof from its words outside the query section (the head's transcript).
// Built by tests/test_proof_compress_emu.py with g++ and included by tests/emu/sanitize_compress_main.cpp; never loaded by the package.
#include <cstring>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/proof_compress.hpp"
#include "../../eth-lc-plonky2_amd/csrc/verify_head.hpp"
#include "emu_rc.hpp"

using namespace lcp2;

static VqLayout emu_layout(const lcp2_params &p) { return vq_make_layout(ProofLayout(p), p); }

// LCP2_OK, or LCP2_E_INVALID for a word count that is not the one the indices imply; nothing is read past comp_words
static int emu_decompress_impl(const VqLayout &V, const u32 *x, const u64 *comp, u64 comp_words, u64 *proof) {
  if (comp_words < pc_outside_words(V) || comp_words != pc_compressed_words(V, x)) return LCP2_E_INVALID;
  memcpy(proof, comp, V.queries * 8);
  memset(proof + V.queries, 0, (V.final_poly - V.queries) * 8);
  memcpy(proof + V.final_poly, comp + V.queries, (V.proof_words - V.final_poly) * 8);
  const u64 *tree = comp + pc_outside_words(V);
  for (u32 t = 0; t < V.num_trees; t++) {
    pc_decompress_tree(V, x, t, tree, proof, emu_round_constants());
    tree += pc_tree_words(V, x, t);
  }
  return LCP2_OK;
}

extern "C" {

// the plan of query q in a tree of shift `shift` and nsib siblings: out[0] = merged, out[1] = stored mask
void emu_compress_plan(const unsigned *x, unsigned R, unsigned q, unsigned shift, unsigned nsib, unsigned *out) {
  const PcPlan p = pc_plan(x, R, q, shift, nsib);
  out[0] = p.merged; out[1] = p.stored;
}
unsigned long long emu_compressed_words(const lcp2_params *p, const unsigned *x) { return pc_compressed_words(emu_layout(*p), x); }
unsigned long long emu_compressed_words_max(const lcp2_params *p) { return pc_compressed_words_max(emu_layout(*p)); }
// proof: the full layout; out: emu_compressed_words(p, x) words.  Returns the word count written
unsigned long long emu_compress(const lcp2_params *p, const unsigned *x, const unsigned long long *proof, unsigned long long *out) {
  const VqLayout V = emu_layout(*p);
  memcpy(out, proof, V.queries * 8);
  memcpy(out + V.queries, proof + V.final_poly, (V.proof_words - V.final_poly) * 8);
  u64 words = pc_outside_words(V);
  for (u32 t = 0; t < V.num_trees; t++) words += pc_compress_tree(V, x, t, (const u64 *)proof, (u64 *)out + words);
  return words;
}
int emu_decompress(const lcp2_params *p, const unsigned *x, const unsigned long long *comp, unsigned long long comp_words, unsigned long long *proof) {
  return emu_decompress_impl(emu_layout(*p), x, (const u64 *)comp, comp_words, (u64 *)proof);
}
// the query indices the verifier derives (x[64]) from the words outside the query section, as a compressed proof begins: 0, or 2
// when the proof of work fails and there are none
int emu_compress_indices(const lcp2_circuit_desc *desc, const unsigned long long *digest, const unsigned long long *outside,
                         const unsigned long long *public_inputs, unsigned *x) {
  const lcp2_params &p = desc->params;
  const ProofLayout L(p);
  VerifierView v = {};
  v.p = &p; v.npi = desc->num_public_inputs; v.num_selectors = desc->num_selectors; v.num_gates = desc->num_gates; v.digest = (const u64 *)digest;
  const HeadLayout H = head_make_layout(v, L, 1);
  OneLaneSponge sp;
  sp.rc = emu_round_constants();
  HeadChallenges hc = {};
  VqChallenge c;
  memset(&c, 0, sizeof c);
  const int rc = head_transcript(sp, H, (const u64 *)outside, (const u64 *)outside + L.queries, (const u64 *)public_inputs, v.digest, hc, c);
  for (u32 q = 0; q < VQ_MAX_QUERIES; q++) x[q] = rc ? 0 : c.x_index[q];
  return rc;
}

}  // extern "C"
