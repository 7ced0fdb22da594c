// TEST HARNESS (not product code): csrc/verify_query.hpp and csrc/verify_head.hpp compiled for the CPU - lcp2_verify_batch as loops
// over the jobs of its kernels: the canonical scan, the host's head per proof, then every Merkle path (proof, query, tree) in the
// one-lane reference form of k_verify_paths and every FRI query (proof, query) in the text k_verify_fri runs, each folded into the
// status word of its (proof, query) by minimum.  Built by tests/test_verify_batch_emu.py with g++ and included by
// tests/emu/sanitize_verify_main.cpp; never loaded by the package.
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/verify_head.hpp"
#include "emu_rc.hpp"

using namespace lcp2;

// the jobs of the two query kernels for one proof whose challenge block is `c`: status[num_queries]
static void emu_query_jobs(const VqLayout &V, const VqChallenge &c, const u64 *proof, const u64 *cs_cap, u32 *status) {
  for (u32 q = 0; q < V.num_queries; q++) status[q] = VQ_STATUS_NONE;
  if (!c.live) return;
  for (u32 t = 0; t < V.num_trees; t++)  // tree-major, as the kernel numbers its groups
    for (u32 q = 0; q < V.num_queries; q++) {
      const u32 s = vq_path_job(V, c, proof, cs_cap, q, t, emu_round_constants());
      if (s < status[q]) status[q] = s;
    }
  for (u32 q = 0; q < V.num_queries; q++) {
    const u32 s = vq_fri_query(V, c, proof, proof + V.final_poly, q);
    if (s < status[q]) status[q] = s;
  }
}

extern "C" {

unsigned emu_verify_status(unsigned ordinal, unsigned check) { return vq_status(ordinal, check); }
unsigned emu_verify_status_none() { return VQ_STATUS_NONE; }
// ordinals of the checks inside a query: kind 0 initial tree `i`, 1 consistency of layer `i`, 2 Merkle path of layer `i`, 3 final polynomial after `i` layers
unsigned emu_verify_ordinal(unsigned kind, unsigned i) {
  return kind == 0 ? vq_ord_initial(i) : kind == 1 ? vq_ord_consistency(i) : kind == 2 ? vq_ord_layer_path(i) : vq_ord_final(i);
}
unsigned emu_verify_reduce(const unsigned *status, unsigned num_queries) { return vq_reduce_statuses(status, num_queries); }
// what tree t of the layout reports, and how many trees it has
unsigned emu_verify_tree_status(const lcp2_params *p, unsigned t) { return vq_make_layout(ProofLayout(*p), *p).tree[t].status; }
unsigned emu_verify_num_trees(const lcp2_params *p) { return vq_make_layout(ProofLayout(*p), *p).num_trees; }

int emu_merkle_path(const unsigned long long *leaf, unsigned leaf_len, unsigned long long index, const unsigned long long *siblings, unsigned nsib,
                    const unsigned long long *cap) {
  return vq_merkle_path(leaf, leaf_len, index, siblings, nsib, cap, emu_round_constants()) ? 1 : 0;
}

// lcp2_verify_batch on the CPU: failed_checks[count], and (nullable) the status words [count][num_query_rounds] of the proofs that
// reached their queries (VQ_STATUS_NONE elsewhere).  desc: the circuit; digest, cap: its verifier data.  Returns the number of
// rejected proofs, -1 for a length that is not the circuit's.
int emu_verify_batch(const lcp2_circuit_desc *desc, const unsigned long long *digest, const unsigned long long *cap, const unsigned long long *proofs,
                     unsigned long long proof_words, unsigned long long count, const unsigned long long *public_inputs,
                     unsigned long long num_public_inputs, int *failed_checks, unsigned *statuses) {
  const lcp2_params &p = desc->params;
  const ProofLayout L(p);
  if (proof_words != L.total || num_public_inputs != desc->num_public_inputs) return -1;
  std::vector<u64> imm(desc->num_imm + 1, 0), k_is(p.num_routed_wires);
  for (size_t i = 0; i < desc->num_imm; i++) imm[i] = gl_canon(desc->imm[i]);
  for (u32 i = 0; i < p.num_routed_wires; i++) k_is[i] = gl_canon(desc->k_is[i]);
  VerifierView v;
  v.p = &p; v.npi = desc->num_public_inputs; v.num_selectors = desc->num_selectors; v.num_gates = desc->num_gates;
  v.gates = desc->gates; v.code = desc->code; v.imm = imm.data(); v.k_is = k_is.data(); v.digest = digest; v.cs_cap = cap;
  const VqLayout V = vq_make_layout(L, p);
  const u32 Q = p.num_query_rounds;
  std::vector<u32> status(Q ? Q : 1);
  int rejected = 0;
  for (u64 i = 0; i < count; i++) {
    const u64 *proof = proofs + i * proof_words;
    int rc = 0;
    for (u64 w = 0; w < proof_words && !rc; w++)
      if (proof[w] >= GL_P) rc = 1;  // k_verify_canon
    VqChallenge c;
    memset(&c, 0, sizeof c);
    if (!rc) {
      // the host sees the words outside the query section only: a copy of exactly those, as the strided download delivers them
      std::vector<u64> outside(proof, proof + L.queries);
      outside.insert(outside.end(), proof + L.final_poly, proof + L.total);
      rc = verify_head(v, L, outside.data(), outside.data() + L.queries, public_inputs + i * num_public_inputs, c);
      if (rc) memset(&c, 0, sizeof c);
    }
    emu_query_jobs(V, c, proof, cap, status.data());
    if (!rc) rc = (int)vq_reduce_statuses(status.data(), Q);
    if (statuses) for (u32 q = 0; q < Q; q++) statuses[i * Q + q] = status[q];
    failed_checks[i] = rc;
    rejected += rc != 0;
  }
  return rejected;
}

}  // extern "C"
