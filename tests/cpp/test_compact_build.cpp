// CircuitBuilder::set_compact_build of the host layer: build() keeps rows, row constants and bindings instead of the expanded matrix
// and attach_gpu goes through lcp2_circuit_create_from_rows; digest, cap and proof must be those of the ordinary build, word for
// word, and the matrix a compact circuit expands on demand must be the ordinary circuit's.
// usage: test_compact_build cpu    both builds of ContractState (src/unit_tests.rs:169-246) and of the SHA-256 Merkle gadget of height 2:
//                                  the compact description holds no matrix, expanded_description() the ordinary one; the upload shrinks
//        test_compact_build gpu    the same circuits attached both ways: digest, cap, proof equal; each proof verifies under both handles
#include <cstdio>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include "../../eth-lc-plonky2_amd/host/gadgets.hpp"
#include "golden_data.hpp"

using namespace lc;

static void need(bool ok, const std::string &what) { if (!ok) throw std::runtime_error(what); }

struct Built {
  std::unique_ptr<CircuitData> data;
  PartialWitness pw;
};

static Built contract_state(bool compact) {
  Built out;
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  builder.set_compact_build(compact);
  ContractStateTarget t = add_virtual_contract_state_target(builder);
  uint8_t cur_slot_bytes[32] = {0}, new_slot_bytes[32] = {0};
  for (int i = 0; i < 8; i++) { cur_slot_bytes[i] = (uint8_t)(CONTRACT_STATE__CUR_SLOT >> (8 * i)); new_slot_bytes[i] = (uint8_t)(CONTRACT_STATE__NEW_SLOT >> (8 * i)); }
  out.pw.set_hash256_target(t.cur_state, CONTRACT_STATE__CUR_STATE);
  out.pw.set_hash256_target(t.cur_header, CONTRACT_STATE__CUR_HEADER);
  out.pw.set_hash256_target(t.cur_slot, cur_slot_bytes);
  out.pw.set_hash256_target(t.cur_sync_committee_i, CONTRACT_STATE__CUR_SYNC_COMMITTEE_I);
  out.pw.set_hash256_target(t.cur_sync_committee_ii, CONTRACT_STATE__CUR_SYNC_COMMITTEE_II);
  out.pw.set_hash256_target(t.new_state, CONTRACT_STATE__NEW_STATE);
  out.pw.set_hash256_target(t.new_header, CONTRACT_STATE__NEW_HEADER);
  out.pw.set_hash256_target(t.new_slot, new_slot_bytes);
  out.pw.set_hash256_target(t.new_sync_committee_i, CONTRACT_STATE__NEW_SYNC_COMMITTEE_I);
  out.pw.set_hash256_target(t.new_sync_committee_ii, CONTRACT_STATE__NEW_SYNC_COMMITTEE_II);
  out.data = builder.build();
  return out;
}

static Built merkle_tree(bool compact) {  // src/merkle_tree_gadget.rs: the root of four zero leaves
  Built out;
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  builder.set_compact_build(compact);
  MerkleTreeSha256Target tree = add_virtual_merkle_tree_sha256_target(builder, 2);
  Hash256Target expected_root = builder.add_virtual_hash256_target();
  builder.connect_hash256(tree.root, expected_root);
  for (int i = 0; i < 8; i++) builder.register_public_input(expected_root[i].t);
  out.data = builder.build();
  std::vector<std::array<uint8_t, 32>> leaves(4);
  for (auto &l : leaves) l.fill(0);
  set_partial_merkle_tree_sha256_target(out.pw, leaves, tree);
  out.pw.set_hash256_target(expected_root, ZERO_ROOT_4);
  return out;
}

static void both_ways(const char *name, const std::function<Built(bool)> &make, lcp2_ctx *ctx) {
  Built plain = make(false), compact = make(true);
  const CircuitDescription &P = plain.data->description();
  need(!P.constants_sigmas.empty() && compact.data->description().constants_sigmas.empty(), std::string(name) + ": only the compact build leaves the matrix out");
  need(compact.data->build_upload_bytes() < plain.data->build_upload_bytes() / 4, std::string(name) + ": the compact upload is no smaller");
  printf("upload: %s ordinary %zu compact %zu bytes\n", name, plain.data->build_upload_bytes(), compact.data->build_upload_bytes());
  if (ctx) {
    plain.data->attach_gpu(ctx);
    compact.data->attach_gpu(ctx);
    need(compact.data->description().constants_sigmas.empty(), std::string(name) + ": attach_gpu expanded the matrix on the host");
    uint64_t d0[4], d1[4];
    std::vector<uint64_t> cap0, cap1;
    plain.data->verifier_only_data(d0, cap0);
    compact.data->verifier_only_data(d1, cap1);
    need(memcmp(d0, d1, sizeof d0) == 0, std::string(name) + ": the circuit digests differ");
    need(cap0 == cap1, std::string(name) + ": the constants_sigmas caps differ");
    const ProofWithPublicInputs a = plain.data->prove(plain.pw), b = compact.data->prove(compact.pw);
    need(a.proof == b.proof && a.public_inputs == b.public_inputs, std::string(name) + ": the proofs differ");
    plain.data->verify(b);
    compact.data->verify(a);
  }
  // the matrix on demand, after the device form was used
  const CircuitDescription &C = compact.data->expanded_description();
  need(C.constants_sigmas == P.constants_sigmas, std::string(name) + ": the matrix expanded on demand differs from the ordinary build's");
  need(&plain.data->expanded_description() == &P, std::string(name) + ": expanded_description of an ordinary build is its description");
  need(C.k_is == P.k_is && C.params.degree_bits == P.params.degree_bits && C.gates.size() == P.gates.size(), std::string(name) + ": the descriptions differ");
}

static int run(bool gpu) {
  lcp2_ctx *ctx = nullptr;
  if (gpu) need(lcp2_ctx_create(0, nullptr, &ctx) == LCP2_OK, "lcp2_ctx_create");
  both_ways("ContractState", contract_state, ctx);
  both_ways("merkle_tree_height_2", merkle_tree, ctx);
  if (ctx) lcp2_ctx_destroy(ctx);
  printf("test_compact_build %s ... ok\n", gpu ? "gpu" : "cpu");
  return 0;
}

int main(int argc, char **argv) {
  try {
    if (argc == 2 && std::string(argv[1]) == "gpu") return run(true);
    if (argc == 2 && std::string(argv[1]) == "cpu") return run(false);
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "usage: %s cpu|gpu\n", argv[0]);
  return 2;
}
