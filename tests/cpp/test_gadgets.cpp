// Circuit-level tests that mirror the reference's own #[test]s one for one (same data, same shape:
// build gadget -> set witness incl. the EXPECTED output connected to the computed one -> prove -> verify):
//   src/merkle_tree_gadget.rs:183-325     test_merkle_root_{2,4,8,16}_leaves
//   src/sync_committee_pubkeys.rs:100-653 test_ssz_sync_committee              (BASELINE configs[1])
//   src/unit_tests.rs:37-246              test_signing_root, test_beacon_block_header, test_verify_finality_branch,
//                                         test_contract_state                   (BASELINE configs[0])
//   src/main.rs:84-233                    test_light_client_update: updates 633 -> 634 through add_virtual_proof_target /
//                                         set_proof_target (BASELINE configs[2], BLS verifier stubbed)
//   src/unit_tests.rs:288-620             sync-committee branch (index 55, height 5): one positive, one #[should_panic]
// usage: test_gadgets <cpu|gpu> <test name | all>
//   cpu: witness generation + row-wise constraint check + oracle prove/verify (the oracle is the checker; the product
//        library has no CPU prover) + the product's host verifier on the oracle's proof
//   gpu: data.prove(pw) on the MI355X through the C ABI, data.verify(proof), and word-for-word parity with the oracle
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include "../../eth-lc-plonky2_amd/host/gadgets.hpp"
#include "../../eth-lc-plonky2_amd/host/recursion.hpp"
#include "../../eth-lc-plonky2_amd/host/biguint.hpp"
#include "../../eth-lc-plonky2_amd/host/host_internal.hpp"
#include "../../oracle/oracle.h"
#include "../../oracle/plonk.h"
#include "golden_data.hpp"

using namespace lc;

static bool g_gpu = false;
static lcp2_ctx *g_ctx = nullptr;
static bool g_skip_oracle_prove = false;  // set by the large test in cpu mode

static std::array<uint8_t, 32> a32(const uint8_t *p) { std::array<uint8_t, 32> a; memcpy(a.data(), p, 32); return a; }

// an inner proof for the recursion tests: data.prove on the GPU in gpu mode, the oracle (the CPU prover of the tests) otherwise
struct InnerProof {
  std::unique_ptr<CircuitData> data;
  ProofWithPublicInputs proof;
  uint64_t digest[4];
  std::vector<uint64_t> cap;
};
// src/unit_tests.rs:29-35 prove_and_verify.  `out` (nullable) receives the proof with its public inputs and the circuit's digest and
// constants/sigmas cap: the oracle's in cpu mode, the GPU's (checked equal to the oracle's) in gpu mode
static void prove_and_verify(CircuitData &data, const PartialWitness &witness, InnerProof *out = nullptr) {

  const CircuitDescription &D = data.description();
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point a) {
    return (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - a).count();
  };
  data.generate_witness(witness, wires, pis);  // throws UnsatisfiedError = prove() returning Err
  const long long witness_ms = ms_since(t0);
  if (g_gpu && getenv("LCP2_TIMING_ONLY")) {  // timing run: GPU build + prove + verify only, no oracle work
    auto t1 = std::chrono::steady_clock::now();
    data.attach_gpu(g_ctx);
    const long long build_ms = ms_since(t1);
    ProofWithPublicInputs warm = data.prove(witness);
    t1 = std::chrono::steady_clock::now();
    ProofWithPublicInputs proof = data.prove(witness);
    const long long prove_ms = ms_since(t1);
    t1 = std::chrono::steady_clock::now();
    data.verify(proof);
    printf("timing: degree_bits %u  generate_witness(host, for comparison) %lld ms  build(GPU) %lld ms  prove incl. device witness generation (2nd call) %lld ms  verify(host) %lld ms\n",
           data.degree_bits(), witness_ms, build_ms, prove_ms, ms_since(t1));
    return;
  }
  orc_params op;
  static_assert(sizeof(orc_params) == sizeof(lcp2_params), "parameter layouts must agree");
  memcpy(&op, &D.params, sizeof op);
  std::vector<orc_gate> og(D.gates.size());
  static_assert(sizeof(orc_gate) == sizeof(lcp2_gate), "gate layouts must agree");
  memcpy(og.data(), D.gates.data(), og.size() * sizeof(orc_gate));
  // the oracle's build() (constants/sigmas commitment) is only needed when the oracle proves or verifies
  const bool need_built = !g_skip_oracle_prove || getenv("LCP2_ORACLE_PROVE_ALL") || (g_gpu && !getenv("LCP2_SKIP_ORACLE_BUILD"));
  orc_circuit *oc = (need_built ? orc_circuit_new : orc_circuit_new_unbuilt)(
      &op, D.constants_sigmas.data(), D.k_is.data(), D.num_selectors, og.data(), (uint32_t)og.size(), D.code.data(), D.code.size(),
      D.imm.data(), D.imm.size(), D.num_public_inputs);
  if (!oc) throw std::runtime_error("oracle rejected the circuit description");
  uint64_t bad[2] = {0, 0};
  size_t nbad = orc_check_witness(oc, wires.data(), pis.data(), bad);
  if (nbad) {
    orc_circuit_free(oc);
    throw std::runtime_error("gate constraints violated: " + std::to_string(nbad) + " (first: row " + std::to_string(bad[0]) + " constraint " + std::to_string(bad[1]) + ")");
  }
  std::vector<uint64_t> oproof;
  // LCP2_ORACLE_PROVE_ALL=1: the oracle also proves the circuits the suite leaves to the GPU run (2^19 rows and up: minutes of CPU
  // time each), so that their GPU proofs are compared word for word too (run once per round, profiles/r04_real_gadget_parity.log)
  const bool oracle_proves = !g_skip_oracle_prove || getenv("LCP2_ORACLE_PROVE_ALL");
  if (oracle_proves) {
    const auto tp = std::chrono::steady_clock::now();
    oproof.resize(orc_proof_words(&op));
    const int prc = orc_prove(oc, wires.data(), pis.data(), oproof.data());
    if (prc != 0) throw std::runtime_error("orc_prove failed with status " + std::to_string(prc));
    if (orc_verify(oc, oproof.data(), pis.data()) != 0) throw std::runtime_error("oracle verifier rejected the oracle proof");
    if (g_skip_oracle_prove) printf("oracle proved in %lld s (degree_bits %u)\n", (long long)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - tp).count(), data.degree_bits());
  }
  if (g_gpu) {
    data.attach_gpu(g_ctx);
    ProofWithPublicInputs proof = data.prove(witness);
    {  // the witness generated on the device (K10) equals the host generators' witness cell for cell
      std::vector<uint64_t> dev_wires;
      data.read_device_witness(dev_wires);
      if (dev_wires != wires) {
        size_t k = 0;
        while (dev_wires[k] == wires[k]) k++;
        const size_t nrows = (size_t)1 << D.params.degree_bits;
        throw std::runtime_error("device witness differs from the host witness at wire " + std::to_string(k / nrows) + " row " + std::to_string(k % nrows));
      }
    }
    auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    printf("proved in %lldms (degree_bits %u)\n", (long long)ms, data.degree_bits());
    data.verify(proof);  // assert!(data.verify(proof).is_ok())
    if (!oproof.empty() && proof.proof != oproof) throw std::runtime_error("GPU proof differs from the oracle proof");
    if (!oproof.empty() && (g_skip_oracle_prove || out)) printf("GPU proof equals the oracle proof word for word (%zu words, degree_bits %u, rate_bits %u)\n", oproof.size(), data.degree_bits(), D.params.rate_bits);
    if (need_built && orc_verify(oc, proof.proof.data(), pis.data()) != 0) throw std::runtime_error("oracle verifier rejected the GPU proof");
    {
      // the independent verifier at ANY size: the oracle's verifier from digest + constants/sigmas cap alone (no oracle build()),
      // as stock plonky2's VerifierCircuitData would check the proof (src/main.rs:233).  Accepts the GPU proof, rejects it after a
      // one-word flip (an opening: the vanishing identity; a Merkle leaf word of the first query: the path check)
      uint64_t digest[4];
      std::vector<uint64_t> cap;
      data.verifier_only_data(digest, cap);
      orc_circuit *ov = orc_verifier_new(&op, D.k_is.data(), D.num_selectors, og.data(), (uint32_t)og.size(), D.code.data(), D.code.size(), D.imm.data(),
                                         D.imm.size(), D.num_public_inputs, digest, cap.data());
      if (!ov) throw std::runtime_error("orc_verifier_new rejected the description");
      if (need_built) {  // where the oracle has built the circuit itself, the product's digest and cap must be the oracle's
        uint64_t od[4];
        std::vector<uint64_t> ocap(cap.size());
        orc_circuit_digest(oc, od, ocap.data());
        if (memcmp(od, digest, 32) != 0 || ocap != cap) throw std::runtime_error("product digest / constants cap differ from the oracle's build()");
      }
      int rc = orc_verify(ov, proof.proof.data(), pis.data());
      if (rc != 0) throw std::runtime_error("oracle verifier (verifier-only) rejected the GPU proof, check " + std::to_string(rc));
      lcp2_proof_layout L;
      lcp2_proof_layout_of(&D.params, &L);
      for (size_t w : {(size_t)L.op_wires + 3, (size_t)(L.queries + L.q_init_off[1] + 2)}) {
        std::vector<uint64_t> bad_proof = proof.proof;
        bad_proof[w] = bad_proof[w] == 5 ? 6 : 5;
        if (orc_verify(ov, bad_proof.data(), pis.data()) == 0) throw std::runtime_error("oracle verifier accepted a proof with word " + std::to_string(w) + " changed");
      }
      orc_circuit_free(ov);
      printf("oracle verifier (digest + cap only) accepted the GPU proof and rejected two one-word changes (degree_bits %u)\n", data.degree_bits());
      if (out) { out->proof = proof; memcpy(out->digest, digest, 32); out->cap = cap; }
    }
  } else if (oproof.empty()) {
    printf("witness generated (host, %lld ms) and every gate constraint checked (oracle), degree_bits %u\n", witness_ms, data.degree_bits());
  } else {
    // product host verifier on the oracle's proof (verifier-only circuit: digest + cap from the oracle's build)
    uint64_t digest[4];
    std::vector<uint64_t> cap((size_t)4 << D.params.cap_height);
    orc_circuit_digest(oc, digest, cap.data());
    lcp2_circuit_desc cd = D.c_desc();
    lcp2_circuit *vc = nullptr;
    if (lcp2_verifier_create(&cd, digest, cap.data(), &vc) != LCP2_OK) throw std::runtime_error("lcp2_verifier_create failed");
    int failed = 0;
    int rc = lcp2_verify(vc, oproof.data(), oproof.size(), pis.data(), pis.size(), &failed);
    lcp2_circuit_destroy(vc);
    if (rc != LCP2_OK) throw std::runtime_error("product verifier rejected the oracle proof, check " + std::to_string(failed));
    if (out) { out->proof.proof = oproof; out->proof.public_inputs = pis; memcpy(out->digest, digest, 32); out->cap = cap; }
    printf("proved (oracle) and verified, degree_bits %u (host witness generation %lld ms)\n", data.degree_bits(), witness_ms);
  }
  orc_circuit_free(oc);
}

// A circuit that verify_proof builds, pinned: the in-circuit verifier adds one gate per call of its target algebra, so walking the
// inner gate programs in another order, or with a multiplication and an addition where one fused operation stood, builds another
// circuit.  The oracle parity cannot see that (the oracle proves whatever circuit it is handed); the digest can.
struct CircuitPin { uint64_t digest[4]; uint32_t degree_bits; size_t num_gates; };
static void expect_circuit(const std::string &what, const CircuitPin &want, const uint64_t digest[4], uint32_t degree_bits, size_t num_gates) {
  printf("%s: digest 0x%llx 0x%llx 0x%llx 0x%llx, 2^%u rows, %zu gates\n", what.c_str(), (unsigned long long)digest[0], (unsigned long long)digest[1],
         (unsigned long long)digest[2], (unsigned long long)digest[3], degree_bits, num_gates);
  if (memcmp(digest, want.digest, 32) != 0 || degree_bits != want.degree_bits || num_gates != want.num_gates)
    throw std::runtime_error(what + ": verify_proof built another circuit than the pinned one");
}

static void prove_standalone(InnerProof &in, const PartialWitness &pw) {
  const CircuitDescription &D = in.data->description();
  if (g_gpu) {
    in.data->attach_gpu(g_ctx);
    in.proof = in.data->prove(pw);
    in.data->verify(in.proof);
    in.data->verifier_only_data(in.digest, in.cap);
    return;
  }
  std::vector<uint64_t> wires;
  in.data->generate_witness(pw, wires, in.proof.public_inputs);
  orc_params op;
  memcpy(&op, &D.params, sizeof op);
  std::vector<orc_gate> og(D.gates.size());
  memcpy(og.data(), D.gates.data(), og.size() * sizeof(orc_gate));
  orc_circuit *oc = orc_circuit_new(&op, D.constants_sigmas.data(), D.k_is.data(), D.num_selectors, og.data(), (uint32_t)og.size(), D.code.data(), D.code.size(),
                                    D.imm.data(), D.imm.size(), D.num_public_inputs);
  if (!oc) throw std::runtime_error("oracle rejected the inner circuit");
  in.proof.proof.resize(orc_proof_words(&op));
  orc_prove(oc, wires.data(), in.proof.public_inputs.data(), in.proof.proof.data());
  if (orc_verify(oc, in.proof.proof.data(), in.proof.public_inputs.data()) != 0) throw std::runtime_error("oracle verifier rejected the inner proof");
  in.cap.resize((size_t)4 << D.params.cap_height);
  orc_circuit_digest(oc, in.digest, in.cap.data());
  orc_circuit_free(oc);
}

// ---- src/merkle_tree_gadget.rs:183-325
static void merkle_root_zero_leaves(size_t height, const uint8_t *root) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  size_t num_gates = builder.num_gates();
  MerkleTreeSha256Target merkle_tree_target = add_virtual_merkle_tree_sha256_target(builder, height);
  Hash256Target expected_root = builder.add_virtual_hash256_target();
  builder.connect_hash256(merkle_tree_target.root, expected_root);
  num_gates = builder.num_gates() - num_gates;
  auto data = builder.build();
  printf("circuit num_gates=%zu, quotient_degree_factor=%u\n", num_gates, data->quotient_degree_factor());
  PartialWitness pw;
  std::vector<std::array<uint8_t, 32>> leaves((size_t)1 << height);
  for (auto &l : leaves) l.fill(0);
  set_partial_merkle_tree_sha256_target(pw, leaves, merkle_tree_target);
  pw.set_hash256_target(expected_root, root);
  prove_and_verify(*data, pw);
}
static void test_merkle_root_2_leaves() { merkle_root_zero_leaves(1, ZERO_ROOT_2); }
static void test_merkle_root_4_leaves() { merkle_root_zero_leaves(2, ZERO_ROOT_4); }
static void test_merkle_root_8_leaves() { merkle_root_zero_leaves(3, ZERO_ROOT_8); }
static void test_merkle_root_16_leaves() { merkle_root_zero_leaves(4, ZERO_ROOT_16); }
static void test_merkle_root_wrong_root_panics() {  // a wrong expected value makes prove() fail (KAT semantics)
  uint8_t wrong[32];
  memcpy(wrong, ZERO_ROOT_4, 32);
  wrong[5] ^= 1;
  merkle_root_zero_leaves(2, wrong);
}

// ---- src/sync_committee_pubkeys.rs:100-653
static void test_ssz_sync_committee() {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  std::vector<std::array<Target, G1_PUBKEY_SIZE>> pubkeys_target;
  for (size_t i = 0; i < SYNC_COMMITTEE_SIZE; i++) pubkeys_target.push_back(builder.add_virtual_target_arr<G1_PUBKEY_SIZE>());
  auto agg_pk_target = builder.add_virtual_target_arr<G1_PUBKEY_SIZE>();
  SyncCommitteeTarget sync_committee_target{pubkeys_target, agg_pk_target};
  Hash256Target sync_committee_ssz_target = ssz_sync_committee(builder, sync_committee_target);
  builder.print_gate_counts(0);
  auto data = builder.build();
  PartialWitness pw;
  for (size_t i = 0; i < SYNC_COMMITTEE_SIZE; i++) {
    std::vector<F> pk_bytes_f(SC_PUBKEYS[i], SC_PUBKEYS[i] + G1_PUBKEY_SIZE);
    pw.set_target_arr(sync_committee_target.pubkeys[i], pk_bytes_f);
  }
  std::vector<F> agg_pk_bytes_f(SC_AGG_PUBKEY, SC_AGG_PUBKEY + G1_PUBKEY_SIZE);
  pw.set_target_arr(sync_committee_target.aggregate_pubkey, agg_pk_bytes_f);
  pw.set_hash256_target(sync_committee_ssz_target, SC_SSZ_ROOT);
  g_skip_oracle_prove = true;  // 2^19 rows: the oracle checks every constraint row-wise; proving is left to the GPU run
  prove_and_verify(*data, pw);
  g_skip_oracle_prove = false;
}

// ---- src/unit_tests.rs:37-65
static void test_signing_root() {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  SigningRootTarget t = add_virtual_signing_root_target(builder);
  PartialWitness witness;
  witness.set_hash256_target(t.header_root, SIGNING_ROOT__ATTESTED_HEADER_ROOT);
  witness.set_hash256_target(t.domain, SIGNING_ROOT__DOMAIN);
  witness.set_hash256_target(t.signing_root, SIGNING_ROOT__SIGNING_ROOT);
  auto data = builder.build();
  prove_and_verify(*data, witness);
}
// ---- src/unit_tests.rs:67-106
static void test_beacon_block_header() {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  BeaconBlockHeaderTarget t = add_virtual_beacon_block_header_target(builder);
  PartialWitness witness;
  set_beacon_block_header_target(witness, BEACON_BLOCK_HEADER__HEADER_ROOT, BEACON_BLOCK_HEADER__SLOT, BEACON_BLOCK_HEADER__PROPOSER_INDEX,
                                 BEACON_BLOCK_HEADER__PARENT_ROOT, BEACON_BLOCK_HEADER__STATE_ROOT, BEACON_BLOCK_HEADER__BODY_ROOT, t);
  auto data = builder.build();
  prove_and_verify(*data, witness);
}
// ---- src/unit_tests.rs:108-167
static void test_verify_finality_branch() {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  VerifyMerkleProofTarget t = add_verify_merkle_proof_target(builder, FINALIZED_HEADER_INDEX, FINALIZED_HEADER_HEIGHT);
  std::vector<std::array<uint8_t, 32>> branch;
  for (size_t i = 0; i < FINALIZED_HEADER_HEIGHT; i++) branch.push_back(a32(VERIFY_FINALITY_BRANCH__FINALITY_BRANCH[i]));
  PartialWitness witness;
  set_verify_merkle_proof_target(witness, VERIFY_FINALITY_BRANCH__FINALIZED_HEADER_ROOT, branch, VERIFY_FINALITY_BRANCH__ATTESTED_STATE_ROOT, t);
  auto data = builder.build();
  prove_and_verify(*data, witness);
}
// ---- src/unit_tests.rs:169-246  (BASELINE configs[0])
static void test_contract_state() {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  ContractStateTarget t = add_virtual_contract_state_target(builder);
  PartialWitness witness;
  uint8_t cur_slot_bytes[32] = {0}, new_slot_bytes[32] = {0};
  for (int i = 0; i < 8; i++) { cur_slot_bytes[i] = (uint8_t)(CONTRACT_STATE__CUR_SLOT >> (8 * i)); new_slot_bytes[i] = (uint8_t)(CONTRACT_STATE__NEW_SLOT >> (8 * i)); }
  witness.set_hash256_target(t.cur_state, CONTRACT_STATE__CUR_STATE);
  witness.set_hash256_target(t.cur_header, CONTRACT_STATE__CUR_HEADER);
  witness.set_hash256_target(t.cur_slot, cur_slot_bytes);
  witness.set_hash256_target(t.cur_sync_committee_i, CONTRACT_STATE__CUR_SYNC_COMMITTEE_I);
  witness.set_hash256_target(t.cur_sync_committee_ii, CONTRACT_STATE__CUR_SYNC_COMMITTEE_II);
  witness.set_hash256_target(t.new_state, CONTRACT_STATE__NEW_STATE);
  witness.set_hash256_target(t.new_header, CONTRACT_STATE__NEW_HEADER);
  witness.set_hash256_target(t.new_slot, new_slot_bytes);
  witness.set_hash256_target(t.new_sync_committee_i, CONTRACT_STATE__NEW_SYNC_COMMITTEE_I);
  witness.set_hash256_target(t.new_sync_committee_ii, CONTRACT_STATE__NEW_SYNC_COMMITTEE_II);
  auto data = builder.build();
  prove_and_verify(*data, witness);
}
// ---- the Merkle-branch part of src/unit_tests.rs:288-383 (positive) and :377-477 (#[should_panic])
static void sync_committee_branch(const uint8_t *leaf, const uint8_t branch[][32], const uint8_t *root) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  VerifyMerkleProofTarget t = add_verify_merkle_proof_target(builder, SYNC_COMMITTEE_INDEX, SYNC_COMMITTEE_HEIGHT);
  std::vector<std::array<uint8_t, 32>> br;
  for (size_t i = 0; i < SYNC_COMMITTEE_HEIGHT; i++) br.push_back(a32(branch[i]));
  PartialWitness witness;
  set_verify_merkle_proof_target(witness, leaf, br, root, t);
  auto data = builder.build();
  prove_and_verify(*data, witness);
}
static void test_verify_sync_committee_branch() {
  sync_committee_branch(SC_ATTESTED_FROM_NEXT_PERIOD1__NEW_SYNC_COMMITTEE_II, SC_ATTESTED_FROM_NEXT_PERIOD1__NEW_SYNC_COMMITTEE_II_BRANCH,
                        SC_ATTESTED_FROM_NEXT_PERIOD1__FINALIZED_STATE_ROOT);
}
static void test_verify_sync_committee_branch_panics() {
  sync_committee_branch(SC_ATTESTED_FROM_NEXT_PERIOD2__NEW_SYNC_COMMITTEE_II, SC_ATTESTED_FROM_NEXT_PERIOD2__NEW_SYNC_COMMITTEE_II_BRANCH,
                        SC_ATTESTED_FROM_NEXT_PERIOD2__FINALIZED_STATE_ROOT);
}
// public inputs + arithmetic glue: read_u32_be of 4 byte targets equals a registered public input
static void test_read_u32_be_public_input() {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  auto bytes = builder.add_virtual_target_arr<4>();
  U32Target v = read_u32_be(builder, bytes.data(), 0);
  builder.register_public_input(v.t);
  auto data = builder.build();
  PartialWitness pw;
  pw.set_target_arr(bytes, {0x12, 0x34, 0x56, 0x78});
  prove_and_verify(*data, pw);
  std::vector<uint64_t> wires; std::vector<F> pis;
  data->generate_witness(pw, wires, pis);
  if (pis.size() != 1 || pis[0] != 0x12345678ull) throw std::runtime_error("public input value");
}

// ---- src/main.rs:84-233: the full light-client step for the committed update pair 633 -> 634 (BASELINE configs[2]).
// Native values (header roots, contract states, committee roots) come from the oracle's SHA-256 restatement, as
// main.rs takes them from tree_hash_root(); the domain is compute_domain(DOMAIN_SYNC_COMMITTEE, Bellatrix fork
// version, mainnet genesis_validators_root) -- with the BLS verifier stubbed any 32 bytes keep the circuit consistent.
static void sha2(const uint8_t *l, const uint8_t *r, uint8_t *out) { orc_sha256_two_to_one(l, r, out); }
enum LcVariant { LC_OK, LC_BAD_STATE_ROOT, LC_LOW_PARTICIPATION, LC_WITH_BLS_PROOF, LC_BLS_PROOF_OF_OTHER_BITS };
static void light_client_update(LcVariant variant, int extra_committees = 0) {
  // src/main.rs:170-176: the BLS-signature proof comes first (here: of the stand-in statement circuit), its common data shapes
  // the recursive verifier inside the light-client circuit
  const bool with_bls = variant == LC_WITH_BLS_PROOF || variant == LC_BLS_PROOF_OF_OTHER_BITS;
  InnerProof bls;
  BlsStatementStandIn bls_circuit;
  CommonCircuitData bls_cd;
  if (with_bls) {
    bls_circuit = build_bls_statement_stand_in();
    bls_cd = CommonCircuitData::of(bls_circuit.data->description());
  }
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  ProofTarget target = add_virtual_proof_target(builder, with_bls ? &bls_cd : nullptr);
  for (auto &limb : target.cur_state) builder.register_public_input(limb.t);  // src/main.rs:180-187
  for (auto &limb : target.new_state) builder.register_public_input(limb.t);
  // the reference's scale made of real gadgets (README.md:71, ~2.98 M gates): the step plus `extra_committees` more
  // SyncCommitteeSSZ gadgets over the signing committee (as examples/lc_prover --extra-committees)
  std::vector<SyncCommitteeTarget> more;
  for (int k = 0; k < extra_committees; k++) {
    more.push_back(add_virtual_sync_committee_target(builder));
    ssz_sync_committee(builder, more.back());
  }
  builder.print_gate_counts(0);
  auto data = builder.build();

  static const uint8_t DOMAIN[32] = {0x07, 0, 0, 0, 0x4a, 0x26, 0xc5, 0x8b, 0x08, 0xad, 0xd8, 0x08, 0x9b, 0x75, 0xca, 0xa5,
                                     0x40, 0x84, 0x88, 0x81, 0xa8, 0xd4, 0xf0, 0xaf, 0x0b, 0xe8, 0x34, 0x17, 0xa8, 0x5c, 0x0f, 0x45};
  uint8_t attested_header_root[32], finalized_header_root[32], cur_header[32], signing_root[32];
  orc_beacon_header_root(LC634__ATTESTED_SLOT, LC634__ATTESTED_PROPOSER_INDEX, LC634__ATTESTED_PARENT_ROOT, LC634__ATTESTED_STATE_ROOT,
                         LC634__ATTESTED_BODY_ROOT, attested_header_root);
  orc_beacon_header_root(LC634__FINALIZED_SLOT, LC634__FINALIZED_PROPOSER_INDEX, LC634__FINALIZED_PARENT_ROOT, LC634__FINALIZED_STATE_ROOT,
                         LC634__FINALIZED_BODY_ROOT, finalized_header_root);
  orc_beacon_header_root(LC633__FINALIZED_SLOT, LC633__FINALIZED_PROPOSER_INDEX, LC633__FINALIZED_PARENT_ROOT, LC633__FINALIZED_STATE_ROOT,
                         LC633__FINALIZED_BODY_ROOT, cur_header);
  sha2(attested_header_root, DOMAIN, signing_root);
  // contract state before: slot/header of 633's finalized block, committees (i, ii) = (633's branch[0], root(633.next))
  uint8_t cur_ii[32], new_ii[32], cur_state[32], new_state[32];
  orc_ssz_sync_committee_root(&LC633__NEXT_SYNC_COMMITTEE_PUBKEYS[0][0], LC633__NEXT_SYNC_COMMITTEE_AGGREGATE, cur_ii);
  orc_ssz_sync_committee_root(&LC634__NEXT_SYNC_COMMITTEE_PUBKEYS[0][0], LC634__NEXT_SYNC_COMMITTEE_AGGREGATE, new_ii);
  const uint8_t *cur_i = LC633__NEXT_SYNC_COMMITTEE_BRANCH[0], *new_i = LC634__NEXT_SYNC_COMMITTEE_BRANCH[0];
  if (memcmp(cur_ii, new_i, 32) != 0) throw std::runtime_error("fixture: root(633.next_sync_committee) != 634.next_sync_committee_branch[0]");
  const uint64_t cur_slot = LC633__FINALIZED_SLOT;
  orc_contract_state_root(cur_slot, cur_header, cur_i, cur_ii, cur_state);
  orc_contract_state_root(LC634__FINALIZED_SLOT, finalized_header_root, new_i, new_ii, new_state);
  std::vector<bool> bits(SYNC_COMMITTEE_SIZE);
  size_t participation = 0;
  for (size_t i = 0; i < SYNC_COMMITTEE_SIZE; i++) {
    bits[i] = (LC634__SYNC_COMMITTEE_BITS[i / 8] >> (i % 8)) & 1;
    if (variant == LC_LOW_PARTICIPATION && participation >= FINALITY_THRESHOLD) bits[i] = false;  // exactly 342 signers: not enough
    participation += bits[i];
  }
  if (LC634__ATTESTED_SLOT / 8192 != LC633__FINALIZED_SLOT / 8192 + 1) throw std::runtime_error("fixture: attested slot is expected to be in the period after the current state");
  uint8_t attested_state_root[32];
  memcpy(attested_state_root, LC634__ATTESTED_STATE_ROOT, 32);
  if (variant == LC_BAD_STATE_ROOT) attested_state_root[5] ^= 1;  // breaks the header root, finality branch and committee branch

  PartialWitness pw;
  set_proof_target(pw, signing_root, DOMAIN, LC634__ATTESTED_SLOT, LC634__ATTESTED_PROPOSER_INDEX, attested_header_root,
                   LC634__ATTESTED_PARENT_ROOT, attested_state_root, LC634__ATTESTED_BODY_ROOT, LC634__FINALIZED_SLOT,
                   LC634__FINALIZED_PROPOSER_INDEX, finalized_header_root, LC634__FINALIZED_PARENT_ROOT, LC634__FINALIZED_STATE_ROOT,
                   LC634__FINALIZED_BODY_ROOT, LC634__FINALITY_BRANCH, cur_state, new_state, LC633__FINALIZED_SLOT, cur_header, cur_i, cur_ii,
                   new_i, new_ii, bits, LC634__NEXT_SYNC_COMMITTEE_BRANCH, LC633__NEXT_SYNC_COMMITTEE_PUBKEYS,
                   LC633__NEXT_SYNC_COMMITTEE_AGGREGATE, LC634__SYNC_COMMITTEE_SIGNATURE, target);
  for (const SyncCommitteeTarget &sc : more) {
    for (size_t i = 0; i < SYNC_COMMITTEE_SIZE; i++)
      pw.set_target_arr(sc.pubkeys[i], std::vector<F>(LC633__NEXT_SYNC_COMMITTEE_PUBKEYS[i], LC633__NEXT_SYNC_COMMITTEE_PUBKEYS[i] + G1_PUBKEY_SIZE));
    pw.set_target_arr(sc.aggregate_pubkey, std::vector<F>(LC633__NEXT_SYNC_COMMITTEE_AGGREGATE, LC633__NEXT_SYNC_COMMITTEE_AGGREGATE + G1_PUBKEY_SIZE));
  }
  if (with_bls) {
    PartialWitness bpw;
    std::vector<bool> proved_bits = bits;
    if (variant == LC_BLS_PROOF_OF_OTHER_BITS) proved_bits[17] = !proved_bits[17];  // a proof about another participation set
    set_bls_statement_stand_in(bpw, bls_circuit, signing_root, LC634__SYNC_COMMITTEE_SIGNATURE, LC633__NEXT_SYNC_COMMITTEE_PUBKEYS, proved_bits);
    bls.data = std::move(bls_circuit.data);
    prove_standalone(bls, bpw);
    printf("BLS statement stand-in: 2^%u rows, %zu public inputs, %zu proof words\n", bls.data->degree_bits(), bls.proof.public_inputs.size(), bls.proof.proof.size());
    set_bls_proof_target(pw, target, bls.proof, bls.digest, bls.cap);
  }
  printf("light-client update 633 -> 634: participation %zu / 512, attested slot %llu (period %llu), state slot %llu -> %llu\n", participation,
         (unsigned long long)LC634__ATTESTED_SLOT, (unsigned long long)(LC634__ATTESTED_SLOT / 8192), (unsigned long long)LC633__FINALIZED_SLOT,
         (unsigned long long)LC634__FINALIZED_SLOT);
  g_skip_oracle_prove = true;  // 2^19 rows: see test_ssz_sync_committee
  try { prove_and_verify(*data, pw); } catch (...) { g_skip_oracle_prove = false; throw; }
  g_skip_oracle_prove = false;
}
static void test_light_client_update() { light_client_update(LC_OK); }
// GPU only: 7 207 two_to_one_sha256, 2.24 M gates, 2^22 rows.  The oracle checks every gate constraint of the witness row-wise,
// the device witness equals the host generators' cell for cell, and the proof is accepted by the product's verifier and by the
// oracle's verifier (from digest + cap alone: the oracle's own build() would take minutes at this size) and rejected by it after
// a one-word change
static void test_real_gadget_circuit_2p22() {
  if (!g_gpu) { printf("(gpu only)\n"); return; }
  setenv("LCP2_SKIP_ORACLE_BUILD", "1", 1);
  try { light_client_update(LC_OK, 6); } catch (...) { unsetenv("LCP2_SKIP_ORACLE_BUILD"); throw; }
  unsetenv("LCP2_SKIP_ORACLE_BUILD");
}
static void test_light_client_update_bad_state_root_panics() { light_client_update(LC_BAD_STATE_ROOT); }
// src/targets.rs:304-332 update_validity and :184-235 find_sync_committee reject what they are there to reject
static void test_light_client_update_low_participation_panics() { light_client_update(LC_LOW_PARTICIPATION); }
// src/targets.rs:468-482 built as in the reference: the circuit verifies a proof with the BLS proof's 25 216 public inputs
// recursively and ties them to the signing root, the signature, the committee and the participation bits
static void test_light_client_update_with_recursive_proof() { light_client_update(LC_WITH_BLS_PROOF); }
static void test_light_client_update_recursive_proof_of_other_bits_panics() { light_client_update(LC_BLS_PROOF_OF_OTHER_BITS); }

// ---- the slot / participation gadgets on their own (src/targets.rs:184-235, :304-332, src/utils.rs:93-113)
static void slot_h256(uint64_t slot, uint8_t out[32]) { memset(out, 0, 32); for (int i = 0; i < 8; i++) out[i] = (uint8_t)(slot >> (8 * i)); }
static void find_sync_committee(uint64_t cur_slot, uint64_t attested_slot, bool expect_next) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  FindSyncCommitteeTarget t = add_virtual_find_sync_committee_target(builder);
  Hash256Target expected = builder.add_virtual_hash256_target();
  builder.connect_hash256(t.sync_committee_for_attested_slot, expected);
  builder.register_public_input(t.is_attested_from_next_period.target);
  builder.register_public_input(t.cur_slot.value);
  auto data = builder.build();
  PartialWitness pw;
  uint8_t b[32];
  slot_h256(cur_slot, b); pw.set_hash256_target(t.cur_slot.h256, b);
  slot_h256(attested_slot, b); pw.set_hash256_target(t.attested_slot.h256, b);
  pw.set_hash256_target(t.cur_sync_committee_i, CONTRACT_STATE__CUR_SYNC_COMMITTEE_I);
  pw.set_hash256_target(t.cur_sync_committee_ii, CONTRACT_STATE__CUR_SYNC_COMMITTEE_II);
  pw.set_hash256_target(expected, expect_next ? CONTRACT_STATE__CUR_SYNC_COMMITTEE_II : CONTRACT_STATE__CUR_SYNC_COMMITTEE_I);
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  data->generate_witness(pw, wires, pis);
  if (pis[0] != (F)expect_next || pis[1] != cur_slot) throw std::runtime_error("find_sync_committee: wrong period flag or slot value");
  prove_and_verify(*data, pw);
}
static void test_find_sync_committee_current_period() { find_sync_committee(LC633__FINALIZED_SLOT, LC633__FINALIZED_SLOT + 100, false); }
static void test_find_sync_committee_next_period() { find_sync_committee(LC633__FINALIZED_SLOT, LC634__ATTESTED_SLOT, true); }
static void test_find_sync_committee_stale_period_panics() { find_sync_committee(LC633__FINALIZED_SLOT - 8192, LC634__ATTESTED_SLOT, true); }
static void test_find_sync_committee_previous_period_panics() { find_sync_committee(LC634__ATTESTED_SLOT, LC633__FINALIZED_SLOT, false); }
static void test_slot_connect_rejects_wide_encoding_panics() {  // byte 8 of the 32-byte slot encoding is not zero
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  SlotConnectTarget t = add_virtual_biguint_hash256_connect_target(builder);
  auto data = builder.build();
  PartialWitness pw;
  uint8_t b[32];
  slot_h256(5, b);
  b[8] = 1;
  pw.set_hash256_target(t.h256, b);
  prove_and_verify(*data, pw);
}
static void update_validity(uint64_t cur_slot, uint64_t finalized_slot, uint64_t participation) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  UpdateValidityTarget t = add_virtual_update_validity_target(builder);
  auto data = builder.build();
  PartialWitness pw;
  pw.set_target(t.cur_slot, cur_slot);
  pw.set_target(t.finalized_slot, finalized_slot);
  pw.set_target(t.participation, participation);
  prove_and_verify(*data, pw);
}
static void test_update_validity() { update_validity(LC633__FINALIZED_SLOT, LC634__FINALIZED_SLOT, 428); }
static void test_update_validity_equal_slots_and_343() { update_validity(7, 7, FINALITY_THRESHOLD + 1); }
static void test_update_validity_finalized_before_current_panics() { update_validity(LC634__FINALIZED_SLOT, LC633__FINALIZED_SLOT, 428); }
static void test_update_validity_threshold_not_exceeded_panics() { update_validity(1, 2, FINALITY_THRESHOLD); }

// ---- BigUint gadgets (plonky2_crypto biguint as the reference uses it: src/targets.rs:184-235, 304-332, src/utils.rs:76-113)
typedef unsigned __int128 u128;
static BigUintValue limbs_of(u128 v, size_t n) { BigUintValue r(n); for (size_t i = 0; i < n; i++) r[i] = (uint32_t)(v >> (32 * i)); return r; }
static void biguint_arithmetic(uint64_t a_val, uint64_t b_val, uint64_t d_val) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  BigUintTarget a = add_virtual_biguint_target(builder, 3), b = add_virtual_biguint_target(builder, 2), d = add_virtual_biguint_target(builder, 2);
  BigUintTarget sum = add_biguint(builder, a, b), prod = mul_biguint(builder, a, b);
  auto qr = div_rem_biguint(builder, prod, d);
  BoolTarget le_ab = cmp_biguint(builder, a, b), le_ba = cmp_biguint(builder, b, a), le_aa = cmp_biguint(builder, a, a);
  BigUintTarget want_sum = add_virtual_biguint_target(builder, 3), want_prod = add_virtual_biguint_target(builder, 4), want_q = add_virtual_biguint_target(builder, 4),
                want_r = add_virtual_biguint_target(builder, 2);
  connect_biguint(builder, sum, want_sum);   // sum has one limb more than its longer operand: it must be zero here
  connect_biguint(builder, prod, want_prod);
  connect_biguint(builder, qr.first, want_q);
  connect_biguint(builder, qr.second, want_r);
  for (Target t : {le_ab.target, le_ba.target, le_aa.target}) builder.register_public_input(t);
  auto data = builder.build();
  PartialWitness pw;
  const u128 A = a_val, B = b_val, D = d_val, S = A + B, M = A * B;
  set_biguint_target(pw, a, limbs_of(A, 3)); set_biguint_target(pw, b, limbs_of(B, 2)); set_biguint_target(pw, d, limbs_of(D, 2));
  set_biguint_target(pw, want_sum, limbs_of(S, 3)); set_biguint_target(pw, want_prod, limbs_of(M, 4));
  set_biguint_target(pw, want_q, limbs_of(D ? M / D : 0, 4)); set_biguint_target(pw, want_r, limbs_of(D ? M % D : 0, 2));  // D = 0: the generator refuses
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  data->generate_witness(pw, wires, pis);
  if (pis[0] != (F)(A <= B) || pis[1] != (F)(B <= A) || pis[2] != 1) throw std::runtime_error("cmp_biguint: wrong comparison result");
  prove_and_verify(*data, pw);
}
static void test_biguint_arithmetic() { biguint_arithmetic(0x123456789abcdef0ull, 0x0fedcba987654321ull, 8192); }
static void test_biguint_arithmetic_all_ones() { biguint_arithmetic(~0ull, ~0ull, 0xffffffff00000001ull); }  // every carry chain at its longest
static void test_biguint_division_by_zero_panics() { biguint_arithmetic(5, 7, 0); }
static void test_biguint_hash256_connect() {  // src/utils.rs:93-113: an SSZ uint256 (32 little-endian bytes) and the integer it encodes
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  BigUintHash256ConnectTarget t = add_virtual_biguint_hash256_connect_target_big(builder);
  auto data = builder.build();
  PartialWitness pw;
  uint8_t bytes[32];
  BigUintValue v(8);
  for (int i = 0; i < 32; i++) bytes[i] = (uint8_t)(17 * i + 3);
  for (int i = 0; i < 8; i++) v[i] = bytes[4 * i] | bytes[4 * i + 1] << 8 | bytes[4 * i + 2] << 16 | (uint32_t)bytes[4 * i + 3] << 24;
  pw.set_hash256_target(t.h256, bytes);
  set_biguint_target(pw, t.big, v);
  prove_and_verify(*data, pw);
}
static void find_sync_committee_big(uint64_t cur_slot, uint64_t attested_slot, bool expect_next) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  FindSyncCommitteeBigTarget t = add_virtual_find_sync_committee_target_big(builder);
  Hash256Target expected = builder.add_virtual_hash256_target();
  builder.connect_hash256(t.sync_committee_for_attested_slot, expected);
  builder.register_public_input(t.is_attested_from_next_period.target);
  auto data = builder.build();
  PartialWitness pw;
  set_biguint_target(pw, t.cur_slot_big, biguint_from_u64(cur_slot));
  set_biguint_target(pw, t.attested_slot_big, biguint_from_u64(attested_slot));
  pw.set_hash256_target(t.cur_sync_committee_i, CONTRACT_STATE__CUR_SYNC_COMMITTEE_I);
  pw.set_hash256_target(t.cur_sync_committee_ii, CONTRACT_STATE__CUR_SYNC_COMMITTEE_II);
  pw.set_hash256_target(expected, expect_next ? CONTRACT_STATE__CUR_SYNC_COMMITTEE_II : CONTRACT_STATE__CUR_SYNC_COMMITTEE_I);
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  data->generate_witness(pw, wires, pis);
  if (pis[0] != (F)expect_next) throw std::runtime_error("find_sync_committee (BigUint form): wrong period flag");
  prove_and_verify(*data, pw);
}
static void test_find_sync_committee_big_current_period() { find_sync_committee_big(LC633__FINALIZED_SLOT, LC633__FINALIZED_SLOT + 100, false); }
static void test_find_sync_committee_big_next_period() { find_sync_committee_big(LC633__FINALIZED_SLOT, LC634__ATTESTED_SLOT, true); }
static void test_find_sync_committee_big_stale_period_panics() { find_sync_committee_big(LC633__FINALIZED_SLOT - 8192, LC634__ATTESTED_SLOT, true); }
static void update_validity_big(uint64_t cur_slot, uint64_t finalized_slot, uint64_t participation) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  UpdateValidityBigTarget t = add_virtual_update_validity_target_big(builder);
  auto data = builder.build();
  PartialWitness pw;
  set_biguint_target(pw, t.cur_slot_big, biguint_from_u64(cur_slot));
  set_biguint_target(pw, t.finalized_slot_big, biguint_from_u64(finalized_slot));
  set_biguint_target(pw, t.participation_big, biguint_from_u64(participation));
  prove_and_verify(*data, pw);
}
static void test_update_validity_big() { update_validity_big(LC633__FINALIZED_SLOT, LC634__FINALIZED_SLOT, 428); }
static void test_update_validity_big_finalized_before_current_panics() { update_validity_big(LC634__FINALIZED_SLOT, LC633__FINALIZED_SLOT, 428); }
static void test_update_validity_big_threshold_not_exceeded_panics() { update_validity_big(1, 2, FINALITY_THRESHOLD); }

// ---- the builder primitives the recursive verifier is made of, against native values: is_equal / inverse / and / or, one
// PoseidonGate row with and without the swap, hash_n_to_hash_no_pad and a Merkle path against the oracle's Poseidon
static void builder_primitives(bool break_it) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  Target a = builder.add_virtual_target(), b = builder.add_virtual_target();
  BoolTarget eq_ab = builder.is_equal(a, b), eq_aa = builder.is_equal(a, a);
  Target inv = builder.inverse(a);
  BoolTarget o = builder.or_(eq_ab, eq_aa), n = builder.and_(eq_ab, eq_aa);
  std::array<Target, 12> st;
  for (auto &t : st) t = builder.add_virtual_target();
  BoolTarget sw = builder.add_virtual_bool_target_safe();
  std::array<Target, 12> out0 = builder.poseidon(st), out1 = builder.poseidon(st, sw);
  std::vector<Target> msg;
  for (int i = 0; i < 19; i++) msg.push_back(builder.add_virtual_target());
  std::array<Target, 4> h = hash_n_to_hash_no_pad(builder, msg);
  for (Target t : {eq_ab.target, eq_aa.target, inv, o.target, n.target}) builder.register_public_input(t);
  for (Target t : out0) builder.register_public_input(t);
  for (Target t : out1) builder.register_public_input(t);
  for (Target t : h) builder.register_public_input(t);
  auto data = builder.build();
  PartialWitness pw;
  const F av = 0x1234567890abcdefull % GOLDILOCKS_P, bv = 77;
  pw.set_target(a, av); pw.set_target(b, bv);
  uint64_t s0[12], s1[12], m[19], want_h[4];
  for (int i = 0; i < 12; i++) { s0[i] = (0x9e3779b97f4a7c15ull * (i + 3)) % GOLDILOCKS_P; pw.set_target(st[i], s0[i]); }
  for (int i = 0; i < 12; i++) s1[i] = i < 4 ? s0[i + 4] : i < 8 ? s0[i - 4] : s0[i];  // the swap exchanges the two digests
  pw.set_bool_target(sw, true);
  for (int i = 0; i < 19; i++) { m[i] = (0xc2b2ae3d27d4eb4full * (i + 1)) % GOLDILOCKS_P; pw.set_target(msg[i], m[i]); }
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  data->generate_witness(pw, wires, pis);
  orc_poseidon_permute(s0); orc_poseidon_permute(s1);
  orc_hash_no_pad(m, 19, want_h);
  unsigned __int128 prod = (unsigned __int128)pis[2] * av % GOLDILOCKS_P;
  bool ok = pis[0] == 0 && pis[1] == 1 && prod == 1 && pis[3] == 1 && pis[4] == 0;
  for (int i = 0; i < 12; i++) ok = ok && pis[5 + i] == s0[i] && pis[17 + i] == s1[i];
  for (int i = 0; i < 4; i++) ok = ok && pis[29 + i] == want_h[i];
  if (!ok) throw std::runtime_error("builder primitives: a public input differs from the native value");
  if (break_it) {  // inverse(0) has no witness
    PartialWitness bad;
    bad.set_target(a, 0); bad.set_target(b, bv);
    for (int i = 0; i < 12; i++) bad.set_target(st[i], 1);
    bad.set_bool_target(sw, false);
    for (int i = 0; i < 19; i++) bad.set_target(msg[i], 2);
    prove_and_verify(*data, bad);
    return;
  }
  prove_and_verify(*data, pw);
}
static void test_builder_primitives() { builder_primitives(false); }
static void test_builder_inverse_of_zero_panics() { builder_primitives(true); }

// ---- the recursive verifier (src/targets.rs:468-482, src/main.rs:172-176: add_virtual_proof_with_pis + verify_proof of an inner
// proof whose public inputs are connected into the outer circuit; the reference's inner proof is the BLS-signature verifier,
// which does not exist here: the inner circuit below is a stand-in with the same interface - a proof with public inputs)
// inner circuit: public inputs (x, y, x * y + x, low 16 bits of y recomposed) and, optionally, one two_to_one_sha256
static InnerProof prove_inner(bool with_sha, F x_val, F y_val) {
  InnerProof in;
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  Target x = builder.add_virtual_target(), y = builder.add_virtual_target();
  Target z = builder.mul_add(x, y, x);
  std::vector<BoolTarget> bits = builder.split_le(y, 20);
  Target low = builder.le_sum(bits, 0, 16);
  builder.register_public_input(x); builder.register_public_input(y); builder.register_public_input(z); builder.register_public_input(low);
  Hash256Target l, r;
  if (with_sha) {
    l = builder.add_virtual_hash256_target(); r = builder.add_virtual_hash256_target();
    Hash256Target d = builder.two_to_one_sha256(l, r);
    for (int i = 0; i < 8; i++) builder.register_public_input(d[i].t);
  }
  in.data = builder.build();
  PartialWitness pw;
  pw.set_target(x, x_val); pw.set_target(y, y_val);
  if (with_sha) { pw.set_hash256_target(l, ZERO_ROOT_2); pw.set_hash256_target(r, ZERO_ROOT_4); }
  prove_standalone(in, pw);
  return in;
}
// After a word that enters the Fiat-Shamir transcript has been changed, the old proof-of-work witness no longer fits and the
// in-circuit PoW check would be the one to fail.  To show that the check the word belongs to fails too, the transcript is replayed
// natively (the host helpers of the C ABI, in the order of csrc/verifier.hip) and a fitting witness is searched, as a cheating
// prover would do.
static void refit_pow_witness(const CommonCircuitData &c, const uint64_t digest[4], ProofWithPublicInputs &p) {
  lcp2_proof_layout L;
  lcp2_proof_layout_of(&c.params, &L);
  const lcp2_params &P = c.params;
  const size_t CH = P.num_challenges, npp = (P.num_routed_wires + P.quotient_degree_factor - 1) / P.quotient_degree_factor - 1;
  uint64_t pi_hash[4], tmp[8];
  lcp2_hash_no_pad(p.public_inputs.data(), p.public_inputs.size(), pi_hash);
  lcp2_challenger ch;
  lcp2_challenger_init(&ch);
  const uint64_t *w = p.proof.data();
  lcp2_challenger_observe(&ch, digest, 4);
  lcp2_challenger_observe(&ch, pi_hash, 4);
  lcp2_challenger_observe(&ch, w + L.wires_cap, L.cap_words);
  lcp2_challenger_get(&ch, tmp, 2 * CH);
  lcp2_challenger_observe(&ch, w + L.zs_cap, L.cap_words);
  lcp2_challenger_get(&ch, tmp, CH);
  lcp2_challenger_observe(&ch, w + L.quot_cap, L.cap_words);
  lcp2_challenger_get(&ch, tmp, 2);
  lcp2_challenger_observe(&ch, w + L.op_constants, 2 * (P.num_constants + P.num_routed_wires + P.num_wires));
  lcp2_challenger_observe(&ch, w + L.op_zs, 2 * CH);
  lcp2_challenger_observe(&ch, w + L.op_partial_products, 2 * CH * npp);
  lcp2_challenger_observe(&ch, w + L.op_quotient, 2 * CH * P.quotient_degree_factor);
  lcp2_challenger_observe(&ch, w + L.op_zs_next, 2 * CH);
  lcp2_challenger_get(&ch, tmp, 2);
  for (uint32_t l = 0; l < P.num_fri_layers; l++) { lcp2_challenger_observe(&ch, w + L.fri_caps + l * L.cap_words, L.cap_words); lcp2_challenger_get(&ch, tmp, 2); }
  lcp2_challenger_observe(&ch, w + L.final_poly, 2 * L.final_len);
  for (uint64_t cand = 0; cand < (1ull << 24); cand++) {
    lcp2_challenger t = ch;
    uint64_t resp;
    lcp2_challenger_observe(&t, &cand, 1);
    lcp2_challenger_get(&t, &resp, 1);
    if ((resp >> (64 - P.proof_of_work_bits)) == 0) { p.proof[L.pow_witness] = cand; return; }
  }
  throw std::runtime_error("no proof-of-work witness found");
}

// outer circuit: verify_proof(inner) with the inner public inputs re-exported; `tamper`: the word of the inner proof to corrupt
static void recursive_verifier(bool with_sha, bool constant_vd, long tamper, bool wrong_public_input = false, bool wrong_digest = false) {
  InnerProof in = prove_inner(with_sha, 123456789, 0xABCDE);
  const CommonCircuitData common = CommonCircuitData::of(in.data->description());
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  ProofWithPublicInputsTarget pt = add_virtual_proof_with_pis(builder, common);
  VerifierCircuitTarget vd = constant_vd ? constant_verifier_data(builder, in.digest, in.cap) : add_virtual_verifier_data(builder, common.params.cap_height);
  verify_proof(builder, pt, vd, common);
  for (Target t : pt.public_inputs) builder.register_public_input(t);
  const size_t rows = builder.num_gates();
  auto data = builder.build();
  printf("recursive verifier of a 2^%u-row proof (%zu words): %zu gates, 2^%u rows\n", common.params.degree_bits, pt.proof.size(), rows, data->degree_bits());
  ProofWithPublicInputs p = in.proof;
  lcp2_proof_layout L;
  lcp2_proof_layout_of(&common.params, &L);
  if (tamper >= 0) {
    const size_t where[] = {L.op_wires + 3, L.quot_cap + 1, L.queries + L.q_init_off[1] + 7, L.queries + L.query_words + L.q_step_off[0] + 2, L.final_poly, L.pow_witness,
                            L.queries + 2 * L.query_words + L.q_init_off[0] + L.q_init_cols[0] + 5};
    size_t w = where[tamper];
    p.proof[w] = p.proof[w] == 5 ? 6 : 5;
  }
  if (wrong_public_input) p.public_inputs[2] += 1;
  uint64_t dg[4] = {in.digest[0], in.digest[1], in.digest[2], in.digest[3]};
  if (wrong_digest) dg[1] ^= 1;
  // words of the transcript: refit the PoW witness (except in the test of the PoW check itself), so that the failure below is
  // the vanishing identity / Merkle / FRI check the word belongs to and not the proof of work
  const bool in_transcript = tamper == 0 || tamper == 1 || tamper == 4 || wrong_public_input || wrong_digest;
  if (in_transcript) refit_pow_witness(common, dg, p);
  PartialWitness pw;
  set_proof_with_pis_target(pw, pt, p);
  if (!constant_vd) set_verifier_data_target(pw, vd, dg, in.cap);
  InnerProof outer;
  try {
    prove_and_verify(*data, pw, &outer);
  } catch (const UnsatisfiedError &e) {
    const bool pow_failed = std::string(e.what()).find("split_le: value does not fit in 16 bits") != std::string::npos;
    if (pow_failed != (tamper == 5)) throw std::runtime_error(std::string("the wrong check failed: ") + e.what());
    throw;
  }
  // test_recursive_verifier's outer circuit, read at commit b984159 (before csrc/gate_program.hpp walked the programs); the
  // standard config in both modes, so one circuit
  static const CircuitPin pin = {{0x6fc2806b7e9f54a2ull, 0xf35328caee2a9c7aull, 0x3011123612b5f45aull, 0xc5ba53fe48a16283ull}, 13, 5403};
  if (!with_sha && !constant_vd) expect_circuit("recursive verifier", pin, outer.digest, data->degree_bits(), rows);
}
static void test_recursive_verifier() { recursive_verifier(false, false, -1); }
static void test_recursive_verifier_constant_verifier_data_sha_inner() { recursive_verifier(true, true, -1); }
static void test_recursive_verifier_tampered_opening_panics() { recursive_verifier(false, false, 0); }
static void test_recursive_verifier_tampered_cap_panics() { recursive_verifier(false, false, 1); }
static void test_recursive_verifier_tampered_leaf_panics() { recursive_verifier(false, false, 2); }
static void test_recursive_verifier_tampered_fri_layer_panics() { recursive_verifier(false, false, 3); }
static void test_recursive_verifier_tampered_final_poly_panics() { recursive_verifier(false, false, 4); }
static void test_recursive_verifier_tampered_pow_panics() { recursive_verifier(false, false, 5); }
static void test_recursive_verifier_tampered_sibling_panics() { recursive_verifier(false, false, 6); }
static void test_recursive_verifier_wrong_public_input_panics() { recursive_verifier(false, false, -1, true); }
static void test_recursive_verifier_wrong_digest_panics() { recursive_verifier(false, false, -1, false, true); }

// ---- shrinking a proof by recursion (plonky2's test_size_optimized_recursion, as examples/lc_prover --shrink and lch_wrap_create do
// it): inner proof -> wrap under `first` -> wrap of that under `second`.  Every level goes through prove_and_verify, i.e. through
// the oracle: its row-wise check of every gate, its prover at rate_bits 7 / 8 with quotient_degree_factor 8 (the quotient on the
// first 8 n points of a 128 n / 256 n LDE) and its verifier.
static CircuitConfig shrink_config(uint32_t rate_bits, uint32_t cap_height, uint32_t proof_of_work_bits, uint32_t num_query_rounds) {
  CircuitConfig cfg = CircuitConfig::standard_recursion_config();
  cfg.rate_bits = rate_bits; cfg.cap_height = cap_height; cfg.proof_of_work_bits = proof_of_work_bits; cfg.num_query_rounds = num_query_rounds;
  return cfg;
}
// gpu mode: the product's build_wrap_circuit (verifier data from the attached inner circuit).  cpu mode: no device holds the inner
// circuit, so the same circuit is put together from the same public pieces with the ORACLE's digest and cap as the constants.
static WrapCircuit wrap_circuit_of(const CircuitConfig &cfg, const CircuitData &inner_data, const InnerProof &inner) {
  if (g_gpu) return build_wrap_circuit(cfg, inner_data);
  const CommonCircuitData common = CommonCircuitData::of(inner_data.description());
  CircuitBuilder builder(cfg);
  WrapCircuit w;
  w.inner_proof = add_virtual_proof_with_pis(builder, common);
  const VerifierCircuitTarget vd = constant_verifier_data(builder, inner.digest, inner.cap);
  verify_proof(builder, w.inner_proof, vd, common);
  for (Target t : w.inner_proof.public_inputs) builder.register_public_input(t);
  w.num_gates = builder.num_gates();
  w.data = builder.build();
  return w;
}
static void wrap_chain(const CircuitConfig &first, const CircuitConfig &second, bool tamper_second_inner) {
  InnerProof in = prove_inner(false, 123456789, 0xABCDE);
  const std::vector<F> want_pis = in.proof.public_inputs;
  const CircuitConfig cfgs[2] = {first, second};
  std::unique_ptr<CircuitData> keep[2];
  const CircuitData *inner_data = in.data.get();
  InnerProof level;  // proof, digest and cap of the level below
  level.proof = in.proof; memcpy(level.digest, in.digest, 32); level.cap = in.cap;
  for (int k = 0; k < 2; k++) {
    const auto t0 = std::chrono::steady_clock::now();
    WrapCircuit w = wrap_circuit_of(cfgs[k], *inner_data, level);
    const lcp2_params &P = w.data->description().params;
    if (P.rate_bits != cfgs[k].rate_bits || P.cap_height != cfgs[k].cap_height || P.num_query_rounds != cfgs[k].num_query_rounds || P.quotient_degree_factor != 8)
      throw std::runtime_error("wrap circuit: parameters are not the shrinking config's");
    ProofWithPublicInputs fed = level.proof;
    if (tamper_second_inner && k == 1) {  // a Merkle leaf word of the first query of the rate-7 proof: outside the transcript
      lcp2_proof_layout L;
      lcp2_proof_layout_of(&inner_data->description().params, &L);
      const size_t at = L.queries + L.q_init_off[1] + 7;
      fed.proof[at] = fed.proof[at] == 5 ? 6 : 5;
    }
    PartialWitness pw;
    set_wrap_witness(pw, w, fed);
    InnerProof next;
    prove_and_verify(*w.data, pw, &next);
    if (next.proof.public_inputs != want_pis) throw std::runtime_error("wrap " + std::to_string(k + 1) + ": public inputs differ from the inner proof's");
    // the two wrap circuits of cpu mode (rate_bits 4 and 5), read at commit b984159 like the pin in recursive_verifier; gpu mode
    // wraps at rates 7 and 8, other circuits, which only the GPU can commit to
    static const CircuitPin pins[2] = {{{0xd58e2c971bcdd9a4ull, 0x8131fd401571619cull, 0x0fc6b335df883911ull, 0x85e796ce0a435694ull}, 13, 5437},
                                       {{0xfe3f76810bd61bb3ull, 0xa91ddb60224bfacbull, 0x08c07c487c36f660ull, 0x004b4ea9e4b7d990ull}, 13, 4474}};
    if (!g_gpu) expect_circuit("wrap " + std::to_string(k + 1), pins[k], next.digest, w.data->degree_bits(), w.num_gates);
    printf("wrap %d: rate_bits %u cap_height %u, %zu gates, 2^%u rows, %zu -> %zu proof words, %lld s\n", k + 1, P.rate_bits, P.cap_height, w.num_gates,
           w.data->degree_bits(), level.proof.proof.size(), next.proof.proof.size(),
           (long long)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0).count());
    keep[k] = std::move(w.data);
    inner_data = keep[k].get();
    level.proof = next.proof; memcpy(level.digest, next.digest, 32); level.cap = next.cap;
  }
}
// gpu mode: plonky2's two shrinking configs, rate_bits 7 and 8.  cpu mode: the same cap heights, PoW bits and query counts at the
// lighter rates 4 and 5 (still quotient_degree_factor 8 = 2^3 below 2^rate_bits, the quotient on the first 8 n points of a 16 n /
// 32 n LDE), because the oracle is the only CPU prover: measured on 8 threads, test_wrap_chain in cpu mode takes 375 s at rates 7
// and 8 (168 s + 202 s for the two 2^13-row wraps) and 44 s at rates 4 and 5 (15 s + 27 s).
static CircuitConfig wrap_first() { return shrink_config(g_gpu ? 7 : 4, 4, 16, 12); }
static CircuitConfig wrap_second() { return shrink_config(g_gpu ? 8 : 5, 0, 20, 10); }
static void test_wrap_chain() { wrap_chain(wrap_first(), wrap_second(), false); }
static void test_wrap_chain_tampered_inner_panics() { wrap_chain(wrap_first(), wrap_second(), true); }

// the outputs-only generator of a PoseidonGate row (what generate_witness_gpu runs on the host; the row itself is filled on the device)
// against the full row generator and the oracle's permutation, swap included, non-canonical inputs included; and the full row
// generator (the AVX2 MDS layer where the CPU has it) against the text it shares with the device (csrc/pos_rows.hpp) run with the
// portable layer pos_mds, every one of the 135 cells.  Six statements of the permutation must agree word for word: the host's grouped
// walk with the portable layers and with the AVX2 layers, the plain definition pos_permute_portable, the row text, poseidon_gate_row,
// the oracle.  Inputs: the edge words rotated through all 12 positions, all 2^64 - 1, all zero (each with both
// swap flags), then the random draws.
static void test_poseidon_gate_outputs_match_rows() {
  static lcp2::u64 rc[lcp2::POS_ROUNDS * lcp2::POS_W];
  lcp2::pos_derive_round_constants(rc);
  uint64_t seed = 12345;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; uint64_t z = seed; z ^= z >> 29; z *= 0xBF58476D1CE4E5B9ull; return z ^ (z >> 32); };
  const F P = GOLDILOCKS_P, edge[8] = {0, 1, P - 1, P, P + 1, 0xFFFFFFFFull, 1ull << 32, ~0ull};
  const int edge_cases = 2 * (12 + 2);
  for (int t = -edge_cases; t < 500; t++) {
    F in[12], row[POS_GATE_WIRES], out[12];
    const int e = (t + edge_cases) / 2;  // edge case e < 14 with swap = 0 and 1
    for (int i = 0; i < 12; i++) in[i] = t < 0 ? (e < 12 ? edge[(i + e) % 8] : e == 12 ? ~0ull : 0) : t < 4 ? (t == 0 ? 0 : t == 1 ? P - 1 : ~0ull) : rnd();
    const bool swap = t & 1;
    F out_portable[12];
    poseidon_gate_row(in, swap, row);
    lcp2::u64 x[12], shared[POS_GATE_WIRES];
    uint32_t stores = 0;
    for (int i = 0; i < 12; i++) x[i] = in[i];
    for (auto &c : shared) c = ~0ull;
    lcp2::pos_row_cells(x, swap, rc, [](lcp2::u64 *s) { lcp2::pos_mds(s); }, [&](lcp2::u32 col, lcp2::u64 v) { shared[col] = v; stores++; });
    if (stores != POS_GATE_WIRES) throw std::runtime_error("pos_row_cells does not store 135 cells");
    for (uint32_t c = 0; c < POS_GATE_WIRES; c++)
      if (row[c] != shared[c]) throw std::runtime_error("poseidon_gate_row differs from the shared row text at case " + std::to_string(t) + ", column " + std::to_string(c));
    poseidon_gate_outputs(in, swap, out);                         // the grouped walk, AVX2 layers where the CPU has them
    poseidon_gate_outputs_impl(in, swap, out_portable, true);     // the grouped walk, 128-bit multiply-accumulates
    for (int i = 0; i < 12; i++) if (out[i] != out_portable[i]) throw std::runtime_error("poseidon_gate_outputs: AVX2 and portable paths differ at case " + std::to_string(t));
    uint64_t s[12];
    lcp2::u64 plain[12];
    for (int i = 0; i < 12; i++) s[i] = in[i] % GOLDILOCKS_P;
    if (swap) for (int i = 0; i < 4; i++) std::swap(s[i], s[i + 4]);
    for (int i = 0; i < 12; i++) plain[i] = s[i];
    lcp2::pos_permute_portable(plain, rc);                        // the plain definition
    orc_poseidon_permute(s);
    for (int i = 0; i < 12; i++)
      if (row[POS_WIRE_OUTPUT + i] != out[i] || out[i] != s[i] || plain[i] != s[i])
        throw std::runtime_error("poseidon_gate_outputs differs from the row generator / the plain definition / the oracle at case " + std::to_string(t));
  }
}

struct TestCase { const char *name; std::function<void()> fn; bool should_panic; bool gpu_only = false; };
static const TestCase TESTS[] = {
    {"test_merkle_root_2_leaves", test_merkle_root_2_leaves, false},
    {"test_merkle_root_4_leaves", test_merkle_root_4_leaves, false},
    {"test_merkle_root_8_leaves", test_merkle_root_8_leaves, false},
    {"test_merkle_root_16_leaves", test_merkle_root_16_leaves, false},
    {"test_merkle_root_wrong_root_panics", test_merkle_root_wrong_root_panics, true},
    {"test_signing_root", test_signing_root, false},
    {"test_beacon_block_header", test_beacon_block_header, false},
    {"test_verify_finality_branch", test_verify_finality_branch, false},
    {"test_contract_state", test_contract_state, false},
    {"test_verify_sync_committee_branch", test_verify_sync_committee_branch, false},
    {"test_verify_sync_committee_branch_panics", test_verify_sync_committee_branch_panics, true},
    {"test_read_u32_be_public_input", test_read_u32_be_public_input, false},
    {"test_ssz_sync_committee", test_ssz_sync_committee, false},
    {"test_light_client_update", test_light_client_update, false},
    {"test_light_client_update_bad_state_root_panics", test_light_client_update_bad_state_root_panics, true},
    {"test_light_client_update_low_participation_panics", test_light_client_update_low_participation_panics, true},
    {"test_light_client_update_with_recursive_proof", test_light_client_update_with_recursive_proof, false},
    {"test_light_client_update_recursive_proof_of_other_bits_panics", test_light_client_update_recursive_proof_of_other_bits_panics, true},
    {"test_find_sync_committee_current_period", test_find_sync_committee_current_period, false},
    {"test_find_sync_committee_next_period", test_find_sync_committee_next_period, false},
    {"test_find_sync_committee_stale_period_panics", test_find_sync_committee_stale_period_panics, true},
    {"test_find_sync_committee_previous_period_panics", test_find_sync_committee_previous_period_panics, true},
    {"test_slot_connect_rejects_wide_encoding_panics", test_slot_connect_rejects_wide_encoding_panics, true},
    {"test_update_validity", test_update_validity, false},
    {"test_update_validity_equal_slots_and_343", test_update_validity_equal_slots_and_343, false},
    {"test_update_validity_finalized_before_current_panics", test_update_validity_finalized_before_current_panics, true},
    {"test_update_validity_threshold_not_exceeded_panics", test_update_validity_threshold_not_exceeded_panics, true},
    {"test_biguint_arithmetic", test_biguint_arithmetic, false},
    {"test_biguint_arithmetic_all_ones", test_biguint_arithmetic_all_ones, false},
    {"test_biguint_division_by_zero_panics", test_biguint_division_by_zero_panics, true},
    {"test_biguint_hash256_connect", test_biguint_hash256_connect, false},
    {"test_find_sync_committee_big_current_period", test_find_sync_committee_big_current_period, false},
    {"test_find_sync_committee_big_next_period", test_find_sync_committee_big_next_period, false},
    {"test_find_sync_committee_big_stale_period_panics", test_find_sync_committee_big_stale_period_panics, true},
    {"test_update_validity_big", test_update_validity_big, false},
    {"test_update_validity_big_finalized_before_current_panics", test_update_validity_big_finalized_before_current_panics, true},
    {"test_update_validity_big_threshold_not_exceeded_panics", test_update_validity_big_threshold_not_exceeded_panics, true},
    {"test_poseidon_gate_outputs_match_rows", test_poseidon_gate_outputs_match_rows, false},
    {"test_builder_primitives", test_builder_primitives, false},
    {"test_builder_inverse_of_zero_panics", test_builder_inverse_of_zero_panics, true},
    {"test_recursive_verifier", test_recursive_verifier, false},
    {"test_recursive_verifier_constant_verifier_data_sha_inner", test_recursive_verifier_constant_verifier_data_sha_inner, false},
    {"test_recursive_verifier_tampered_opening_panics", test_recursive_verifier_tampered_opening_panics, true},
    {"test_recursive_verifier_tampered_cap_panics", test_recursive_verifier_tampered_cap_panics, true},
    {"test_recursive_verifier_tampered_leaf_panics", test_recursive_verifier_tampered_leaf_panics, true},
    {"test_recursive_verifier_tampered_fri_layer_panics", test_recursive_verifier_tampered_fri_layer_panics, true},
    {"test_recursive_verifier_tampered_final_poly_panics", test_recursive_verifier_tampered_final_poly_panics, true},
    {"test_recursive_verifier_tampered_pow_panics", test_recursive_verifier_tampered_pow_panics, true},
    {"test_recursive_verifier_tampered_sibling_panics", test_recursive_verifier_tampered_sibling_panics, true},
    {"test_recursive_verifier_wrong_public_input_panics", test_recursive_verifier_wrong_public_input_panics, true},
    {"test_recursive_verifier_wrong_digest_panics", test_recursive_verifier_wrong_digest_panics, true},
    {"test_wrap_chain", test_wrap_chain, false},
    {"test_wrap_chain_tampered_inner_panics", test_wrap_chain_tampered_inner_panics, true},
    {"test_real_gadget_circuit_2p22", test_real_gadget_circuit_2p22, false, true},
};

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <cpu|gpu> <test|all|list>\n", argv[0]); return 2; }
  g_gpu = std::string(argv[1]) == "gpu";
  std::string which = argv[2];
  if (which == "list") { for (auto &t : TESTS) if (!t.gpu_only) printf("%s\n", t.name); return 0; }
  if (which == "list-gpu-only") { for (auto &t : TESTS) if (t.gpu_only) printf("%s\n", t.name); return 0; }
  if (g_gpu) {
    int rc = lcp2_ctx_create(0, nullptr, &g_ctx);
    if (rc != LCP2_OK) { fprintf(stderr, "lcp2_ctx_create: %s\n", lcp2_status_str(rc)); return 3; }
  }
  int failures = 0, ran = 0;
  for (auto &t : TESTS) {
    if (which != "all" && which != t.name) continue;
    if (t.gpu_only && !g_gpu) continue;
    ran++;
    bool panicked = false;
    std::string msg;
    try { t.fn(); } catch (const UnsatisfiedError &e) { panicked = true; msg = std::string("UnsatisfiedError: ") + e.what(); }
    catch (const std::exception &e) { panicked = true; msg = e.what(); if (!t.should_panic) msg = "UNEXPECTED: " + msg; }
    bool ok = panicked == t.should_panic && (t.should_panic ? msg.rfind("UnsatisfiedError", 0) == 0 : true);
    printf("test %s ... %s%s%s\n", t.name, ok ? "ok" : "FAILED", msg.empty() ? "" : " -- ", msg.c_str());
    if (!ok) failures++;
  }
  if (g_ctx) lcp2_ctx_destroy(g_ctx);
  if (!ran) { fprintf(stderr, "no such test\n"); return 2; }
  return failures ? 1 : 0;
}
