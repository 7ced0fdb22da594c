// K6's half tier on the light-client gate set of the host layer (host/gates.cpp: the four SHA-256 gates, three selector groups).
// usage: test_tiers degrees                 host only: "<gate> <derived degree> <GATE_DEGREE>" for every gate of build_gate_set
//        test_tiers prove <tiny|sha>         GPU: the circuit's gate -> bundle map, then the proof with the tiers on, with
//                                            LCP2_QUOTIENT_TIERS=0 and from the oracle, compared word for word; then the caps of the
//                                            lcp2_commit_wires / lcp2_perm_zs / lcp2_quotient seams under forced challenges with
//                                            alpha = (0, 1), both ways, against orc_prove_forced
//   tiny: a few arithmetic rows and public inputs (the smallest circuit the builder makes; every gate kernel of the set still runs
//         at every point); sha: one two_to_one_sha256 (310 rows: 2^9, the smallest circuit with SHA rows)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include "../../eth-lc-plonky2_amd/host/gadgets.hpp"
#include "../../eth-lc-plonky2_amd/host/host_internal.hpp"
#include "../../oracle/oracle.h"
#include "../../oracle/plonk.h"
#include "golden_data.hpp"

using namespace lc;

static void need(bool ok, const std::string &what) { if (!ok) throw std::runtime_error(what); }

static int degrees() {
  const GateSetLayout gs = build_gate_set(9);
  for (uint32_t g = 0; g < gs.gates.size(); g++) {
    uint32_t d = ~0u;
    const int rc = lcp2_gate_program_degree(gs.code.data() + 2 * (size_t)gs.gates[g].code_offset, gs.gates[g].code_len, gs.num_regs, &d);
    if (rc != LCP2_OK) { printf("lcp2_gate_program_degree failed for %s: %d\n", gate_name(g), rc); return 1; }
    printf("degree %s %u %u\n", gate_name(g), d, GATE_DEGREE[g]);
  }
  return 0;
}

static std::unique_ptr<CircuitData> make_circuit(const std::string &which, PartialWitness &pw) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  if (which == "tiny") {
    Target x = builder.add_virtual_target(), y = builder.add_virtual_target();
    Target z = builder.mul_add(x, y, x);
    Target w = builder.mul(z, builder.add_const(y, 11));
    builder.register_public_input(z);
    builder.register_public_input(w);
    builder.register_public_input(builder.constant(77));
    pw.set_target(x, 3);
    pw.set_target(y, 0xFFFFFFFF00000000ull);
    return builder.build();
  }
  MerkleTreeSha256Target tree = add_virtual_merkle_tree_sha256_target(builder, 1);
  Hash256Target expected = builder.add_virtual_hash256_target();
  builder.connect_hash256(tree.root, expected);
  for (int i = 0; i < 8; i++) builder.register_public_input(expected[i].t);
  std::vector<std::array<uint8_t, 32>> leaves(2);
  for (auto &l : leaves) l.fill(0);
  set_partial_merkle_tree_sha256_target(pw, leaves, tree);
  pw.set_hash256_target(expected, ZERO_ROOT_2);
  return builder.build();
}

static lcp2_circuit *create(lcp2_ctx *ctx, const CircuitDescription &D, bool tiers) {
  if (tiers) unsetenv("LCP2_QUOTIENT_TIERS"); else setenv("LCP2_QUOTIENT_TIERS", "0", 1);
  lcp2_circuit_desc cd = D.c_desc();
  lcp2_circuit *c = nullptr;
  const int rc = lcp2_circuit_create(ctx, &cd, &c);
  unsetenv("LCP2_QUOTIENT_TIERS");
  need(rc == LCP2_OK, std::string("lcp2_circuit_create: ") + lcp2_last_error(ctx));
  return c;
}

static int prove(const std::string &which) {
  lcp2_ctx *ctx = nullptr;
  need(lcp2_ctx_create(0, nullptr, &ctx) == LCP2_OK, "lcp2_ctx_create");
  PartialWitness pw;
  auto data = make_circuit(which, pw);
  const CircuitDescription &D = data->description();
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  data->generate_witness(pw, wires, pis);
  const lcp2_params &p = D.params;
  printf("circuit %s degree_bits %u num_selectors %u quotient_degree_factor %u\n", which.c_str(), p.degree_bits, D.num_selectors, p.quotient_degree_factor);
  orc_params op;
  memcpy(&op, &p, sizeof op);
  std::vector<orc_gate> og(D.gates.size());
  memcpy(og.data(), D.gates.data(), og.size() * sizeof(orc_gate));
  orc_circuit *oc = orc_circuit_new(&op, D.constants_sigmas.data(), D.k_is.data(), D.num_selectors, og.data(), (uint32_t)og.size(), D.code.data(),
                                    D.code.size(), D.imm.data(), D.imm.size(), D.num_public_inputs);
  need(oc != nullptr, "oracle rejected the circuit");
  uint64_t bad[2];
  need(orc_check_witness(oc, wires.data(), pis.data(), bad) == 0, "the witness violates a gate constraint");
  const size_t words = orc_proof_words(&op), capw = (size_t)4 << p.cap_height;
  std::vector<uint64_t> want(words), forced_want(words);
  need(orc_prove(oc, wires.data(), pis.data(), want.data()) == 0, "orc_prove");
  orc_challenges f{};
  const uint32_t CH = p.num_challenges;
  for (uint32_t k = 0; k < CH; k++) { f.betas[k] = 0x1234567 + 77 * k; f.gammas[k] = 0x89ABCDEF01ull + 5 * k; f.alphas[k] = k; }  // alpha = (0, 1)
  need(orc_prove_forced(oc, wires.data(), pis.data(), &f, ORC_FORCE_BETAS | ORC_FORCE_GAMMAS | ORC_FORCE_ALPHAS, forced_want.data()) == 0, "orc_prove_forced");
  uint64_t pi_hash[4];
  need(lcp2_hash_no_pad(pis.data(), pis.size(), pi_hash) == LCP2_OK, "lcp2_hash_no_pad");
  std::vector<uint64_t> proofs[2];
  for (int tiers = 1; tiers >= 0; tiers--) {
    lcp2_circuit *c = create(ctx, D, tiers != 0);
    const uint32_t ng = (uint32_t)D.gates.size();
    std::vector<uint32_t> deg(ng);
    std::vector<int32_t> bun(ng);
    need(lcp2_circuit_gate_tiers(c, ng, deg.data(), bun.data()) == LCP2_OK, "lcp2_circuit_gate_tiers");
    for (uint32_t g = 0; g < ng; g++)
      printf("tier %s %s %u %u %u %u %u %d\n", tiers ? "on" : "off", gate_name(g), D.gates[g].selector_index, D.gates[g].group_start, D.gates[g].group_end,
             D.gates[g].num_constraints, deg[g], bun[g]);
    std::vector<uint64_t> &proof = proofs[tiers];
    proof.assign(words, 0);
    need(lcp2_prove(c, wires.data(), LCP2_MEM_HOST, pis.data(), pis.size(), proof.data(), words) == LCP2_OK, std::string("lcp2_prove: ") + lcp2_last_error(ctx));
    need(proof == want, std::string("proof differs from the oracle's, tiers ") + (tiers ? "on" : "off"));
    // the seams under forced challenges: wires cap, Zs cap, quotient cap
    std::vector<uint64_t> caps(3 * capw);
    need(lcp2_commit_wires(c, wires.data(), LCP2_MEM_HOST, caps.data()) == LCP2_OK, "lcp2_commit_wires");
    need(lcp2_perm_zs(c, f.betas, f.gammas, caps.data() + capw) == LCP2_OK, "lcp2_perm_zs");
    need(lcp2_quotient(c, f.alphas, pi_hash, caps.data() + 2 * capw) == LCP2_OK, std::string("lcp2_quotient: ") + lcp2_last_error(ctx));
    need(memcmp(caps.data(), forced_want.data(), 3 * capw * 8) == 0, std::string("forced alpha = (0, 1): caps differ from the oracle's, tiers ") + (tiers ? "on" : "off"));
    need(memcmp(caps.data() + 2 * capw, want.data() + 2 * capw, capw * 8) != 0, "the forced quotient cap equals the unforced one");
    lcp2_circuit_destroy(c);
  }
  need(proofs[0] == proofs[1], "tiered and untiered proofs differ");
  printf("proofs equal: tiers on = tiers off = oracle (%zu words); forced alpha = (0, 1) caps equal both ways\n", words);
  orc_circuit_free(oc);
  lcp2_ctx_destroy(ctx);
  return 0;
}

int main(int argc, char **argv) {
  try {
    if (argc == 2 && std::string(argv[1]) == "degrees") return degrees();
    if (argc == 3 && std::string(argv[1]) == "prove") return prove(argv[2]);
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "usage: %s degrees | prove <tiny|sha>\n", argv[0]);
  return 2;
}
