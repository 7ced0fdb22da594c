// CircuitData::set_fill_copies of the host layer: with the opt-in generate_witness_gpu lists one host-written cell per variable class
// and sends the list through lcp2_witness_fill_copies; the proof must be the one made without it, word for word.
// usage: test_fill_copies gpu    ContractState (src/unit_tests.rs:169-246) and a circuit with one two_to_one_sha256: for each, a proof
//                                with the opt-in off, one with it on, one with it off again - all three equal and verified - and the
//                                number of lcp2_cell records sent per proof in both modes ("cells: <circuit> off N on M")
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include "../../eth-lc-plonky2_amd/host/gadgets.hpp"
#include "golden_data.hpp"

using namespace lc;

static void need(bool ok, const std::string &what) { if (!ok) throw std::runtime_error(what); }

static void both_modes(const char *name, CircuitData &data, const PartialWitness &pw, lcp2_ctx *ctx) {
  data.attach_gpu(ctx);
  const ProofWithPublicInputs off = data.prove(pw);
  const size_t cells_off = data.cells_sent_last();
  data.verify(off);
  data.set_fill_copies(true);
  const ProofWithPublicInputs on = data.prove(pw);
  const size_t cells_on = data.cells_sent_last();
  const ProofWithPublicInputs on_again = data.prove(pw);  // the planned list replayed
  data.set_fill_copies(false);
  const ProofWithPublicInputs off_again = data.prove(pw);
  printf("cells: %s off %zu on %zu\n", name, cells_off, cells_on);
  need(on.proof == off.proof && on.public_inputs == off.public_inputs, std::string(name) + ": the proof with the opt-in differs from the one without");
  need(on_again.proof == off.proof, std::string(name) + ": the second proof with the opt-in differs");
  need(off_again.proof == off.proof && data.cells_sent_last() == cells_off, std::string(name) + ": switching the opt-in off again does not give the first proof back");
  need(cells_on <= cells_off && cells_on > 0, std::string(name) + ": the opt-in sends more cells than the list of every bound cell");
}

static int run() {
  lcp2_ctx *ctx = nullptr;
  need(lcp2_ctx_create(0, nullptr, &ctx) == LCP2_OK, "lcp2_ctx_create");
  {
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
    both_modes("ContractState", *data, witness, ctx);
  }
  {
    // arithmetic, a bit split and one two_to_one_sha256 whose digest is public: host-written classes beside device-written rows
    CircuitBuilder builder(CircuitConfig::standard_recursion_config());
    Target x = builder.add_virtual_target(), y = builder.add_virtual_target();
    Target z = builder.mul_add(x, y, x);
    std::vector<BoolTarget> bits = builder.split_le(y, 20);
    Target low = builder.le_sum(bits, 0, 16);
    builder.register_public_input(x); builder.register_public_input(y); builder.register_public_input(z); builder.register_public_input(low);
    Hash256Target l = builder.add_virtual_hash256_target(), r = builder.add_virtual_hash256_target();
    Hash256Target d = builder.two_to_one_sha256(l, r);
    for (int i = 0; i < 8; i++) builder.register_public_input(d[i].t);
    auto data = builder.build();
    PartialWitness pw;
    pw.set_target(x, 3); pw.set_target(y, 0xABCDEull);
    pw.set_hash256_target(l, ZERO_ROOT_2); pw.set_hash256_target(r, ZERO_ROOT_4);
    both_modes("two_to_one_sha256", *data, pw, ctx);
  }
  lcp2_ctx_destroy(ctx);
  printf("test_fill_copies gpu ... ok\n");
  return 0;
}

int main(int argc, char **argv) {
  try {
    if (argc == 2 && std::string(argv[1]) == "gpu") return run();
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "usage: %s gpu\n", argv[0]);
  return 2;
}
