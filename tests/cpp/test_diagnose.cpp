// CircuitData::diagnose / diagnose_witness / describe_report of the host layer on the smallest circuit the builder makes, with one
// broken ArithmeticGate row.  The oracle's orc_check_witness says what is wrong (count, row, constraint).
// usage: test_diagnose cpu    no device: the text of the report the oracle's finding makes names the gate by the builder's name and
//                             the row; without attach_gpu the two calls that need the device say so (std::runtime_error)
//        test_diagnose gpu    attach_gpu, then diagnose_witness on the broken witness (lcp2_check_witness on the device) names the
//                             oracle's row, gate and constraint and a copy constraint; diagnose(pw) of the clean witness finds nothing;
//                             the proof made afterwards verifies
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include "../../eth-lc-plonky2_amd/host/gadgets.hpp"
#include "../../eth-lc-plonky2_amd/host/host_internal.hpp"
#include "../../oracle/oracle.h"
#include "../../oracle/plonk.h"

using namespace lc;

static void need(bool ok, const std::string &what) { if (!ok) throw std::runtime_error(what); }
static bool has(const std::string &text, const std::string &part) { return text.find(part) != std::string::npos; }

static int run(bool gpu) {
  CircuitBuilder builder(CircuitConfig::standard_recursion_config());
  PartialWitness pw;
  Target x = builder.add_virtual_target(), y = builder.add_virtual_target();
  Target z = builder.mul_add(x, y, x);
  Target w = builder.mul(z, builder.add_const(y, 11));
  builder.register_public_input(z);
  builder.register_public_input(w);
  pw.set_target(x, 3);
  pw.set_target(y, 0xFFFFFFFF00000000ull);
  auto data = builder.build();
  const CircuitDescription &D = data->description();
  const lcp2_params &p = D.params;
  const size_t n = (size_t)1 << p.degree_bits;
  std::vector<uint64_t> wires;
  std::vector<F> pis;
  data->generate_witness(pw, wires, pis);

  orc_params op;
  memcpy(&op, &p, sizeof op);
  std::vector<orc_gate> og(D.gates.size());
  memcpy(og.data(), D.gates.data(), og.size() * sizeof(orc_gate));
  orc_circuit *oc = orc_circuit_new(&op, D.constants_sigmas.data(), D.k_is.data(), D.num_selectors, og.data(), (uint32_t)og.size(), D.code.data(),
                                    D.code.size(), D.imm.data(), D.imm.size(), D.num_public_inputs);
  need(oc != nullptr, "oracle rejected the circuit");
  uint64_t bad[2] = {0, 0};
  need(orc_check_witness(oc, wires.data(), pis.data(), bad) == 0, "the clean witness violates a gate constraint");

  // one broken ArithmeticGate row: the output of its first operation
  const std::vector<uint32_t> &gate_of_row = data->impl_for_tools()->gate_of_row;
  size_t row = n;
  for (size_t r = 0; r < gate_of_row.size() && row == n; r++)
    if (gate_of_row[r] == G_ARITHMETIC) row = r;
  need(row < n, "the circuit has no ArithmeticGate row");
  std::vector<uint64_t> broken = wires;
  broken[3 * n + row] = (broken[3 * n + row] + 1) % GOLDILOCKS_P;
  const size_t count = orc_check_witness(oc, broken.data(), pis.data(), bad);
  need(count > 0 && bad[0] == row, "the changed cell does not break its row");
  const std::string want = "row " + std::to_string(row) + ", gate ArithmeticGate, constraint " + std::to_string(bad[1]) + " (" + std::to_string(count) +
                           " gate constraints violated)";

  if (!gpu) {
    lcp2_witness_report r{};
    r.gate_violations = count; r.gate_row = bad[0]; r.gate_constraint = (uint32_t)bad[1]; r.gate_index = gate_of_row[row];
    r.copy_row = r.copy_to_row = ~0ull; r.copy_to_wire = 0xFFFFFFFFu;
    std::string text = data->describe_report(r);
    printf("diagnose: %s\n", text.c_str());
    need(text == want, "describe_report: unexpected text");
    r.copy_violations = 2; r.copy_row = row; r.copy_wire = 3; r.copy_to_row = row + 1; r.copy_to_wire = 0;
    text = data->describe_report(r);
    printf("diagnose: %s\n", text.c_str());
    need(text == want + "; copy constraint (" + std::to_string(row) + ", 3) != (" + std::to_string(row + 1) + ", 0) (2 cells)", "describe_report: unexpected copy text");
    lcp2_witness_report clean{};
    need(has(data->describe_report(clean), "satisfies every gate and copy constraint"), "describe_report: a clean report");
    for (int which = 0; which < 2; which++) {  // the device calls say that they need the device
      bool refused = false;
      try { which ? (void)data->diagnose(pw) : (void)data->diagnose_witness(broken, pis); } catch (const std::runtime_error &e) { refused = has(e.what(), "attach_gpu"); }
      need(refused, "diagnose without a device did not say that it needs attach_gpu()");
    }
  } else {
    lcp2_ctx *ctx = nullptr;
    need(lcp2_ctx_create(0, nullptr, &ctx) == LCP2_OK, "lcp2_ctx_create");
    data->attach_gpu(ctx);
    std::string text = data->diagnose_witness(broken, pis);
    printf("diagnose: %s\n", text.c_str());
    need(text.compare(0, want.size(), want) == 0, "diagnose_witness does not name the oracle's row, gate and constraint");
    need(has(text, "; copy constraint (" + std::to_string(row) + ", 3) != ("), "diagnose_witness does not name the broken copy constraint of the cell");
    text = data->diagnose_witness(wires, pis);
    need(has(text, "satisfies every gate and copy constraint"), "diagnose_witness of the clean witness: " + text);
    text = data->diagnose(pw);
    printf("diagnose: %s\n", text.c_str());
    need(has(text, "satisfies every gate and copy constraint"), "diagnose(pw) of the clean witness: " + text);
    ProofWithPublicInputs proof = data->prove(pw);
    data->verify(proof);
    need(orc_verify(oc, proof.proof.data(), proof.public_inputs.data()) == 0, "the oracle rejects the proof made after diagnose");
    data.reset();
    lcp2_ctx_destroy(ctx);
  }
  orc_circuit_free(oc);
  printf("test_diagnose %s ... ok\n", gpu ? "gpu" : "cpu");
  return 0;
}

int main(int argc, char **argv) {
  try {
    if (argc == 2 && (std::string(argv[1]) == "cpu" || std::string(argv[1]) == "gpu")) return run(std::string(argv[1]) == "gpu");
  } catch (const std::exception &e) {
    printf("FAILED: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "usage: %s cpu | gpu\n", argv[0]);
  return 2;
}
