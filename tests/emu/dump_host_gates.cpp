// TEST HARNESS (not product code): prints the gate programs of build_gate_set(9) (eth-lc-plonky2_amd/host/gates.cpp) in the text
// format of tools/gen/reference_gate_programs.txt, so that tests/test_sha_rows.py can hold the rows of tests/sha_rows_ref.py to the
// very constraints the prover checks, through tests/gate_program_ref.py:
//   gateset host <num_imm> <imm...>
//   gate <name> <flags without the native claim> <num_constraints> <code_len> <2 * code_len words>       (all numbers in hex)
// Built by the test with g++:  g++ -O1 -std=c++17 -o dump tests/emu/dump_host_gates.cpp eth-lc-plonky2_amd/host/gates.cpp
//                              eth-lc-plonky2_amd/host/poseidon_host.cpp
#include <cstdio>
#include "../../eth-lc-plonky2_amd/host/host_internal.hpp"

using namespace lc;

int main() {
  const GateSetLayout gs = build_gate_set(9);
  printf("gateset host %zx", gs.imm.size());
  for (uint64_t v : gs.imm) printf(" %llx", (unsigned long long)v);
  printf("\n");
  for (uint32_t g = 0; g < G_COUNT; g++) {
    const lcp2_gate &G = gs.gates[g];
    printf("gate %s %x %x %x", gate_name(g), G.flags & ~LCP2_GATE_NATIVE_MASK, G.num_constraints, G.code_len);
    for (size_t k = 2 * (size_t)G.code_offset; k < 2 * ((size_t)G.code_offset + G.code_len); k++) printf(" %x", gs.code[k]);
    printf("\n");
  }
  return 0;
}
