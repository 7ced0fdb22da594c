// TEST HARNESS (not product code): emu_verify_head.cpp under ASan + UBSan as a stand-alone program, linked against nothing else
// (built like its siblings in tests/checks/emu_sanitize.sh: g++ -O1 -g -std=c++17 -fsanitize=address,undefined).
// A small layout (4 rows, 9 wires, 13 public inputs, two FRI layers) with a two-gate circuit whose programs use every opcode and
// operand kind, and proofs of random canonical words in heap blocks of exactly proof_words words, the public inputs in a block of
// exactly 13: the proof-of-work word is searched until the transcript passes, so that every slot of the identity and the finish
// run (to code 3: random openings satisfy nothing) without leaving the proof; the gate slots must add up to eval_gates_filtered.
#include <vector>
#include "emu_verify_head.cpp"
#include "sanitize_common.hpp"

static u64 rnd_gl() { return rnd() % GL_P; }

static void put(std::vector<uint32_t> &code, u32 op, u32 dst, u32 ka, u32 ia, u32 kb = 0, u32 ib = 0) {
  gate_program::Insn in(0, 0);
  in.op = op; in.dst = dst; in.kind[0] = ka; in.kind[1] = kb; in.idx[0] = ia; in.idx[1] = ib;
  uint32_t w[2];
  in.encode(w);
  code.push_back(w[0]); code.push_back(w[1]);
}

int main() {
  using namespace gate_program;
  lcp2_circuit_desc desc = {};
  lcp2_params &p = desc.params;
  p.degree_bits = 2; p.rate_bits = 2; p.num_wires = 9; p.num_routed_wires = 5; p.num_constants = 3; p.cap_height = 1; p.num_challenges = 2;
  p.quotient_degree_factor = 2; p.num_query_rounds = 3; p.proof_of_work_bits = 2; p.num_fri_layers = 2; p.fri_arity_bits[0] = 1; p.fri_arity_bits[1] = 1;
  std::vector<uint32_t> code;
  // gate 0, constraints listed last to first
  put(code, LCP2_OP_ADD, 0, KIND_WIRE, 0, KIND_CONST, 0);
  put(code, LCP2_OP_MUL, 1, KIND_REG, 0, KIND_IMM, 0);
  put(code, LCP2_OP_MULADD, 1, KIND_WIRE, 1, KIND_PI, 3);
  put(code, LCP2_OP_XOR, 2, KIND_REG, 0, KIND_REG, 1);
  put(code, LCP2_OP_DBLADD, 3, KIND_REG, 2, KIND_WIRE, 8);
  put(code, LCP2_OP_SUB, 4, KIND_REG, 3, KIND_IMM, 1);
  put(code, LCP2_OP_EMIT, 0, KIND_REG, 4);
  put(code, LCP2_OP_EMITBOOL, 0, KIND_WIRE, 3);
  const u32 len0 = (u32)code.size() / 2;
  // gate 1, first to last: an S-box, an MDS layer from registers 12..23 into 0..11 with immediates 2..13
  for (u32 i = 0; i < 12; i++) put(code, LCP2_OP_ADD, 12 + i, KIND_WIRE, i % 9, KIND_IMM, i % 2);
  put(code, LCP2_OP_SBOX, 12, KIND_REG, 12);
  put(code, LCP2_OP_PMDS, 0, KIND_REG, 12, KIND_IMM, 2);
  put(code, LCP2_OP_EMIT, 0, KIND_REG, 0);
  put(code, LCP2_OP_EMIT, 0, KIND_REG, 11);
  const u32 len1 = (u32)code.size() / 2 - len0;
  lcp2_gate gates[2] = {{0, 0, 0, 2, 0, len0, 2, 0}, {0, 1, 0, 2, len0, len1, 2, LCP2_GATE_EMIT_FORWARD}};
  std::vector<u64> imm(14), k_is(p.num_routed_wires), digest(4);
  for (u64 &w : imm) w = rnd_gl();
  for (u64 &w : k_is) w = rnd_gl();
  for (u64 &w : digest) w = rnd_gl();
  desc.k_is = (const uint64_t *)k_is.data(); desc.num_selectors = 1; desc.num_gates = 2; desc.gates = gates; desc.code = code.data(); desc.code_words = code.size();
  desc.imm = (const uint64_t *)imm.data(); desc.num_imm = imm.size(); desc.num_public_inputs = 13; desc.num_regs = 24;
  const ProofLayout L(p);
  CHECK(emu_head_block_bytes() == sizeof(VqChallenge));

  u32 reached = 0;
  for (int kind = 0; kind < 4; kind++) {
    std::vector<u64> proof(L.total), pis(13);
    for (u64 &w : proof) w = kind == 1 ? GL_P - 1 : kind == 2 ? 0 : rnd_gl();
    for (u64 &w : pis) w = kind == 3 ? ~0ull : rnd_gl();  // public inputs are canonicalised by the head, not by the caller
    int dev = -9, host = -9;
    VqChallenge a, b;
    for (u64 witness = 0; witness < 64; witness++) {  // 2 bits of work: a few tries
      proof[L.pow_witness] = witness;
      CHECK(emu_head_batch(&desc, (const unsigned long long *)digest.data(), (const unsigned long long *)proof.data(), L.total, 1,
                           (const unsigned long long *)pis.data(), 13, &dev, &host, &a, &b) == 0);
      CHECK(dev == host && (dev == 2 || dev == 3 || dev == 0));
      if (dev != 2) break;
    }
    CHECK(dev != 2);
    CHECK(memcmp(&a, &b, sizeof a) == 0);
    u64 got[4], ref[4];
    CHECK(emu_head_gate_sums(&desc, (const unsigned long long *)digest.data(), (const unsigned long long *)proof.data(), (const unsigned long long *)pis.data(),
                             (unsigned long long *)got, (unsigned long long *)ref) == 0);
    CHECK(memcmp(got, ref, sizeof got) == 0);
    reached++;
  }
  // a word >= p stops at check 1 in both forms; wrong lengths read nothing
  {
    std::vector<u64> proof(L.total, 1), pis(13, 1);
    proof[L.total - 1] = GL_P;
    int dev = -9, host = -9;
    VqChallenge a, b;
    CHECK(emu_head_batch(&desc, (const unsigned long long *)digest.data(), (const unsigned long long *)proof.data(), L.total, 1,
                         (const unsigned long long *)pis.data(), 13, &dev, &host, &a, &b) == 0 && dev == 1 && host == 1);
    CHECK(emu_head_batch(&desc, nullptr, nullptr, L.total + 1, 1, nullptr, 13, nullptr, nullptr, nullptr, nullptr) == -1);
  }
  printf("sanitize_verify_head: proofs of %zu words, 13 public inputs, %u fills through transcript, %u slots and finish in both forms: ok\n", (size_t)L.total,
         reached, desc.num_gates + 1);
  return 0;
}
