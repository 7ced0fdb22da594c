// TEST HARNESS (not product code): emu_stark.cpp (csrc/stark.hpp) under ASan + UBSan as a stand-alone program, linked against
// nothing else, built and run on the CPU by hand like its siblings:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_stark tests/emu/sanitize_stark_main.cpp && /tmp/emu_sanitize_stark
// A Fibonacci AIR (8 rows, rate 2, q = 1, 2 challenges) and a Poseidon full-round AIR (4 rows, rate 3, q = 3, 13 registers): the
// witness check over heap blocks of exactly width * n words (satisfied, then one cell changed: the violation is named), the quotient
// of every coset point from an LDE block of exactly width * N words into a block of exactly challenges * 2^q n words - its
// interpolant must vanish above the degree bound, i.e. the division by Z_H was exact -, the verifier judging blocks of exactly the
// proof's word count (zeros, p - 1, 2^64 - 1, random words) to the end, and every refusal taken from a one-word block.
#include <vector>
#include "emu_stark.cpp"
#include "sanitize_common.hpp"

namespace gp = gate_program;

static void push(std::vector<uint32_t> &code, u32 op, u32 dst, u32 ka, u32 ia, u32 kb = gp::KIND_REG, u32 ib = 0) {
  gp::Insn in(0, 0);
  in.op = op; in.dst = dst; in.kind[0] = ka; in.kind[1] = kb; in.idx[0] = ia; in.idx[1] = ib;
  u32 w[2];
  in.encode(w);
  code.push_back(w[0]); code.push_back(w[1]);
}

struct Air {
  std::vector<uint32_t> code;
  std::vector<uint64_t> imm;
  lcp2_stark_desc d = {};
  void finish(u32 log_n, u32 width, u32 npi, u32 ch, u32 q, u32 rate_bits, u32 regs) {
    d.log_n = log_n; d.width = width; d.num_public_inputs = npi; d.num_challenges = ch; d.quotient_degree_bits = q;
    d.fri.rate_bits = rate_bits; d.fri.cap_height = 1; d.fri.proof_of_work_bits = 2; d.fri.num_query_rounds = 2;
    d.fri.num_fri_layers = 1; d.fri.fri_arity_bits[0] = 1;
    d.code = code.data(); d.code_words = code.size(); d.imm = imm.data(); d.num_imm = imm.size(); d.num_regs = regs;
  }
};

// values on H -> values on 7 H_N in leaf order, by definition (O(n N))
static std::vector<u64> lde_of(const std::vector<u64> &trace, u32 width, u32 log_n, u32 rate_bits) {
  const u64 n = 1ull << log_n, N = n << rate_bits;
  std::vector<u64> out(width * N);
  const u64 w = gl_root_of_unity(log_n), n_inv = gl_inv(n);
  for (u32 c = 0; c < width; c++) {
    std::vector<u64> coeff(n);
    for (u64 j = 0; j < n; j++) {
      u64 acc = 0;
      for (u64 i = 0; i < n; i++) acc = gl_add(acc, gl_mul(trace[c * n + i] % GL_P, gl_pow(gl_inv(w), i * j % n)));
      coeff[j] = gl_mul(acc, n_inv);
    }
    for (u64 i = 0; i < N; i++) {
      const u64 x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(log_n + rate_bits), bitrev32((u32)i, log_n + rate_bits)));
      u64 acc = 0;
      for (u64 j = n; j-- > 0;) acc = gl_add(gl_mul(acc, x), coeff[j]);
      out[c * N + i] = acc;
    }
  }
  return out;
}

static int run(Air &A, const std::vector<u64> &trace, const std::vector<u64> &pis, u32 degree_bound_chunks) {
  const lcp2_stark_desc &d = A.d;
  const u64 n = 1ull << d.log_n, M = n << d.quotient_degree_bits;
  const u64 words = emu_stark_words(&d);
  CHECK(words != 0);
  lcp2_stark_violation v = {};
  CHECK(emu_stark_check(&d, pis.data(), trace.data(), &v) == 0);
  {
    std::vector<u64> bad(trace);
    bad[(d.width - 1) * n + n / 2] ^= 1;
    CHECK(emu_stark_check(&d, pis.data(), bad.data(), &v) == 1 && v.kind == 1 && v.row == n / 2 - 1);
    bad = trace;
    bad[0] += GL_P * (bad[0] < ~0ull - GL_P ? 1 : 0);  // a non-canonical word is reduced
    CHECK(emu_stark_check(&d, pis.data(), bad.data(), &v) == 0);
  }
  const std::vector<u64> lde = lde_of(trace, d.width, d.log_n, d.fri.rate_bits);
  u64 alphas[ST_MAX_CH] = {rnd() % GL_P, rnd() % GL_P, rnd() % GL_P, rnd() % GL_P};
  std::vector<u64> quot(d.num_challenges * M);
  CHECK(emu_stark_quotient(&d, pis.data(), lde.data(), alphas, quot.data()) == 0);
  // the interpolant of the values on 7 H_M: coefficients from degree_bound_chunks * n on must vanish
  const u32 lgM = d.log_n + d.quotient_degree_bits;
  for (u32 c = 0; c < d.num_challenges; c++)
    for (u64 j = degree_bound_chunks * n; j < M; j++) {
      u64 acc = 0;
      for (u64 i = 0; i < M; i++) acc = gl_add(acc, gl_mul(quot[c * M + i], gl_pow(gl_inv(gl_root_of_unity(lgM)), (u64)bitrev32((u32)i, lgM) * j % M)));
      CHECK(acc == 0);
    }
  // the verifier on blocks of exactly the proof's size
  const u64 fills[3] = {0, GL_P - 1, ~0ull};
  for (int round = 0; round < 6; round++) {
    std::vector<u64> proof(words);
    for (u64 &w : proof) w = round < 3 ? fills[round] : rnd() % (round == 5 ? ~0ull : GL_P);
    lcp2_challenger ch = {};
    int failed = 0;
    CHECK(emu_stark_verify(&d, pis.data(), &ch, proof.data(), words, &failed) == LCP2_E_VERIFY && failed >= 1 && failed <= 9);
  }
  // refusals read nothing of the proof
  std::vector<u64> one(1);
  lcp2_challenger ch = {};
  int failed = 0;
  CHECK(emu_stark_verify(&d, pis.data(), &ch, one.data(), words - 1, &failed) == LCP2_E_INVALID);
  lcp2_stark_desc bad = d;
  bad.quotient_degree_bits = d.fri.rate_bits + 1;
  CHECK(emu_stark_words(&bad) == 0 && emu_stark_verify(&bad, pis.data(), &ch, one.data(), 1, &failed) == LCP2_E_INVALID);
  bad = d; bad.width = d.width - 1;  // the next-row operands now reach past 2 * width
  CHECK(emu_stark_words(&bad) == 0 && emu_stark_verify(&bad, pis.data(), &ch, one.data(), 1, &failed) == LCP2_E_INVALID);
  bad = d; bad.num_regs = 0;
  CHECK(emu_stark_words(&bad) == 0);
  return 0;
}

int main() {
  {  // Fibonacci: (a, b) -> (b, a + b)
    Air A;
    push(A.code, LCP2_OP_SUB, 0, gp::KIND_WIRE, 0, gp::KIND_PI, 0); push(A.code, LCP2_OP_EMIT, 0, gp::KIND_REG, 0);
    A.d.first_row = {0, 2, 1};
    push(A.code, LCP2_OP_SUB, 0, gp::KIND_WIRE, 2, gp::KIND_WIRE, 1); push(A.code, LCP2_OP_EMIT, 0, gp::KIND_REG, 0);
    push(A.code, LCP2_OP_ADD, 0, gp::KIND_WIRE, 0, gp::KIND_WIRE, 1); push(A.code, LCP2_OP_SUB, 0, gp::KIND_WIRE, 3, gp::KIND_REG, 0);
    push(A.code, LCP2_OP_EMIT, 0, gp::KIND_REG, 0);
    A.d.transition = {2, 5, 2};
    push(A.code, LCP2_OP_SUB, 0, gp::KIND_WIRE, 1, gp::KIND_PI, 1); push(A.code, LCP2_OP_EMIT, 0, gp::KIND_REG, 0);
    A.d.last_row = {7, 2, 1};
    A.finish(3, 2, 2, 2, 1, 2, 1);
    std::vector<u64> t(2 * 8);
    u64 a = 3, b = 5;
    for (u32 i = 0; i < 8; i++) { t[i] = a; t[8 + i] = b; const u64 s = gl_add(a, b); a = b; b = s; }
    if (run(A, t, {3, t[8 + 7]}, 1)) return 1;
  }
  {  // a Poseidon full round: next = MDS(sbox(local)) + constants
    Air A;
    for (u32 j = 0; j < 12; j++) A.imm.push_back(rnd() % GL_P);
    A.d.first_row = {0, 0, 0};
    for (u32 j = 0; j < 12; j++) push(A.code, LCP2_OP_SBOX, j, gp::KIND_WIRE, j);
    push(A.code, LCP2_OP_PMDS, 0, gp::KIND_REG, 0, gp::KIND_IMM, 0);
    for (u32 j = 0; j < 12; j++) { push(A.code, LCP2_OP_SUB, 12, gp::KIND_WIRE, 12 + j, gp::KIND_REG, j); push(A.code, LCP2_OP_EMIT, 0, gp::KIND_REG, 12); }
    A.d.transition = {0, 37, 12};
    A.d.last_row = {37, 0, 0};
    A.finish(2, 12, 0, 1, 3, 3, 13);
    std::vector<u64> t(12 * 4), s(12);
    for (u32 j = 0; j < 12; j++) s[j] = rnd() % GL_P;
    for (u32 i = 0; i < 4; i++) {
      for (u32 j = 0; j < 12; j++) t[j * 4 + i] = s[j];
      std::vector<u64> p(12), nx(12);
      for (u32 j = 0; j < 12; j++) p[j] = gl_pow(s[j], 7);
      for (u32 r = 0; r < 12; r++) {
        u64 acc = gl_add(A.imm[r], gl_mul(p[r], gp::MDS_DIAG[r]));
        for (u32 k = 0; k < 12; k++) acc = gl_add(acc, gl_mul(p[(k + r) % 12], gp::MDS_CIRC[k]));
        nx[r] = acc;
      }
      s = nx;
    }
    if (run(A, t, {}, 6)) return 1;
  }
  printf("sanitize_stark: ok\n");
  return 0;
}
