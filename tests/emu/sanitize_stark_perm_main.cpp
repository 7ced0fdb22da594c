// TEST HARNESS (not product code): emu_stark_perm.cpp (the permutation-argument text of csrc/stark.hpp) under ASan + UBSan as a
// stand-alone program, linked against nothing else, built and run on the CPU by hand like its siblings:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_stark_perm tests/emu/sanitize_stark_perm_main.cpp && /tmp/emu_sanitize_stark_perm
// An AIR without constraints of its own, width 5, 8 and 32 rows, rate 2, q = 1, 2 challenges: three pairs of 1, 1 and 2 columns in
// batches of 2 (6 instances, 3 Z columns) and of 1 (6 Z columns), all tables heap blocks of exactly their size.  The ratios and Z
// columns from a trace block of exactly width * n words with lanes 128, 2 and 1 rows apart (the products close, the ratios are
// those of one inversion per row; one changed cell: the right Z stays open), the quotient of every coset point from LDE blocks of
// exactly width * N and numZ * N words - its interpolant must vanish above the degree bound, i.e. the all-rows constraint holds on
// the wrap-around too -, the verifier judging blocks of exactly the proof's word count to the end, and every refusal taken from
// tables of exactly the size the description states.
#include <vector>
#include "emu_stark_perm.cpp"
#include "sanitize_common.hpp"

// values on H -> values on 7 H_N in leaf order, by definition (O(n N))
static std::vector<u64> lde_of(const std::vector<u64> &vals, u32 cols, u32 log_n, u32 rate_bits) {
  const u64 n = 1ull << log_n, N = n << rate_bits;
  std::vector<u64> out(cols * N);
  const u64 w = gl_root_of_unity(log_n), n_inv = gl_inv(n);
  for (u32 c = 0; c < cols; c++) {
    std::vector<u64> coeff(n);
    for (u64 j = 0; j < n; j++) {
      u64 acc = 0;
      for (u64 i = 0; i < n; i++) acc = gl_add(acc, gl_mul(vals[c * n + i] % GL_P, gl_pow(gl_inv(w), i * j % n)));
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

static int run(u32 log_n, u32 batch) {
  const u32 width = 5, CH = 2, q = 1, rate_bits = 2;
  const u64 n = 1ull << log_n, N = n << rate_bits, M = n << q;
  lcp2_stark_desc d = {};
  d.log_n = log_n; d.width = width; d.num_challenges = CH; d.quotient_degree_bits = q;
  d.fri.rate_bits = rate_bits; d.fri.cap_height = 1; d.fri.proof_of_work_bits = 2; d.fri.num_query_rounds = 2;
  d.fri.num_fri_layers = 1; d.fri.fri_arity_bits[0] = 1;
  // columns 0, 1 are permutations of column 4 and of each other's source; (2, 3) as tuples of (1, 0) under a third permutation
  std::vector<lcp2_stark_perm_pair> pairs = {{0, 1}, {1, 1}, {2, 2}};
  std::vector<uint32_t> columns = {0, 4, 1, 0, 2, 1, 3, 0};   // [4][2]
  lcp2_stark_perm perm = {3, pairs.data(), columns.data(), 4, batch};
  std::vector<u64> t(width * n);
  for (u64 i = 0; i < n; i++) {
    t[4 * n + i] = rnd();                                    // any u64: reduced where it is read
    t[0 * n + (5 * i + 3) % n] = t[4 * n + i] % GL_P;        // column 0 = column 4 permuted
    t[1 * n + (3 * i + 1) % n] = t[0 * n + (5 * i + 3) % n] + ((t[4 * n + i] % GL_P) < ~0ull - GL_P && (i & 1) ? GL_P : 0);  // column 1 = column 0 permuted
  }
  for (u64 i = 0; i < n; i++) { t[2 * n + (7 * i + 2) % n] = t[1 * n + i]; t[3 * n + (7 * i + 2) % n] = t[0 * n + i]; }
  const u32 numZ = (3 * CH + batch - 1) / batch;
  const u64 words = emu_stark_perm_words(&d, &perm);
  CHECK(words != 0 && words > emu_stark_perm_words(&d, nullptr));
  std::vector<u64> draws(2 * batch * CH);
  for (u64 &v : draws) v = rnd() % GL_P;
  std::vector<u64> ratio(numZ * n), zs(numZ * n), ratio1(numZ * n), zs1(numZ * n);
  CHECK(emu_stark_perm_columns(&d, &perm, draws.data(), t.data(), 128, ratio.data(), zs.data()) == -1);
  for (u32 threads : {2u, 1u}) {
    CHECK(emu_stark_perm_columns(&d, &perm, draws.data(), t.data(), threads, ratio1.data(), zs1.data()) == -1);
    CHECK(ratio1 == ratio && zs1 == zs);
  }
  for (u32 z = 0; z < numZ; z++) CHECK(zs[z * n] == 1);
  {
    std::vector<u64> bad(t);
    bad[3 * n + n / 2] ^= 1;  // the last pair: the Z column of its first instance, 2 CH, is the smallest that stays open
    CHECK(emu_stark_perm_columns(&d, &perm, draws.data(), bad.data(), 128, ratio1.data(), zs1.data()) == (int)(2 * CH / batch));
    bad[0 * n + 1] ^= 1;      // the lhs of the first pair: Z 0
    CHECK(emu_stark_perm_columns(&d, &perm, draws.data(), bad.data(), 128, ratio1.data(), zs1.data()) == 0);
  }
  const std::vector<u64> lde = lde_of(t, width, log_n, rate_bits), z_lde = lde_of(zs, numZ, log_n, rate_bits);
  u64 alphas[ST_MAX_CH] = {rnd() % GL_P, rnd() % GL_P, rnd() % GL_P, rnd() % GL_P};
  std::vector<u64> quot(CH * M);
  CHECK(emu_stark_perm_quotient(&d, &perm, draws.data(), nullptr, lde.data(), z_lde.data(), alphas, quot.data()) == 0);
  // the all-rows constraint of batch B has degree B + 1: the quotient's degree is at most (B + 1)(n - 1) - n
  const u32 lgM = log_n + q;
  for (u32 c = 0; c < CH; c++)
    for (u64 j = (batch + 1) * (n - 1) - n + 1; j < M; j++) {
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
    CHECK(emu_stark_perm_verify(&d, &perm, nullptr, &ch, proof.data(), words, &failed) == LCP2_E_VERIFY && failed >= 1 && failed <= 9);
  }
  // refusals read nothing of the proof and nothing past the tables
  std::vector<u64> one(1);
  lcp2_challenger ch = {};
  int failed = 0;
  char why[128];
  CHECK(emu_stark_perm_verify(&d, &perm, nullptr, &ch, one.data(), words - 1, &failed) == LCP2_E_INVALID);
  lcp2_stark_perm bad = perm;
  bad.batch_size = 3;
  CHECK(emu_stark_perm_problem(&d, &bad, why, sizeof why) == 1 && emu_stark_perm_words(&d, &bad) == 0);
  bad = perm; bad.num_column_pairs = 3;   // the last pair's run now ends outside
  CHECK(emu_stark_perm_problem(&d, &bad, why, sizeof why) == 1 && emu_stark_perm_verify(&d, &bad, nullptr, &ch, one.data(), 1, &failed) == LCP2_E_INVALID);
  std::vector<uint32_t> wide(columns);
  wide[7] = width;
  bad = perm; bad.columns = wide.data();
  CHECK(emu_stark_perm_problem(&d, &bad, why, sizeof why) == 1);
  std::vector<lcp2_stark_perm_pair> empty_pair = {{0, 1}, {1, 0}, {2, 2}};
  bad = perm; bad.pairs = empty_pair.data();
  CHECK(emu_stark_perm_problem(&d, &bad, why, sizeof why) == 1);
  bad = perm; bad.num_pairs = 65;  // refused before pairs[3] would be read
  CHECK(emu_stark_perm_problem(&d, &bad, why, sizeof why) == 1);
  bad = perm; bad.num_pairs = 0;   // no permutation: the plain call, tables unread
  bad.pairs = nullptr; bad.columns = nullptr;
  CHECK(emu_stark_perm_problem(&d, &bad, why, sizeof why) == 0 && emu_stark_perm_words(&d, &bad) == emu_stark_perm_words(&d, nullptr));
  return 0;
}

int main() {
  if (run(3, 2) || run(3, 1) || run(5, 2)) return 1;
  printf("sanitize_stark_perm: ok\n");
  return 0;
}
