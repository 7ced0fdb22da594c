// TEST HARNESS (not product code): emu_openings.cpp (csrc/fri_openings.hpp) under ASan + UBSan as a stand-alone program, linked
// against nothing else, built and run on the CPU like its siblings:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_openings tests/emu/sanitize_openings_main.cpp && /tmp/emu_sanitize_openings
// Two oracles of 3 and 2 columns, 8 coefficients, rate 1, cap height 1, two points (the second over one column that the first lists
// too), two layers of arity 2: the proof is assembled here - openings by Horner, the committed polynomial by the portable
// composition and division, LDEs by evaluation, Merkle trees, folds, the smallest proof-of-work witness - into a heap block of
// exactly the layout's word count, and must be accepted.  Then every one-word change (+1 mod p, and +p where it fits) must be
// rejected from a block of exactly that size, the +p ones as check 1; proofs of p - 1, zeros, 2^64 - 1 and random words are judged to
// the end inside their blocks; and every refusal is taken before a word of the proof is read (a one-word block is handed over).
#include <vector>
#include "emu_openings.cpp"
#include "sanitize_common.hpp"

static u64 rnd_gl() { return rnd() % GL_P; }
static const u64 *RC() { return HostPoseidon::get().round_constants(); }

struct Tree {
  std::vector<std::vector<u64>> levels;
  void build(const std::vector<u64> &leaves, u32 nleaves, u32 leaf_len, u32 cap_height) {
    levels.assign(1, std::vector<u64>(4 * nleaves));
    for (u32 i = 0; i < nleaves; i++) vq_hash_or_noop(&leaves[(size_t)i * leaf_len], leaf_len, &levels[0][4 * i], RC());
    for (u32 n = nleaves; n > (1u << cap_height); n >>= 1) {
      std::vector<u64> up(4 * (n / 2));
      for (u32 i = 0; i < n / 2; i++) {
        u64 s[12] = {0};
        for (u32 k = 0; k < 8; k++) s[k] = levels.back()[8 * i + k];
        pos_permute(s, RC());
        for (u32 k = 0; k < 4; k++) up[4 * i + k] = s[k];
      }
      levels.push_back(up);
    }
  }
  void siblings(u32 index, u64 *out) const {
    for (size_t l = 0; l + 1 < levels.size(); l++, index >>= 1)
      for (u32 k = 0; k < 4; k++) out[4 * l + k] = levels[l][4 * (index ^ 1) + k];
  }
};

static gl2 horner(const std::vector<gl2> &c, gl2 x) {
  gl2 r = gl2_make(0, 0);
  for (size_t i = c.size(); i-- > 0;) r = gl2_add(gl2_mul(r, x), c[i]);
  return r;
}
// values in leaf order on the coset shift * <w_{2^lg}>
static std::vector<gl2> lde(const std::vector<gl2> &c, u32 lg, u64 shift) {
  std::vector<gl2> v(1u << lg);
  for (u32 i = 0; i < (1u << lg); i++) v[i] = horner(c, gl2_make(gl_mul(shift, gl_pow(gl_root_of_unity(lg), bitrev32(i, lg))), 0));
  return v;
}

int main() {
  const u32 log_n = 3, n = 8, lgN = 4, N = 16, cols[2] = {3, 2};
  lcp2_fri_config cfg = {};
  cfg.rate_bits = 1; cfg.cap_height = 1; cfg.proof_of_work_bits = 3; cfg.num_query_rounds = 4; cfg.num_fri_layers = 2;
  cfg.fri_arity_bits[0] = 1; cfg.fri_arity_bits[1] = 1;
  const lcp2_fri_range r0[2] = {{0, 0, 3}, {1, 0, 2}}, r1[1] = {{1, 1, 1}};
  lcp2_fri_instance inst = {};
  inst.num_oracles = 2; inst.num_points = 2; inst.num_ranges[0] = 2; inst.num_ranges[1] = 1; inst.ranges[0] = r0; inst.ranges[1] = r1;
  const u64 points[4] = {rnd_gl(), rnd_gl(), gl_root_of_unity(log_n), 0};  // the second point lies in H
  const u64 total = emu_open_words(&cfg, log_n, cols, &inst);
  CHECK(total != 0);
  u32 pp[FO_MAX_POINTS] = {5, 1, 0, 0};
  const FoLayout L = fo_make_layout(cfg, log_n, cols, 2, pp, 2);
  CHECK(L.total == total && L.final_len == 2 && L.init_sib == 3 && L.step_sib[0] == 2 && L.step_sib[1] == 1);

  // the oracles
  std::vector<u64> coeffs[2], leaves[2];
  Tree trees[2];
  for (u32 o = 0; o < 2; o++) {
    coeffs[o].resize((size_t)cols[o] * n);
    for (u64 &w : coeffs[o]) w = rnd_gl();
    leaves[o].resize((size_t)N * cols[o]);
    for (u32 c = 0; c < cols[o]; c++) {
      std::vector<gl2> p(n);
      for (u32 i = 0; i < n; i++) p[i] = gl2_make(coeffs[o][(size_t)c * n + i], 0);
      const std::vector<gl2> v = lde(p, lgN, GL_GENERATOR);
      for (u32 i = 0; i < N; i++) leaves[o][(size_t)i * cols[o] + c] = v[i].c0;
    }
    trees[o].build(leaves[o], N, cols[o], cfg.cap_height);
  }
  const unsigned long long *caps[2] = {trees[0].levels.back().data(), trees[1].levels.back().data()};

  std::vector<u64> proof(total, 0);  // exactly
  HostChallenger ch;
  ch.observe(42);
  {  // openings
    u32 at = 0;
    for (u32 b = 0; b < 2; b++)
      for (u32 r = 0; r < inst.num_ranges[b]; r++)
        for (u32 j = 0; j < inst.ranges[b][r].num_polys; j++, at++) {
          const lcp2_fri_range &g = inst.ranges[b][r];
          std::vector<gl2> p(n);
          for (u32 i = 0; i < n; i++) p[i] = gl2_make(coeffs[g.oracle][(size_t)(g.first_poly + j) * n + i], 0);
          const gl2 v = horner(p, gl2_make(points[2 * b], points[2 * b + 1]));
          proof[2 * at] = v.c0; proof[2 * at + 1] = v.c1;
        }
  }
  ch.observe_n(proof.data(), 2 * L.total_polys);
  const gl2 alpha = ch.get_ext();
  std::vector<u64> f0(n), f1(n);
  {
    const unsigned long long *cp[2] = {coeffs[0].data(), coeffs[1].data()};
    const u64 a[2] = {alpha.c0, alpha.c1};
    CHECK(emu_open_compose(&inst, cols, cp, log_n, (const unsigned long long *)a, (const unsigned long long *)points, (unsigned long long *)f0.data(),
                           (unsigned long long *)f1.data()) == 0);
  }
  std::vector<gl2> f(n);
  for (u32 i = 0; i < n; i++) f[i] = gl2_make(f0[i], f1[i]);
  std::vector<u64> layer_leaves[2];
  Tree layer_trees[2];
  u32 lg = lgN;
  u64 shift = GL_GENERATOR;
  for (u32 l = 0; l < 2; l++) {
    const std::vector<gl2> v = lde(f, lg, shift);
    layer_leaves[l].resize(2 * v.size());
    for (size_t i = 0; i < v.size(); i++) { layer_leaves[l][2 * i] = v[i].c0; layer_leaves[l][2 * i + 1] = v[i].c1; }
    layer_trees[l].build(layer_leaves[l], (u32)v.size() / 2, 4, cfg.cap_height);
    CHECK(layer_trees[l].levels.back().size() == L.capw);
    for (u32 i = 0; i < L.capw; i++) proof[L.fri_caps + l * L.capw + i] = layer_trees[l].levels.back()[i];
    ch.observe_n(&proof[L.fri_caps + l * L.capw], L.capw);
    const gl2 beta = ch.get_ext();
    std::vector<gl2> g(f.size() / 2);
    for (size_t k = 0; k < g.size(); k++) g[k] = gl2_add(f[2 * k], gl2_mul(beta, f[2 * k + 1]));
    f = g; lg -= 1; shift = gl_sqr(shift);
  }
  CHECK(f.size() == L.final_len);
  for (u32 i = 0; i < L.final_len; i++) { proof[L.final_poly + 2 * i] = f[i].c0; proof[L.final_poly + 2 * i + 1] = f[i].c1; }
  ch.observe_n(&proof[L.final_poly], 2 * L.final_len);
  u64 witness = 0;
  for (;; witness++) { HostChallenger t = ch; t.observe(witness); if ((t.get() >> (64 - cfg.proof_of_work_bits)) == 0) break; }
  proof[L.pow_witness] = witness;
  ch.observe(witness);
  (void)ch.get();
  for (u32 q = 0; q < cfg.num_query_rounds; q++) {
    u32 idx = (u32)(ch.get() % N);
    u64 *R = &proof[L.queries + (u64)q * L.query_words];
    for (u32 o = 0; o < 2; o++) {
      for (u32 c = 0; c < cols[o]; c++) R[L.init_off[o] + c] = leaves[o][(size_t)idx * cols[o] + c];
      trees[o].siblings(idx, R + L.init_off[o] + cols[o]);
    }
    for (u32 l = 0; l < 2; l++) {
      idx >>= 1;
      for (u32 k = 0; k < 4; k++) R[L.step_off[l] + k] = layer_leaves[l][(size_t)4 * idx + k];
      layer_trees[l].siblings(idx, R + L.step_off[l] + 4);
    }
  }

  auto judge = [&](const std::vector<u64> &pr, const unsigned long long *pts, int *failed, lcp2_challenger *out) {
    lcp2_challenger c = {};
    HostChallenger h;
    h.observe(42);
    h.save((u64 *)c.sponge, (u64 *)c.input, c.input_len, (u64 *)c.output, c.output_len);
    const int rc = emu_open_verify(caps, cols, log_n, &inst, pts, &cfg, &c, (const unsigned long long *)pr.data(), pr.size(), failed);
    if (out) *out = c;
    return rc;
  };
  int failed = -1;
  lcp2_challenger after = {}, mine = {};
  CHECK(judge(proof, (const unsigned long long *)points, &failed, &after) == LCP2_OK && failed == 0);
  ch.save((u64 *)mine.sponge, (u64 *)mine.input, mine.input_len, (u64 *)mine.output, mine.output_len);
  CHECK(memcmp(after.sponge, mine.sponge, sizeof mine.sponge) == 0 && after.output_len == mine.output_len && after.input_len == mine.input_len);
  u32 seen[8] = {0};
  for (u64 w = 0; w < total; w++) {
    std::vector<u64> bad(proof);  // exactly
    bad[w] = (proof[w] + 1) % GL_P;
    CHECK(judge(bad, (const unsigned long long *)points, &failed, nullptr) == LCP2_E_VERIFY && failed >= 2 && failed <= 6);
    seen[failed]++;
    if (proof[w] < (u64)0 - GL_P) {
      bad[w] = proof[w] + GL_P;
      CHECK(judge(bad, (const unsigned long long *)points, &failed, nullptr) == LCP2_E_VERIFY && failed == 1);
    }
  }
  CHECK(seen[3] && seen[5]);
  for (int kind = 0; kind < 4; kind++) {
    std::vector<u64> fill(total);
    for (u64 &w : fill) w = kind == 0 ? GL_P - 1 : kind == 1 ? 0 : kind == 2 ? ~0ull : rnd_gl();
    CHECK(judge(fill, (const unsigned long long *)points, &failed, nullptr) == LCP2_E_VERIFY && failed >= 1 && failed <= 7);
  }
  // refusals read nothing of the proof: a one-word block
  const std::vector<u64> one(1, 0);
  CHECK(judge(one, (const unsigned long long *)points, &failed, nullptr) == LCP2_E_INVALID);
  const u64 zero_point[4] = {0, 0, 5, 6};
  std::vector<u64> same(total, 1);
  CHECK(judge(same, (const unsigned long long *)zero_point, &failed, nullptr) == LCP2_E_INVALID);
  printf("sanitize_openings: a proof of %llu words assembled and accepted, %llu one-word changes rejected (checks 2..6: %u %u %u %u %u), filled proofs judged, refusals taken: ok\n",
         (unsigned long long)total, (unsigned long long)total, seen[2], seen[3], seen[4], seen[5], seen[6]);
  return 0;
}
