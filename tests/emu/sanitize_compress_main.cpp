// TEST HARNESS (not product code): emu_compress.cpp (csrc/proof_compress.hpp) under ASan + UBSan as a stand-alone program, linked
// against nothing else, built and run on the CPU like its siblings (tests/checks/emu_sanitize.sh):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_compress tests/emu/sanitize_compress_main.cpp && /tmp/emu_sanitize_compress
// A small layout (32 leaves, two FRI layers of arity 2, cap height 1) with real Merkle trees over random leaves.  For index sets of
// every class - the same index, level-0 siblings, merges at a middle and at the last level, no merge, 64 queries, and random sets -
// the proof is compressed into a heap block of exactly pc_compressed_words words and decompressed from it into a block of exactly
// proof_words words, so a read or write outside either is a heap overflow; the result must be the proof word for word.  Every other
// word count from 0 to proof_words + 2 is refused from a block of exactly that many words, and filled compressed proofs (p - 1,
// zeros, 2^64 - 1, random words) decode to the end inside their blocks whatever they hold.
#include <vector>
#include "emu_compress.cpp"
#include "sanitize_common.hpp"

static u64 rnd_gl() { return rnd() % GL_P; }

struct Tree {
  std::vector<std::vector<u64>> levels;
  void build(const std::vector<u64> &leaves, u32 nleaves, u32 leaf_len, u32 cap_height) {
    const u64 *rc = emu_round_constants();
    levels.assign(1, std::vector<u64>(4 * nleaves));
    for (u32 i = 0; i < nleaves; i++) vq_hash_or_noop(&leaves[(size_t)i * leaf_len], leaf_len, &levels[0][4 * i], rc);
    for (u32 n = nleaves; n > (1u << cap_height); n >>= 1) {
      std::vector<u64> up(4 * (n / 2));
      for (u32 i = 0; i < n / 2; i++) {
        u64 s[12] = {0};
        for (u32 k = 0; k < 8; k++) s[k] = levels.back()[8 * i + k];
        pos_permute(s, rc);
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

static int run_set(lcp2_params p, const std::vector<u32> &xs, const std::vector<u64> *leaves, const Tree *trees, u64 *saved, bool sweep) {
  p.num_query_rounds = (u32)xs.size();
  const ProofLayout L(p);
  const VqLayout V = vq_make_layout(L, p);
  u32 x[VQ_MAX_QUERIES] = {0};
  for (size_t q = 0; q < xs.size(); q++) x[q] = xs[q];
  std::vector<u64> proof(L.total);
  for (u64 &w : proof) w = rnd_gl();
  for (u32 t = 0; t < V.num_trees; t++)
    for (u32 q = 0; q < V.num_queries; q++) {
      u64 *leaf = &proof[pc_full_leaf(V, t, q)];
      const u32 index = x[q] >> V.tree[t].index_shift;
      for (u32 j = 0; j < V.tree[t].leaf_len; j++) leaf[j] = leaves[t][(size_t)index * V.tree[t].leaf_len + j];
      trees[t].siblings(index, leaf + V.tree[t].leaf_len);
    }
  const u64 words = emu_compressed_words(&p, x);
  CHECK(words <= emu_compressed_words_max(&p) && words >= pc_outside_words(V));
  std::vector<u64> comp(words);  // exactly
  CHECK(emu_compress(&p, x, (const unsigned long long *)proof.data(), (unsigned long long *)comp.data()) == words);
  std::vector<u64> back(L.total, 0x5555555555555555ull);
  CHECK(emu_decompress(&p, x, (const unsigned long long *)comp.data(), words, (unsigned long long *)back.data()) == LCP2_OK);
  CHECK(back == proof);
  *saved += L.total - words;
  // the predicates against their definition
  for (u32 t = 0; t < V.num_trees; t++)
    for (u32 q = 0; q < V.num_queries; q++) {
      const PcPlan plan = pc_plan(x, V.num_queries, q, V.tree[t].index_shift, V.tree[t].nsib);
      const u32 idx = x[q] >> V.tree[t].index_shift;
      bool leaf = true;
      for (u32 o = 0; o < q; o++) leaf = leaf && (x[o] >> V.tree[t].index_shift) != idx;
      CHECK(pc_leaf_stored(plan) == leaf);
      for (u32 l = 0; l < V.tree[t].nsib; l++) {
        bool stored = true;
        for (u32 o = 0; o < V.num_queries; o++) {
          const u32 y = (x[o] >> V.tree[t].index_shift) >> l;
          if ((o < q && y == idx >> l) || y == ((idx >> l) ^ 1)) stored = false;
        }
        CHECK(pc_sibling_stored(plan, l) == stored);
      }
    }
  if (!sweep) return 0;
  for (u64 n = 0; n <= L.total + 2; n++) {
    if (n == words) continue;
    std::vector<u64> block(n);  // exactly n words: nothing may be read past them
    for (u64 i = 0; i < n; i++) block[i] = i < words ? comp[i] : rnd_gl();
    std::vector<u64> out(L.total, 7);
    CHECK(emu_decompress(&p, x, (const unsigned long long *)block.data(), n, (unsigned long long *)out.data()) == LCP2_E_INVALID);
    for (u64 w : out) CHECK(w == 7);
  }
  for (int kind = 0; kind < 4; kind++) {
    std::vector<u64> f(words);
    for (u64 &w : f) w = kind == 0 ? GL_P - 1 : kind == 1 ? 0 : kind == 2 ? ~0ull : rnd();
    CHECK(emu_decompress(&p, x, (const unsigned long long *)f.data(), words, (unsigned long long *)back.data()) == LCP2_OK);
    for (u64 i = 0; i < V.queries; i++) CHECK(back[i] == f[i]);
  }
  return 0;
}

int main() {
  lcp2_params p = {};
  p.degree_bits = 3; p.rate_bits = 2; p.num_wires = 9; p.num_routed_wires = 4; p.num_constants = 1; p.cap_height = 1; p.num_challenges = 2;
  p.quotient_degree_factor = 2; p.num_query_rounds = 3; p.proof_of_work_bits = 1; p.num_fri_layers = 2; p.fri_arity_bits[0] = 1; p.fri_arity_bits[1] = 1;
  const u32 N = 32;
  const VqLayout V = vq_make_layout(ProofLayout(p), p);
  CHECK(V.num_trees == 6 && V.tree[0].nsib == 4 && V.tree[4].nsib == 3 && V.tree[5].nsib == 2 && V.tree[0].leaf_len == 5 && V.tree[4].leaf_len == 4);
  std::vector<u64> leaves[6];
  Tree trees[6];
  for (u32 t = 0; t < 6; t++) {
    const u32 n = N >> V.tree[t].index_shift;
    leaves[t].resize((size_t)n * V.tree[t].leaf_len);
    for (u64 &w : leaves[t]) w = rnd_gl();
    trees[t].build(leaves[t], n, V.tree[t].leaf_len, p.cap_height);
    CHECK(trees[t].levels.size() == V.tree[t].nsib + 1);
  }
  u64 saved = 0;
  const std::vector<std::vector<u32>> sets = {{5, 5, 20}, {9, 9, 9, 9}, {6, 7, 25}, {7, 25, 6}, {1, 2, 16}, {1, 6}, {0, 8}, {0, 16}, {3, 19}, {11}, {1, 0, 1, 14, 30, 31, 8}, {31, 0}};
  u32 runs = 0;
  for (const auto &s : sets) { if (run_set(p, s, leaves, trees, &saved, true)) return 1; runs++; }
  std::vector<u32> all(64);
  for (u32 i = 0; i < 64; i++) all[i] = (37 * i + 3) % N;
  if (run_set(p, all, leaves, trees, &saved, false)) return 1;
  runs++;
  for (int k = 0; k < 40; k++, runs++) {
    std::vector<u32> s(1 + rnd() % 64);
    for (u32 &v : s) v = (u32)(rnd() % N);
    if (run_set(p, s, leaves, trees, &saved, false)) return 1;
  }
  {  // no siblings at all: every tree no deeper than its cap
    lcp2_params e = p;
    e.degree_bits = 1; e.rate_bits = 1; e.cap_height = 2; e.num_fri_layers = 0;
    const VqLayout E = vq_make_layout(ProofLayout(e), e);
    CHECK(E.num_trees == 4 && E.tree[0].nsib == 0);
    std::vector<u64> el[4];
    Tree et[4];
    for (u32 t = 0; t < 4; t++) {
      el[t].resize((size_t)4 * E.tree[t].leaf_len);
      for (u64 &w : el[t]) w = rnd_gl();
      et[t].build(el[t], 4, E.tree[t].leaf_len, e.cap_height);
    }
    if (run_set(e, {0, 3, 3, 1, 2}, el, et, &saved, true)) return 1;
    runs++;
  }
  printf("sanitize_compress: %u index sets round-tripped through blocks of exactly their sizes (%llu words dropped in all), every other word count refused, filled proofs decoded: ok\n",
         runs, (unsigned long long)saved);
  return 0;
}
