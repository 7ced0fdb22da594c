// TEST HARNESS (not product code): emu_verify.cpp under ASan + UBSan as a stand-alone program, linked against nothing else
// (tests/checks/emu_sanitize.sh).
// A small layout (16 leaves, two FRI layers of arity 2, cap height 1, three queries) and every job of the two query kernels over:
// a GENERATED proof - real Merkle trees over random leaves, the fold chain of query 0 made consistent down to the final polynomial -
// whose paths must all hold and whose query 0 must pass; then proofs filled with p - 1, with zeros and with random words, whose jobs
// must run to a verdict without leaving the proof.  Every proof lives in a heap block of exactly proof_words words, so a read past it
// is a heap overflow.
#include <vector>
#include "emu_verify.cpp"
#include "sanitize_common.hpp"

static u64 rnd_gl() { return rnd() % GL_P; }  // a canonical field element

// a Merkle tree over nleaves leaves of leaf_len words: level 0 = leaf digests ... the cap level
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

int main() {
  lcp2_params p = {};
  p.degree_bits = 2; p.rate_bits = 2; p.num_wires = 9; p.num_routed_wires = 4; p.num_constants = 1; p.cap_height = 1; p.num_challenges = 2;
  p.quotient_degree_factor = 2; p.num_query_rounds = 3; p.proof_of_work_bits = 1; p.num_fri_layers = 2; p.fri_arity_bits[0] = 1; p.fri_arity_bits[1] = 1;
  const ProofLayout L(p);
  const VqLayout V = vq_make_layout(L, p);
  const u32 N = 16, Q = p.num_query_rounds;
  CHECK(V.num_trees == 6 && V.final_len == 1 && V.tree[0].leaf_len == 5 && V.tree[1].leaf_len == 9 && V.tree[2].leaf_len == 4 && V.tree[4].leaf_len == 4);
  std::vector<u64> cs_cap(L.capw);
  VqChallenge c;
  memset(&c, 0, sizeof c);
  c.zeta = gl2_make(rnd_gl(), rnd_gl()); c.g_zeta = gl2_scale(c.zeta, gl_root_of_unity(p.degree_bits)); c.fri_alpha = gl2_make(rnd_gl(), rnd_gl());
  c.alpha_ch = gl2_pow(c.fri_alpha, p.num_challenges); c.red0 = gl2_make(rnd_gl(), rnd_gl()); c.red1 = gl2_make(rnd_gl(), rnd_gl());
  c.fri_betas[0] = gl2_make(rnd_gl(), rnd_gl()); c.fri_betas[1] = gl2_make(rnd_gl(), rnd_gl());
  c.x_index[0] = 3; c.x_index[1] = 12; c.x_index[2] = 9;  // distinct cosets in both layers
  c.live = 1;

  // ---- the generated proof
  std::vector<u64> proof(L.total);
  for (u64 &w : proof) w = rnd_gl();
  std::vector<u64> leaves[6];
  for (u32 t = 0; t < 4; t++) { leaves[t].resize((size_t)N * V.tree[t].leaf_len); for (u64 &w : leaves[t]) w = rnd_gl(); }
  for (u32 l = 0; l < 2; l++) { leaves[4 + l].resize((size_t)(N >> V.tree[4 + l].index_shift) * 4); for (u64 &w : leaves[4 + l]) w = rnd_gl(); }
  {  // query 0's fold chain: each layer's leaf holds the value carried so far at `within`, the final polynomial the last one
    u64 *R = &proof[L.queries];
    for (u32 t = 0; t < 4; t++) for (u32 j = 0; j < V.tree[t].leaf_len; j++) R[V.tree[t].leaf_off + j] = leaves[t][(size_t)c.x_index[0] * V.tree[t].leaf_len + j];
    u64 xi = c.x_index[0], x = vq_subgroup_x(V, c.x_index[0]);
    gl2 eval = vq_combine_initial(V, c, R, x);
    for (u32 l = 0; l < 2; l++) {
      const u32 within = (u32)xi & 1, coset = (u32)(xi >> 1);
      leaves[4 + l][4 * coset + 2 * within] = eval.c0;
      leaves[4 + l][4 * coset + 2 * within + 1] = eval.c1;
      for (u32 j = 0; j < 4; j++) R[V.tree[4 + l].leaf_off + j] = leaves[4 + l][4 * coset + j];
      CHECK(vq_fold_layer(V, c, R, l, xi, x, eval));
    }
    proof[L.final_poly] = eval.c0; proof[L.final_poly + 1] = eval.c1;
  }
  for (u32 t = 0; t < 6; t++) {
    Tree tree;
    const u32 nleaves = N >> V.tree[t].index_shift;
    tree.build(leaves[t], nleaves, V.tree[t].leaf_len, p.cap_height);
    CHECK(tree.levels.size() == V.tree[t].nsib + 1 && tree.levels.back().size() == L.capw);
    u64 *cap = t == 0 ? cs_cap.data() : &proof[V.tree[t].cap_off];
    for (size_t k = 0; k < L.capw; k++) cap[k] = tree.levels.back()[k];
    for (u32 q = 0; q < Q; q++) {
      u64 *leaf = &proof[L.queries + (size_t)q * L.query_words + V.tree[t].leaf_off];
      const u32 index = c.x_index[q] >> V.tree[t].index_shift;
      for (u32 j = 0; j < V.tree[t].leaf_len; j++) leaf[j] = leaves[t][(size_t)index * V.tree[t].leaf_len + j];
      tree.siblings(index, leaf + V.tree[t].leaf_len);
    }
  }
  u32 status[3];
  u32 paths = 0;
  for (u32 t = 0; t < V.num_trees; t++)
    for (u32 q = 0; q < Q; q++, paths++) CHECK(vq_path_job(V, c, proof.data(), cs_cap.data(), q, t, emu_round_constants()) == VQ_STATUS_NONE);
  emu_query_jobs(V, c, proof.data(), cs_cap.data(), status);
  CHECK(status[0] == VQ_STATUS_NONE);  // query 0 is consistent down to the final polynomial
  CHECK(status[1] == vq_status(vq_ord_consistency(0), VQ_CHECK_CONSISTENCY) && status[2] == status[1] && vq_reduce_statuses(status, Q) == 5);
  {  // one word of each kind, then the first failure in the host's order
    std::vector<u64> bad = proof;
    bad[L.final_poly] = gl_add(bad[L.final_poly], 1);
    emu_query_jobs(V, c, bad.data(), cs_cap.data(), status);
    CHECK(status[0] == vq_status(vq_ord_final(2), VQ_CHECK_FINAL_POLY));
    bad[L.queries + V.tree[5].leaf_off + V.tree[5].leaf_len] ^= 1;  // a sibling of layer 1
    emu_query_jobs(V, c, bad.data(), cs_cap.data(), status);
    CHECK(status[0] == vq_status(vq_ord_layer_path(1), VQ_CHECK_LAYER_PATH));
    bad[L.queries + V.tree[3].leaf_off] ^= 1;  // a leaf word of the quotient oracle: the path fails, and the fold chain's start moves
    emu_query_jobs(V, c, bad.data(), cs_cap.data(), status);
    CHECK(status[0] == vq_status(vq_ord_initial(3), VQ_CHECK_INITIAL_PATH));
    VqChallenge dead = c;
    dead.live = 0;
    emu_query_jobs(V, dead, bad.data(), cs_cap.data(), status);
    CHECK(status[0] == VQ_STATUS_NONE && status[1] == VQ_STATUS_NONE && status[2] == VQ_STATUS_NONE);
  }
  // ---- filled proofs: every job runs to a verdict inside the proof's own words, whatever they hold
  u32 fills = 0;
  for (int kind = 0; kind < 5; kind++, fills++) {
    std::vector<u64> f(L.total);
    for (u64 &w : f) w = kind == 0 ? GL_P - 1 : kind == 1 ? 0 : rnd_gl();
    VqChallenge cc = c;
    if (kind == 1) { memset(&cc, 0, sizeof cc); cc.live = 1; }                                         // zero challenges: inverses of zero
    if (kind >= 2) for (u32 q = 0; q < Q; q++) cc.x_index[q] = (u32)(rnd_gl() % N);
    if (kind == 4) for (u32 q = 0; q < Q; q++) cc.x_index[q] = N - 1;                                  // the last leaf, the last cap entry
    std::vector<u64> cap(L.capw, kind == 0 ? GL_P - 1 : 0);
    emu_query_jobs(V, cc, f.data(), cap.data(), status);
    for (u32 q = 0; q < Q; q++) CHECK(status[q] == vq_status(vq_ord_initial(0), VQ_CHECK_INITIAL_PATH));  // tree 0 fails first everywhere
    for (u32 q = 0; q < Q; q++) { const u32 s = vq_fri_query(V, cc, f.data(), f.data() + V.final_poly, q); CHECK(s == VQ_STATUS_NONE || (s & 0xFF) == 5 || (s & 0xFF) == 7); }
  }
  printf("sanitize_verify: generated proof of %zu words (%u paths hold, query 0 folds to its final polynomial), 4 tamper verdicts, %u filled proofs x %u jobs: ok\n",
         (size_t)L.total, paths, fills, Q * (V.num_trees + 1));
  return 0;
}
