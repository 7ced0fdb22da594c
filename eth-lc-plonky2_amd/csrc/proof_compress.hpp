// Compressed proofs - pruned Merkle multiproofs - as portable text, the way verify_query.hpp holds the query phase: what
// lcp2_proof_compress / lcp2_proof_decompress run on the host (proof_compress.hip), what k_decompress_paths is held to on the device,
// and what tests/emu/emu_compress.cpp runs on the CPU.  The layout is plonky2-shaped (proof.compress()) but PARITY UNPINNED: the
// reference holds no compressed proof.  Unlike plonky2 the evaluation at the queried position of every FRI step is kept.
//
// The format.  Trees are numbered as in VqLayout (t < 4: initial oracle t, 4 + l: FRI layer l); the leaf index of query q in tree t
// is  x_q >> tree[t].index_shift,  x_q the query index the transcript gives.  A compressed proof is
//   1. the words [0, queries) of the full proof,
//   2. its words [final_poly, total) (final polynomial, proof-of-work witness),
//   3. for t = 0, 1, ... and inside a tree for q = 0 .. R - 1:
//        the leaf of (t, q)                       iff no q' < q has the same leaf index, then
//        for level l = 0 .. nsib - 1, y = idx >> l,
//        the sibling digest of (t, q, l)          iff no q' < q has idx' >> l == y  and  no q' at all has idx' >> l == y ^ 1.
// There are no length fields: the word count is a function of the parameters and the indices (pc_compressed_words).
//
// Both predicates come from one pass over the indices of a tree (pc_plan): with b = bit length of idx_q ^ idx_q', the paths of q and
// q' share their node from level b on (b = 0: the same leaf), and q' passes through the sibling of q's node at level b - 1 only.
#pragma once
#include "verify_query.hpp"

namespace lcp2 {

constexpr u32 PC_NEVER = 33;           // pc_plan: no earlier query ever shares a node of this path below the cap
constexpr u32 PC_NONE = 0xFFFFFFFFu;   // pc_first_through: no query passes through that node

LCP2_HD u32 pc_bitlen(u32 x) { return x ? 32u - (u32)__builtin_clz(x) : 0u; }
LCP2_HD u32 pc_mask_below(u32 n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

// Query q in one tree.  merged: the lowest level at which an earlier query is on the same node (0: the same leaf; PC_NEVER: none),
// so q is the FIRST query through its node at the levels below `merged`.  stored: bit l set iff the sibling of level l is stored.
struct PcPlan {
  u32 merged, stored;
};
// x: the R query indices, shift: the tree's index_shift, nsib: its sibling count (<= 32)
LCP2_HD PcPlan pc_plan(const u32 *x, u32 R, u32 q, u32 shift, u32 nsib) {
  const u32 mine = x[q] >> shift;
  u32 merged = PC_NEVER, on_sibling = 0;
  for (u32 o = 0; o < R; o++) {
    const u32 b = pc_bitlen(mine ^ (x[o] >> shift));
    if (o < q && b < merged) merged = b;
    if (b) on_sibling |= 1u << (b - 1);
  }
  PcPlan p;
  p.merged = merged;
  p.stored = ~on_sibling & pc_mask_below(merged) & pc_mask_below(nsib);
  return p;
}
// the two predicates of the format
LCP2_HD bool pc_leaf_stored(PcPlan p) { return p.merged > 0; }
LCP2_HD bool pc_sibling_stored(PcPlan p, u32 level) { return (p.stored >> level) & 1u; }

// ---- word counts and offsets (a prefix sum over (tree, query, level) in format order)
LCP2_HD u32 pc_plan_words(PcPlan p, u32 leaf_len) { return (pc_leaf_stored(p) ? leaf_len : 0u) + 4u * (u32)__builtin_popcount(p.stored); }
// the words of a compressed proof in front of its trees, and the most a compressed proof of this layout takes
LCP2_HD u64 pc_outside_words(const VqLayout &V) { return V.queries + (V.proof_words - V.final_poly); }
LCP2_HD u64 pc_compressed_words_max(const VqLayout &V) { return V.proof_words; }
LCP2_HD u64 pc_tree_words(const VqLayout &V, const u32 *x, u32 t) {
  u64 words = 0;
  for (u32 q = 0; q < V.num_queries; q++) words += pc_plan_words(pc_plan(x, V.num_queries, q, V.tree[t].index_shift, V.tree[t].nsib), V.tree[t].leaf_len);
  return words;
}
LCP2_HD u64 pc_compressed_words(const VqLayout &V, const u32 *x) {
  u64 words = pc_outside_words(V);
  for (u32 t = 0; t < V.num_trees; t++) words += pc_tree_words(V, x, t);
  return words;
}
// where the stored sibling of level `level` lies, `at` being the offset of the query's first stored item
LCP2_HD u64 pc_level_offset(PcPlan p, u32 leaf_len, u64 at, u32 level) {
  return at + (pc_leaf_stored(p) ? leaf_len : 0u) + 4u * (u32)__builtin_popcount(p.stored & pc_mask_below(level));
}
// the first query whose path passes through node `node` of level `level`, PC_NONE if none does
LCP2_HD u32 pc_first_through(const u32 *x, u32 R, u32 shift, u32 level, u32 node) {
  for (u32 o = 0; o < R; o++)
    if (((x[o] >> shift) >> level) == node) return o;
  return PC_NONE;
}
// where the full layout keeps the leaf of (t, q); its 4 * nsib sibling words follow the leaf
LCP2_HD u64 pc_full_leaf(const VqLayout &V, u32 t, u32 q) { return V.queries + (u64)q * V.query_words + V.tree[t].leaf_off; }

// ---- compression of one tree: the stored items of `proof` (full layout) in format order into out; returns their word count
LCP2_HD u64 pc_compress_tree(const VqLayout &V, const u32 *x, u32 t, const u64 *proof, u64 *out) {
  const VqTree T = V.tree[t];
  u64 at = 0;
  for (u32 q = 0; q < V.num_queries; q++) {
    const PcPlan p = pc_plan(x, V.num_queries, q, T.index_shift, T.nsib);
    const u64 *leaf = proof + pc_full_leaf(V, t, q), *sib = leaf + T.leaf_len;
    if (pc_leaf_stored(p))
      for (u32 i = 0; i < T.leaf_len; i++) out[at++] = leaf[i];
    for (u32 l = 0; l < T.nsib; l++)
      if (pc_sibling_stored(p, l))
        for (u32 i = 0; i < 4; i++) out[at++] = sib[4 * l + i];
  }
  return at;
}

// ---- reconstruction of one tree, level by level, on one lane (the reference form of a workgroup of k_decompress_paths).
// comp: the tree's stored items (pc_tree_words of them); proof: the full layout, of which the leaf and the whole sibling list of
// every query of this tree are written.  Stored words are copied as they are; what enters a hash is canonicalised, as in
// vq_hash_or_noop.  Every node of a level that lies on a path has both children on a path (computed one level below) or stored by
// the first query through the other child, so every shared node is hashed once.  rc: the round constants.
LCP2_HD void pc_decompress_tree(const VqLayout &V, const u32 *x, u32 t, const u64 *comp, u64 *proof, const u64 *rc) {
  const VqTree T = V.tree[t];
  const u32 R = V.num_queries;
  PcPlan plan[VQ_MAX_QUERIES];
  u64 at[VQ_MAX_QUERIES];
  u64 cur[2][VQ_MAX_QUERIES][4];  // the digests of the current level, by the first query through each node (ping-pong)
  u64 words = 0;
  for (u32 q = 0; q < R; q++) {
    plan[q] = pc_plan(x, R, q, T.index_shift, T.nsib);
    at[q] = words;
    words += pc_plan_words(plan[q], T.leaf_len);
  }
  for (u32 q = 0; q < R; q++) {
    const u32 first = pc_first_through(x, R, T.index_shift, 0, x[q] >> T.index_shift);
    const u64 *leaf = comp + at[first];
    u64 *dst = proof + pc_full_leaf(V, t, q);
    for (u32 i = 0; i < T.leaf_len; i++) dst[i] = leaf[i];
    if (first == q) vq_hash_or_noop(leaf, T.leaf_len, cur[0][q], rc);
  }
  for (u32 l = 0; l < T.nsib; l++) {
    const u32 a = l & 1, b = a ^ 1;
    for (u32 q = 0; q < R; q++) {
      const u32 y = (x[q] >> T.index_shift) >> l;
      const u32 first = pc_first_through(x, R, T.index_shift, l, y), other = pc_first_through(x, R, T.index_shift, l, y ^ 1);
      const u64 *sib = other != PC_NONE ? cur[a][other] : comp + pc_level_offset(plan[first], T.leaf_len, at[first], l);
      u64 *dst = proof + pc_full_leaf(V, t, q) + T.leaf_len + 4 * l;
      for (u32 i = 0; i < 4; i++) dst[i] = sib[i];
      if (first != q) continue;
      u64 s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (u32 i = 0; i < 4; i++) {
        const u64 mine = cur[a][q][i], theirs = gl_canon(sib[i]);
        s[i] = (y & 1) ? theirs : mine;
        s[4 + i] = (y & 1) ? mine : theirs;
      }
      pos_permute(s, rc);
      for (u32 i = 0; i < 4; i++) cur[b][q][i] = s[i];
    }
  }
}

}  // namespace lcp2
