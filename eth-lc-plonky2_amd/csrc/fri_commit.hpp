// The FRI back end of both provers - the Plonk opening (prover_open.hip) and the openings of bare oracles (fri_openings.hip): column
// evaluation at a point, the commitment of one layer, the commit phase down to the final polynomial, the proof-of-work search, the
// query indices and the FRI-layer part of the query answers.  Host orchestration only (fri_commit.hip): no kernel and no launcher of
// its own, no allocation and no proof layout.  A caller describes the work area it owns with a FriWork and says where in its proof
// the caps, the final polynomial and the query rounds lie.
#pragma once
#include "circuit_state.hpp"

namespace lcp2 {

struct FriWork {
  u32 log_n, rate_bits, cap_height, num_layers, arity_bits[LCP2_MAX_FRI_LAYERS], final_len, pow_bits, num_queries;
  u64 *fri_c[2];  // ping-pong coefficient planes [2][n]; the committed polynomial is in fri_c[0]
  struct Layer {
    u64 *vals, *dig;                     // value planes [2][values()], digests of every level
    const u64 *d_level_off, *level_off;  // the node offset of each level inside dig, on the device and on the host
    u32 nlevels;                         // leaves to cap
  } layer[LCP2_MAX_FRI_LAYERS];
  u64 *d_pow;   // one word: the result of a proof-of-work batch
  u32 bf, bc;   // layer 0 covers the leaf blocks [bf, bf + bc) of 2^rate_bits only; bc = 0: all of them

  u32 capw() const { return 4u << cap_height; }
  u64 coeffs(u32 l) const { u64 m = 1ull << log_n; for (u32 k = 0; k < l; k++) m >>= arity_bits[k]; return m; }
  u64 values(u32 l) const { return l == 0 && bc ? (u64)bc * coeffs(0) : coeffs(l) << rate_bits; }  // per plane, as held
  u32 nsib(u32 l) const { return layer[l].nlevels - 1; }
  const u64 *d_cap(u32 l) const { return layer[l].dig + 4 * layer[l].level_off[layer[l].nlevels - 1]; }
};

// ---- `ncols` (<= 65535: they are the grid's y) coefficient columns [ncols][n] at z: d_out[2 * ncols].  d_tab: eval_tables of z,
// eval_table_words(n) words, made once per point; d_partial: scratch of 2 * ncols * (n / eval_chunk_len(n)) words
u32 eval_chunk_len(u64 n);
size_t eval_table_words(u64 n);
void eval_tables(hipStream_t s, u64 n, gl2 z, u64 *d_tab);  // z travels in the kernel arguments: no staging copy, no synchronisation
void eval_columns(hipStream_t s, const u64 *coeffs, u32 ncols, u64 n, gl2 z, const u64 *d_tab, u64 *d_partial, u64 *d_out);

// LDE of the m coefficients in fri_c[cur] (the zero padding is implicit), leaf hashing and Merkle levels of layer l; then the cap
// into cap_out - unless cap_out is null: the caller copies w.d_cap(l) itself (a sharded layer 0, whose cap is a share of the cap)
int fri_commit_layer(lcp2_ctx *ctx, const FriWork &w, u32 l, int cur, u64 m, u64 shift, u64 *cap_out);
// The commit phase down to the final polynomial: per layer commit (layer 0 not if the caller has committed it and its cap is in
// caps_out already), observe the cap, draw beta, fold.  caps_out: capw() words per layer; betas_out: null or [num_layers];
// final_poly_out: 2 * final_len words, interleaved
int fri_commit_phase(lcp2_ctx *ctx, const FriWork &w, HostChallenger &ch, bool first_layer_committed, u64 *caps_out, gl2 *betas_out, u64 *final_poly_out);
// the smallest witness (0 bits: every witness passes, 0 is the smallest and nothing is launched), observed; the response is drawn
int fri_proof_of_work(lcp2_ctx *ctx, const FriWork &w, HostChallenger &ch, u64 *witness_out);
// idx[1 + num_layers][num_queries]: the queried leaf of the initial trees, then of every layer
void fri_draw_indices(const FriWork &w, HostChallenger &ch, std::vector<u64> &idx);

// ---- the FRI-layer part of the query answers: gathered into a side buffer, copied back by the caller, scattered into the rounds.
// Per layer the leaves of all queries (2 << arity_bits words each), then their siblings (4 * nsib words each)
struct FriSide {
  size_t leaf[LCP2_MAX_FRI_LAYERS], sib[LCP2_MAX_FRI_LAYERS];
};
size_t fri_side_layout(const FriWork &w, size_t at, FriSide &o);  // from word `at` on; returns the end
// d_leaf_of_layer[l]: the num_queries leaf indices of layer l, as the layer is held
void fri_gather_layers(lcp2_ctx *ctx, const FriWork &w, const u64 *const *d_leaf_of_layer, u64 *d_side, const FriSide &o);
// rounds: query_words words per query, layer l at step_off[l]; skip_layer0(q): leave layer 0 of query q as it is
template <class Off, class Skip>
inline void fri_scatter_layers(const FriWork &w, const u64 *side, const FriSide &o, u64 *rounds, size_t query_words, const Off *step_off, Skip skip_layer0) {
  for (u32 q = 0; q < w.num_queries; q++)
    for (u32 l = 0; l < w.num_layers; l++) {
      if (l == 0 && skip_layer0(q)) continue;
      const size_t words = (size_t)2 << w.arity_bits[l], sibw = (size_t)4 * w.nsib(l);
      u64 *R = rounds + (size_t)q * query_words + step_off[l];
      memcpy(R, side + o.leaf[l] + q * words, words * 8);
      memcpy(R + words, side + o.sib[l] + q * sibw, sibw * 8);
    }
}

}  // namespace lcp2
