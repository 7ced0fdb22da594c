// fri_commit.hpp: the one text of the FRI back end.  Host orchestration over the launchers of kernels_prover.hip / kernels_hash.hip
// and the device transforms; both provers (prover_open.hip, fri_openings.hip) call it.
#include "fri_commit.hpp"

namespace lcp2 {

u32 eval_chunk_len(u64 n) { return (u32)std::min<u64>(n, EVAL_CHUNK); }
size_t eval_table_words(u64 n) { return 512 + 2 * (size_t)(n / eval_chunk_len(n)); }
void eval_tables(hipStream_t s, u64 n, gl2 z, u64 *d_tab) {
  launch_eval_tables(s, z.c0, z.c1, eval_chunk_len(n), (u32)(n / eval_chunk_len(n)), d_tab);
}
void eval_columns(hipStream_t s, const u64 *coeffs, u32 ncols, u64 n, gl2 z, const u64 *d_tab, u64 *d_partial, u64 *d_out) {
  EvalArgs a{};
  a.coeffs = coeffs; a.col_stride = n;
  a.chunk_len = eval_chunk_len(n);
  a.items = (a.chunk_len + 255) / 256;
  a.nchunks = (u32)(n / a.chunk_len);
  const gl2 zs = gl2_pow(z, 256);
  a.zstep[0] = zs.c0; a.zstep[1] = zs.c1;
  a.zpow_t = d_tab; a.zpow_chunk = d_tab + 512;
  a.partial = d_partial;
  launch_eval_polys(s, a, ncols, d_out);
}

int fri_commit_layer(lcp2_ctx *ctx, const FriWork &w, u32 l, int cur, u64 m, u64 shift, u64 *cap_out) {
  hipStream_t s = ctx->stream;
  const FriWork::Layer &y = w.layer[l];
  const u32 arity = 1u << w.arity_bits[l];
  u32 lgm = 0;
  while ((1ull << lgm) < m) lgm++;
  const u64 nvals = w.values(l), nleaves = nvals >> w.arity_bits[l];
  DeviceNttBackend be{ctx};
  NttHost<DeviceNttBackend> ntt(be);
  {
    ProfScope ps(ctx, LCP2_K_FRI, 16.0 * m + 16.0 * nvals + 32.0 * nleaves);
    // coset_fft of the zero-padded coefficients = 2^rate_bits coset transforms of the m coefficients (the held blocks of them); leaf order out
    ntt.forward(w.fri_c[cur], m, y.vals, nvals, lgm, 2, shift, w.rate_bits, l ? 0 : w.bf, l ? 0 : w.bc);
    if (be.status) return be.status;
    launch_hash_ext_leaves(s, y.vals, y.vals + nvals, arity, nleaves, y.dig, ctx->d_rc);
    for (u32 k = 1; k < y.nlevels; k++)
      launch_merkle_level(s, y.dig + 4 * y.level_off[k - 1], y.dig + 4 * y.level_off[k], nleaves >> k, ctx->d_rc);
  }
  LCP2_HIP(ctx, hipGetLastError());
  return cap_out ? download(ctx, cap_out, w.d_cap(l), (size_t)w.capw() * 8) : LCP2_OK;
}

int fri_commit_phase(lcp2_ctx *ctx, const FriWork &w, HostChallenger &ch, bool first_layer_committed, u64 *caps_out, gl2 *betas_out, u64 *final_poly_out) {
  u64 m = 1ull << w.log_n;  // number of (possibly) non-zero coefficients
  u64 shift = GL_GENERATOR;
  int cur = 0;
  for (u32 l = 0; l < w.num_layers; l++) {
    const u32 ab = w.arity_bits[l], arity = 1u << ab;
    u64 *cap = caps_out + (size_t)l * w.capw();
    if (l || !first_layer_committed) LCP2_TRY(fri_commit_layer(ctx, w, l, cur, m, shift, cap));
    ch.observe_n(cap, w.capw());
    const gl2 beta = ch.get_ext();
    if (betas_out) betas_out[l] = beta;
    {
      ProfScope ps(ctx, LCP2_K_FRI, 16.0 * m + 16.0 * (m >> ab));
      launch_fri_fold(ctx->stream, w.fri_c[cur], w.fri_c[cur] + m, w.fri_c[cur ^ 1], w.fri_c[cur ^ 1] + (m >> ab), m >> ab, arity, beta.c0, beta.c1);
    }
    cur ^= 1;
    m >>= ab;
    shift = gl_pow(shift, arity);
  }
  if (m != w.final_len) return ctx->fail(LCP2_E_INVALID, "internal: final polynomial length mismatch");
  std::vector<u64> f(2 * m);
  LCP2_TRY(download(ctx, f.data(), w.fri_c[cur], 2 * m * 8));
  for (u64 i = 0; i < m; i++) { final_poly_out[2 * i] = f[i]; final_poly_out[2 * i + 1] = f[m + i]; }
  ch.observe_n(final_poly_out, 2 * (size_t)w.final_len);
  return LCP2_OK;
}

int fri_proof_of_work(lcp2_ctx *ctx, const FriWork &w, HostChallenger &ch, u64 *witness_out) {
  u64 witness = 0;
  if (w.pow_bits) {
    PowArgs a{};
    ch.pow_state(a.state, a.pos);
    a.bits = w.pow_bits; a.rc = ctx->d_rc; a.result = w.d_pow;
    const u64 batch = 1ull << 20;
    witness = ~0ull;
    ProfScope ps(ctx, LCP2_K_POW, 0.0);
    for (u64 start = 0; witness == ~0ull; start += batch) {
      if (start >= (1ull << 44)) return ctx->fail(LCP2_E_UNSUPPORTED, "proof of work not found");
      { SmallWords r{}; r.v[0] = ~0ull; launch_set_words(ctx->stream, a.result, r, 1); }
      a.start = start;
      launch_pow_search(ctx->stream, a, batch);
      LCP2_TRY(download(ctx, &witness, a.result, 8));
    }
  }
  *witness_out = witness;
  ch.observe(witness);
  const u64 response = ch.get();
  if (w.pow_bits && (response >> (64 - w.pow_bits)) != 0) return ctx->fail(LCP2_E_HIP, "internal: proof-of-work self check failed");
  return LCP2_OK;
}

void fri_draw_indices(const FriWork &w, HostChallenger &ch, std::vector<u64> &idx) {
  const u32 Qn = w.num_queries;
  const u64 N = 1ull << (w.log_n + w.rate_bits);
  idx.assign((size_t)Qn * (1 + w.num_layers), 0);
  for (u32 q = 0; q < Qn; q++) {
    u64 xi = ch.get() % N;
    idx[q] = xi;
    for (u32 l = 0; l < w.num_layers; l++) { xi >>= w.arity_bits[l]; idx[(size_t)(1 + l) * Qn + q] = xi; }
  }
}

size_t fri_side_layout(const FriWork &w, size_t at, FriSide &o) {
  for (u32 l = 0; l < w.num_layers; l++) {
    o.leaf[l] = at; at += (size_t)w.num_queries * (2u << w.arity_bits[l]);
    o.sib[l] = at; at += (size_t)w.num_queries * 4 * w.nsib(l);
  }
  return at;
}

void fri_gather_layers(lcp2_ctx *ctx, const FriWork &w, const u64 *const *d_leaf_of_layer, u64 *d_side, const FriSide &o) {
  for (u32 l = 0; l < w.num_layers; l++) {
    const FriWork::Layer &y = w.layer[l];
    launch_gather_ext_leaves(ctx->stream, y.vals, y.vals + w.values(l), 1u << w.arity_bits[l], d_leaf_of_layer[l], w.num_queries, d_side + o.leaf[l]);
    launch_gather_digests(ctx->stream, y.dig, y.d_level_off, w.nsib(l), d_leaf_of_layer[l], w.num_queries, d_side + o.sib[l]);
  }
}

}  // namespace lcp2
