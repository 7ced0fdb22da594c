// The batched opening (OpeningSet::new + PolynomialBatch::prove_openings): openings, final polynomial, FRI commit phase, proof of
// work and the query answers.  Host orchestration over the kernels of kernels_prover.hip / kernels_hash.hip.
#include "circuit_state.hpp"

using namespace lcp2;

namespace {
// evaluate `ncols` coefficient columns at z; results (ext) land in d_out[2 * ncols].  d_tab: the power tables of z (eval_tables)
u32 eval_chunk_len(u64 n) { return (u32)std::min<u64>(n, EVAL_CHUNK); }
size_t eval_table_words(u64 n) { return 512 + 2 * (size_t)(n / eval_chunk_len(n)); }
void eval_tables(lcp2_circuit *c, gl2 z, u64 *d_tab) {  // z travels in the kernel arguments: no staging copy, no synchronisation
  const u64 n = 1ull << c->p.degree_bits;
  launch_eval_tables(c->ctx->stream, z.c0, z.c1, eval_chunk_len(n), (u32)(n / eval_chunk_len(n)), d_tab);
}
void eval_columns(lcp2_circuit *c, const u64 *coeffs, u32 ncols, gl2 z, u64 *d_out, const u64 *d_tab) {
  const u64 n = 1ull << c->p.degree_bits;
  EvalArgs a{};
  a.coeffs = coeffs; a.col_stride = n;
  a.chunk_len = eval_chunk_len(n);
  a.items = (a.chunk_len + 255) / 256;
  a.nchunks = (u32)(n / a.chunk_len);
  const gl2 zs = gl2_pow(z, 256);
  a.zstep[0] = zs.c0; a.zstep[1] = zs.c1;
  a.zpow_t = d_tab; a.zpow_chunk = d_tab + 512;
  a.partial = c->partial.u();
  launch_eval_polys(c->ctx->stream, a, ncols, d_out);
}
}  // namespace

// OpeningSet::new + PolynomialBatch::prove_openings (K7-K9, a13) in three phases (state in c->fo).  The challenger has observed
// everything up to the quotient cap and zeta was drawn from it; at the end it has absorbed the openings, the FRI caps, the final
// polynomial and the PoW witness and produced the query indices.  Together the phases write proof words [op_constants, total).
//
// A coset-sharded circuit (rank = bf / bc of world = 2^rate_bits / bc) does a share of the first two phases:
//   openings: the columns column_shard(rank) of every oracle (each rank holds all coefficients); zeros for the others
//   commit:   FRI layer 0 (the big one: LDE, leaf hashing, Merkle levels) for its own leaf blocks; its cap entries at their
//             global position.  Folding happens in coefficient form, so no values cross the ranks.
// and the caller sums the shares (lcp2_proof_section) before the next phase.
int lcp2::fri_open_openings(lcp2_circuit *c, u64 *proof) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; const ProofLayout &L = e.L;
  const u64 n = e.n; const u32 W = e.W, CH = e.CH, Q = e.Q, npp = e.npp, ncs = e.ncs;
  if (c->stage != lcp2_circuit::ST_QUOT) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_open: the quotient is not committed");
  if (!c->cap_final) return ctx->fail(LCP2_E_INVALID, "sharded circuit: lcp2_circuit_set_constants_cap has not been called");
  FriOpenState &fo = c->fo;
  const gl2 zeta = fo.zeta, g_zeta = gl2_scale(zeta, gl_root_of_unity(p.degree_bits));
  // k_divide_finalize divides by X - zeta and X - g zeta through the inverse powers of zeta and g zeta (k_compose_tables):
  // zeta = 0, and with it g zeta = 0, has none.  Refused before anything is written; the handle keeps its state.
  if ((zeta.c0 | zeta.c1) == 0 || (g_zeta.c0 | g_zeta.c1) == 0)
    return ctx->fail(LCP2_E_INVALID, "lcp2_fri_open: zeta = 0 is not supported (the opening divides by powers of zeta and of g zeta)");
  const auto oracles = c->oracles();
  memset(proof + L.op_constants, 0, (L.total - L.op_constants) * 8);
  // the power tables of zeta and g zeta (device-made), every oracle's columns evaluated back to back, ONE copy back
  u64 *d_tab = c->tables.u(), *d_tab_g = d_tab + eval_table_words(n);
  const u32 all_cols = ncs + W + CH * (1 + npp) + CH * Q + CH;
  LCP2_HIP(ctx, c->open_out.ensure((size_t)2 * all_cols * 8));
  u64 *d_open = c->open_out.u();
  std::vector<u64> tmp((size_t)2 * all_cols);
  u32 at_col[5], first_col[4], num_cols[4], pos = 0, share_cols = 0;
  for (int o = 0; o < 4; o++) { c->column_share(oracles[o]->ncols, first_col[o], num_cols[o]); share_cols += num_cols[o]; }
  ProfScope ps(ctx, LCP2_K_OPENINGS, 8.0 * n * (share_cols + CH));
  eval_tables(c, zeta, d_tab);
  const bool with_next = !c->sharded() || c->bf == 0;
  if (with_next) eval_tables(c, g_zeta, d_tab_g);
  for (int o = 0; o < 4; o++) {
    at_col[o] = pos;
    if (num_cols[o]) eval_columns(c, oracles[o]->coeffs.u() + (size_t)first_col[o] * n, num_cols[o], zeta, d_open + 2 * pos, d_tab);
    pos += num_cols[o];
  }
  at_col[4] = pos;
  if (with_next) { eval_columns(c, c->zs.coeffs.u(), CH, g_zeta, d_open + 2 * pos, d_tab_g); pos += CH; }
  LCP2_HIP(ctx, hipGetLastError());
  LCP2_TRY(download(ctx, tmp.data(), d_open, (size_t)2 * pos * 8));
  for (int o = 0; o < 4; o++)
    for (u32 j = 0; j < num_cols[o]; j++) {
      const u32 col = first_col[o] + j;
      size_t at = o == 0 ? L.op_constants + 2 * col   // constants then sigmas, contiguous
                : o == 1 ? L.op_wires + 2 * col
                : o == 2 ? (col < CH ? L.op_zs + 2 * col : L.op_pp + 2 * (col - CH))
                         : L.op_quot + 2 * col;
      proof[at] = tmp[2 * (at_col[o] + j)]; proof[at + 1] = tmp[2 * (at_col[o] + j) + 1];
    }
  if (with_next) memcpy(proof + L.op_zs_next, tmp.data() + 2 * at_col[4], 2 * CH * 8);
  fo.phase = 1;
  return LCP2_OK;
}

// LDE of the coefficients in fri_c[cur] (m of them, zero padding to 8m implicit), leaf hashing and Merkle levels of FRI layer l;
// the cap lands in the proof.  Layer 0 of a sharded circuit covers its own leaf blocks.
static int fri_commit_layer(lcp2_circuit *c, u32 l, int cur, u64 m, u64 shift, u64 *proof) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; const ProofLayout &L = e.L; hipStream_t s = e.s;
  const u32 ab = p.fri_arity_bits[l], arity = 1u << ab;
  const bool part = l == 0 && c->sharded();
  u32 lgm = 0;
  while ((1ull << lgm) < m) lgm++;
  const u64 nvals = part ? (u64)c->bc * m : m << p.rate_bits, nleaves = nvals >> ab;
  u64 *vals = c->fri_vals[l].u();
  {
    ProfScope ps(ctx, LCP2_K_FRI, 16.0 * m + 16.0 * nvals + 32.0 * nleaves);
    // coset_fft of the zero-padded coefficients = 2^rate_bits coset transforms of the m coefficients; leaf order out
    if (part) e.ntt.forward(c->fri_c[cur].u(), m, vals, nvals, lgm, 2, shift, p.rate_bits, c->bf, c->bc);
    else e.ntt.forward(c->fri_c[cur].u(), m, vals, nvals, lgm, 2, shift, p.rate_bits);
    if (e.be.status) return e.be.status;
    launch_hash_ext_leaves(s, vals, vals + nvals, arity, nleaves, c->fri_dig[l].u(), ctx->d_rc);
    const auto &off = c->fri_level_off[l];
    for (size_t k = 1; k < off.size(); k++)
      launch_merkle_level(s, c->fri_dig[l].u() + 4 * off[k - 1], c->fri_dig[l].u() + 4 * off[k], nleaves >> k, ctx->d_rc);
  }
  LCP2_HIP(ctx, hipGetLastError());
  u64 *cap = proof + L.fri_caps + l * L.capw;
  const u64 *d_cap = c->fri_dig[l].u() + 4 * c->fri_level_off[l].back();
  if (!part) return download(ctx, cap, d_cap, L.capw * 8);
  Download d(ctx);
  LCP2_TRY(queue_cap(d, c, d_cap, cap));
  return d.wait();
}

int lcp2::fri_open_commit(lcp2_circuit *c, u64 *proof) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; const ProofLayout &L = e.L; hipStream_t s = e.s;
  const u64 n = e.n; const u32 W = e.W, CH = e.CH, Q = e.Q, npp = e.npp, ncs = e.ncs;
  FriOpenState &fo = c->fo;
  if (fo.phase != 1) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_open_commit: call lcp2_fri_open_begin first");
  HostChallenger &ch = fo.ch;
  const gl2 zeta = fo.zeta;
  const auto oracles = c->oracles();
  ch.observe_n(proof + L.op_constants, 2 * (ncs + W));
  ch.observe_n(proof + L.op_zs, 2 * CH);
  ch.observe_n(proof + L.op_pp, 2 * CH * npp);
  ch.observe_n(proof + L.op_quot, 2 * CH * Q);
  ch.observe_n(proof + L.op_zs_next, 2 * CH);

  // ---- K7b: final polynomial of the batched opening
  const gl2 alpha = fo.alpha = ch.get_ext();
  {
    const u32 total_polys = ncs + W + CH * (1 + npp) + CH * Q;
    const u32 h = (p.degree_bits + 1) / 2;
    const u64 hi_count = (n >> h) + 1;
    // alpha^j and the two-level power tables of zeta, g zeta and their inverses: made on the device from the two challenges in
    // the kernel arguments (k_compose_tables; the host used to spend 0.3 ms here, then copy and synchronise)
    const size_t per = (size_t)2 * ((1ull << h) + hi_count);
    size_t off[4][2];
    for (int b = 0; b < 4; b++) { off[b][0] = (size_t)2 * total_polys + b * per; off[b][1] = off[b][0] + ((size_t)2 << h); }
    if (((size_t)2 * total_polys + 4 * per) * 8 > c->tables.bytes) return ctx->fail(LCP2_E_INVALID, "internal: table workspace too small");
    launch_compose_tables(s, alpha.c0, alpha.c1, zeta.c0, zeta.c1, gl_root_of_unity(p.degree_bits), total_polys, h, hi_count, c->tables.u());
    ComposeArgs a{};
    for (int o = 0; o < 4; o++) { a.coeffs[o] = oracles[o]->coeffs.u(); a.ncols[o] = oracles[o]->ncols; }
    a.num_challenges = CH; a.n = n;
    const u64 *T = c->tables.u();
    a.alpha_pows = T;
    a.z0_lo = T + off[0][0]; a.z0_hi = T + off[0][1]; a.z1_lo = T + off[1][0]; a.z1_hi = T + off[1][1];
    a.zi0_lo = T + off[2][0]; a.zi0_hi = T + off[2][1]; a.zi1_lo = T + off[3][0]; a.zi1_hi = T + off[3][1];
    a.zh = h; a.zmask = (1ull << h) - 1;
    gl2 ash = gl2_pow(alpha, CH);
    a.alpha_shift[0] = ash.c0; a.alpha_shift[1] = ash.c1;
    a.planes = c->planes.u();
    ProfScope ps(ctx, LCP2_K_OPENINGS, 8.0 * n * (total_polys + CH));
    launch_compose(s, a);
    launch_scan(s, false, c->planes.u(), c->planes.u(), c->scan_tmp.u(), n, true, 4, n);
    launch_divide_finalize(s, a, c->fri_c[0].u(), c->fri_c[0].u() + n);
  }
  LCP2_HIP(ctx, hipGetLastError());
  if (p.num_fri_layers) LCP2_TRY(fri_commit_layer(c, 0, 0, n, GL_GENERATOR, proof));
  fo.phase = 2;
  return LCP2_OK;
}

// ---- the last phase in its four steps; each continues from what the one before left in c->fo and the proof
namespace {
// K8: the FRI commit phase (layer 0 is committed already) down to the final polynomial
int fri_commit_phase(lcp2_circuit *c, u64 *proof) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p; hipStream_t s = ctx->stream; HostChallenger &ch = c->fo.ch;
  const ProofLayout L(p);
  u64 m = 1ull << p.degree_bits;  // number of (possibly) non-zero coefficients; the zero padding to 8m is implicit
  u64 shift = GL_GENERATOR;
  int cur = 0;
  for (u32 l = 0; l < p.num_fri_layers; l++) {
    const u32 ab = p.fri_arity_bits[l], arity = 1u << ab;
    if (l) LCP2_TRY(fri_commit_layer(c, l, cur, m, shift, proof));
    ch.observe_n(proof + L.fri_caps + l * L.capw, L.capw);
    gl2 beta = ch.get_ext();
    c->fo.fri_betas[l] = beta;
    {
      ProfScope ps(ctx, LCP2_K_FRI, 16.0 * m + 16.0 * (m >> ab));
      launch_fri_fold(s, c->fri_c[cur].u(), c->fri_c[cur].u() + m, c->fri_c[cur ^ 1].u(), c->fri_c[cur ^ 1].u() + (m >> ab), m >> ab, arity, beta.c0, beta.c1);
    }
    cur ^= 1;
    m >>= ab;
    shift = gl_pow(shift, arity);
  }
  if (m != L.final_len) return ctx->fail(LCP2_E_INVALID, "internal: final polynomial length mismatch");
  std::vector<u64> f(2 * m);
  LCP2_TRY(download(ctx, f.data(), c->fri_c[cur].u(), 2 * m * 8));
  for (u64 i = 0; i < m; i++) { proof[L.final_poly + 2 * i] = f[i]; proof[L.final_poly + 2 * i + 1] = f[m + i]; }
  ch.observe_n(proof + L.final_poly, 2 * L.final_len);
  return LCP2_OK;
}

// K9: proof of work, minimum witness
int fri_proof_of_work(lcp2_circuit *c, u64 *proof) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p; hipStream_t s = ctx->stream; HostChallenger &ch = c->fo.ch;
  u64 res = ~0ull;
  {
    PowArgs a{};
    ch.pow_state(a.state, a.pos);
    a.bits = p.proof_of_work_bits; a.rc = ctx->d_rc;
    u64 *d_res = c->small.u() + SMALL_POW;
    a.result = d_res;
    const u64 batch = 1ull << 20;
    ProfScope ps(ctx, LCP2_K_POW, 0.0);
    for (u64 start = 0; res == ~0ull; start += batch) {
      if (start >= (1ull << 44)) return ctx->fail(LCP2_E_UNSUPPORTED, "proof of work not found");
      { SmallWords w{}; w.v[0] = ~0ull; launch_set_words(s, d_res, w, 1); }
      a.start = start;
      launch_pow_search(s, a, batch);
      LCP2_TRY(download(ctx, &res, d_res, 8));
    }
  }
  c->fo.pow_witness = proof[ProofLayout(p).pow_witness] = res;
  ch.observe(res);
  if ((ch.get() >> (64 - p.proof_of_work_bits)) != 0) return ctx->fail(LCP2_E_HIP, "internal: proof-of-work self check failed");
  return LCP2_OK;
}

// a sharded circuit answers the initial-tree and FRI-layer-0 parts of the queries whose leaf it holds and leaves zeros for
// the others (its share of the proof); the smaller FRI layers are replicated on every rank
bool holds_leaf(const lcp2_circuit *c, u64 leaf) {
  const u64 n = 1ull << c->p.degree_bits, leaf0 = (u64)c->bf * n;
  return leaf >= leaf0 && leaf < leaf0 + (u64)c->nblocks() * n;
}

// the query indices: drawn from the challenger, uploaded as [1 + layers][Qn] global leaves, [Qn] local leaves of the initial
// trees, [Qn] local leaves of FRI layer 0
int fri_query_indices(lcp2_circuit *c, u64 *) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p;
  std::vector<u64> &idx = c->fo.idx, &up = c->fo.idx_up;
  const u32 Qn = p.num_query_rounds;
  const u64 n = 1ull << p.degree_bits, N = n << p.rate_bits;
  idx.assign(Qn * (1 + p.num_fri_layers), 0);
  for (u32 q = 0; q < Qn; q++) {
    u64 x = c->fo.ch.get() % N;
    idx[q] = x;
    u64 xi = x;
    for (u32 l = 0; l < p.num_fri_layers; l++) { xi >>= p.fri_arity_bits[l]; idx[(1 + l) * Qn + q] = xi; }
  }
  up = idx;
  for (u32 q = 0; q < Qn; q++) up.push_back(holds_leaf(c, idx[q]) ? idx[q] - (u64)c->bf * n : 0);
  for (u32 q = 0; q < Qn; q++) up.push_back(p.num_fri_layers ? up[idx.size() + q] >> p.fri_arity_bits[0] : 0);  // layer-0 leaf, local
  if (ctx->pin && up.size() * 8 <= lcp2_ctx::PIN_BYTES) {  // through the pinned staging buffer (every earlier download has been waited for)
    memcpy(ctx->pin, up.data(), up.size() * 8);
    LCP2_HIP(ctx, hipMemcpyAsync(c->q_idx.p, ctx->pin, up.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  } else {
    LCP2_HIP(ctx, hipMemcpyAsync(c->q_idx.p, up.data(), up.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  return LCP2_OK;
}

// query phase: gather leaves and Merkle paths on the device, one copy back, and scatter them into the query rounds of the proof
int fri_answer_queries(lcp2_circuit *c, u64 *proof) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p; hipStream_t s = ctx->stream;
  const ProofLayout L(p);
  const std::vector<u64> &idx = c->fo.idx;
  const auto oracles = c->oracles();
  const u32 Qn = p.num_query_rounds;
  const u64 n = 1ull << p.degree_bits, N = n << p.rate_bits, nlocal = (u64)c->nblocks() * n;
  u64 *d_idx = c->q_idx.u();
  const u64 *d_idx_local = d_idx + idx.size(), *d_idx_local0 = d_idx_local + Qn;
  u64 *buf = c->q_buf.u();
  size_t pos = 0;
  size_t o_leaf[4], o_sib[4], f_leaf[LCP2_MAX_FRI_LAYERS], f_sib[LCP2_MAX_FRI_LAYERS];
  for (int o = 0; o < 4; o++) {
    o_leaf[o] = pos; pos += (size_t)Qn * oracles[o]->ncols;
    o_sib[o] = pos; pos += (size_t)Qn * L.q_init_sib * 4;
    const lcp2_oracle &O = *oracles[o];
    launch_gather_rows(s, O.lde.u(), O.nleaves(), O.ncols, d_idx_local, Qn, buf + o_leaf[o]);
    launch_gather_digests(s, O.digests.u(), O.d_level_off.u(), O.nlevels() - 1, d_idx_local, Qn, buf + o_sib[o]);
  }
  for (u32 l = 0; l < p.num_fri_layers; l++) {
    const u32 arity = 1u << p.fri_arity_bits[l];
    u64 nvals = N;  // values of layer l: N >> (arity bits of the layers before it)
    for (u32 k = 0; k < l; k++) nvals >>= p.fri_arity_bits[k];
    if (l == 0) nvals = nlocal;
    const u64 *d_leaf = l == 0 ? d_idx_local0 : d_idx + (1 + l) * Qn;
    f_leaf[l] = pos; pos += (size_t)Qn * 2 * arity;
    f_sib[l] = pos; pos += (size_t)Qn * L.q_step_sib[l] * 4;
    launch_gather_ext_leaves(s, c->fri_vals[l].u(), c->fri_vals[l].u() + nvals, arity, d_leaf, Qn, buf + f_leaf[l]);
    launch_gather_digests(s, c->fri_dig[l].u(), c->fri_d_level_off[l].u(), (u32)L.q_step_sib[l], d_leaf, Qn, buf + f_sib[l]);
  }
  LCP2_HIP(ctx, hipGetLastError());
  if (pos * 8 > c->q_buf.bytes) return ctx->fail(LCP2_E_INVALID, "internal: query workspace too small");
  std::vector<u64> h(pos);
  LCP2_TRY(download(ctx, h.data(), buf, pos * 8));
  for (u32 q = 0; q < Qn; q++) {
    u64 *R = proof + L.queries + (size_t)q * L.query_words;
    const bool mine = holds_leaf(c, idx[q]);
    for (int o = 0; o < 4 && mine; o++) {
      u32 nc = oracles[o]->ncols;
      memcpy(R + L.q_init_off[o], h.data() + o_leaf[o] + (size_t)q * nc, nc * 8);
      memcpy(R + L.q_init_off[o] + nc, h.data() + o_sib[o] + (size_t)q * L.q_init_sib * 4, L.q_init_sib * 32);
    }
    for (u32 l = 0; l < p.num_fri_layers; l++) {
      if (l == 0 && !mine) continue;
      const u32 arity = 1u << p.fri_arity_bits[l];
      memcpy(R + L.q_step_off[l], h.data() + f_leaf[l] + (size_t)q * 2 * arity, 2 * arity * 8);
      memcpy(R + L.q_step_off[l] + 2 * arity, h.data() + f_sib[l] + (size_t)q * L.q_step_sib[l] * 4, L.q_step_sib[l] * 32);
    }
  }
  // Shares must SUM to the proof (RCCL has no bitwise reductions): the words every rank holds identically (openings,
  // FRI caps, the smaller FRI layers, final polynomial, PoW witness) are contributed by the rank that holds leaf block 0 only.
  if (c->sharded() && c->bf != 0) {
    std::vector<u64> keep(proof + L.queries, proof + L.queries + (size_t)Qn * L.query_words);
    memset(proof + L.op_constants, 0, (L.total - L.op_constants) * 8);
    const size_t own_words = p.num_fri_layers >= 2 ? L.q_step_off[1] : L.query_words;  // initial trees and FRI layer 0 come first
    for (u32 q = 0; q < Qn; q++)
      if (holds_leaf(c, idx[q])) memcpy(proof + L.queries + (size_t)q * L.query_words, keep.data() + (size_t)q * L.query_words, own_words * 8);
  }
  return LCP2_OK;
}
}  // namespace

int lcp2::fri_open_finish(lcp2_circuit *c, u64 *proof) {
  LCP2_TRY(select_device(c->ctx));
  if (c->fo.phase != 2) return c->ctx->fail(LCP2_E_INVALID, "lcp2_fri_open_finish: call lcp2_fri_open_commit first");
  c->fo.phase = 0;
  LCP2_TRY(fri_commit_phase(c, proof));
  LCP2_TRY(fri_proof_of_work(c, proof));
  LCP2_TRY(fri_query_indices(c, proof));
  return fri_answer_queries(c, proof);
}
