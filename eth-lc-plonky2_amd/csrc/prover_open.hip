// The batched opening (OpeningSet::new + PolynomialBatch::prove_openings): openings, final polynomial, FRI commit phase, proof of
// work and the query answers.  Host orchestration over the kernels of kernels_prover.hip / kernels_hash.hip.  What is the Plonk
// opening's own is here: its openings, its compose / scan / divide, the initial-tree gathers, the share of a coset-sharded circuit
// and the three phases; the FRI back end (layer commitment, commit phase, proof of work, query indices, layer answers) is
// fri_commit.hip, shared with the openings of bare oracles (fri_openings.hip).
#include "circuit_state.hpp"
#include "fri_commit.hpp"

using namespace lcp2;

namespace {
// the FRI work area of the handle (allocated by prover_build.hip), as fri_commit.hpp takes it
FriWork fri_work_of(lcp2_circuit *c) {
  const lcp2_params &p = c->p;
  FriWork w{};
  w.log_n = p.degree_bits; w.rate_bits = p.rate_bits; w.cap_height = p.cap_height; w.num_layers = p.num_fri_layers;
  w.final_len = (u32)ProofLayout(p).final_len; w.pow_bits = p.proof_of_work_bits; w.num_queries = p.num_query_rounds;
  w.fri_c[0] = c->fri_c[0].u(); w.fri_c[1] = c->fri_c[1].u();
  for (u32 l = 0; l < p.num_fri_layers; l++) {
    w.arity_bits[l] = p.fri_arity_bits[l];
    w.layer[l] = {c->fri_vals[l].u(), c->fri_dig[l].u(), c->fri_d_level_off[l].u(), c->fri_level_off[l].data(), (u32)c->fri_level_off[l].size()};
  }
  w.d_pow = c->small.u() + SMALL_POW;
  w.bf = c->bf; w.bc = c->bc;
  return w;
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
  hipStream_t s = e.s;
  u64 *d_partial = c->partial.u();
  eval_tables(s, n, zeta, d_tab);
  const bool with_next = !c->sharded() || c->bf == 0;
  if (with_next) eval_tables(s, n, g_zeta, d_tab_g);
  for (int o = 0; o < 4; o++) {
    at_col[o] = pos;
    if (num_cols[o]) eval_columns(s, oracles[o]->coeffs.u() + (size_t)first_col[o] * n, num_cols[o], n, zeta, d_tab, d_partial, d_open + 2 * pos);
    pos += num_cols[o];
  }
  at_col[4] = pos;
  if (with_next) { eval_columns(s, c->zs.coeffs.u(), CH, n, g_zeta, d_tab_g, d_partial, d_open + 2 * pos); pos += CH; }
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
  // FRI layer 0 here, so that the shards can exchange its cap before the last phase; a sharded circuit covers its own leaf blocks
  if (p.num_fri_layers) {
    const FriWork w = fri_work_of(c);
    u64 *cap = proof + L.fri_caps;
    LCP2_TRY(fri_commit_layer(ctx, w, 0, 0, n, GL_GENERATOR, c->sharded() ? nullptr : cap));
    if (c->sharded()) {
      Download d(ctx);
      LCP2_TRY(queue_cap(d, c, w.d_cap(0), cap));
      LCP2_TRY(d.wait());
    }
  }
  fo.phase = 2;
  return LCP2_OK;
}

namespace {
// a sharded circuit answers the initial-tree and FRI-layer-0 parts of the queries whose leaf it holds and leaves zeros for
// the others (its share of the proof); the smaller FRI layers are replicated on every rank
bool holds_leaf(const lcp2_circuit *c, u64 leaf) {
  const u64 n = 1ull << c->p.degree_bits, leaf0 = (u64)c->bf * n;
  return leaf >= leaf0 && leaf < leaf0 + (u64)c->nblocks() * n;
}

// the query indices: drawn from the challenger, uploaded as [1 + layers][Qn] global leaves, [Qn] local leaves of the initial
// trees, [Qn] local leaves of FRI layer 0
int fri_query_indices(lcp2_circuit *c, const FriWork &w) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p;
  std::vector<u64> &idx = c->fo.idx, &up = c->fo.idx_up;
  const u32 Qn = p.num_query_rounds;
  const u64 n = 1ull << p.degree_bits;
  fri_draw_indices(w, c->fo.ch, idx);
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
int fri_answer_queries(lcp2_circuit *c, const FriWork &w, u64 *proof) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p; hipStream_t s = ctx->stream;
  const ProofLayout L(p);
  const std::vector<u64> &idx = c->fo.idx;
  const auto oracles = c->oracles();
  const u32 Qn = p.num_query_rounds;
  u64 *d_idx = c->q_idx.u();
  const u64 *d_idx_local = d_idx + idx.size(), *d_idx_local0 = d_idx_local + Qn;
  u64 *buf = c->q_buf.u();
  size_t pos = 0;
  size_t o_leaf[4], o_sib[4];
  for (int o = 0; o < 4; o++) {
    o_leaf[o] = pos; pos += (size_t)Qn * oracles[o]->ncols;
    o_sib[o] = pos; pos += (size_t)Qn * L.q_init_sib * 4;
  }
  FriSide side;
  pos = fri_side_layout(w, pos, side);
  if (pos * 8 > c->q_buf.bytes) return ctx->fail(LCP2_E_INVALID, "internal: query workspace too small");
  for (int o = 0; o < 4; o++) {
    const lcp2_oracle &O = *oracles[o];
    launch_gather_rows(s, O.lde.u(), O.nleaves(), O.ncols, d_idx_local, Qn, buf + o_leaf[o]);
    launch_gather_digests(s, O.digests.u(), O.d_level_off.u(), O.nlevels() - 1, d_idx_local, Qn, buf + o_sib[o]);
  }
  const u64 *d_leaf[LCP2_MAX_FRI_LAYERS];  // layer 0 by its local leaves, the replicated layers by their global ones
  for (u32 l = 0; l < p.num_fri_layers; l++) d_leaf[l] = l == 0 ? d_idx_local0 : d_idx + (1 + l) * Qn;
  fri_gather_layers(ctx, w, d_leaf, buf, side);
  LCP2_HIP(ctx, hipGetLastError());
  std::vector<u64> h(pos);
  LCP2_TRY(download(ctx, h.data(), buf, pos * 8));
  for (u32 q = 0; q < Qn; q++) {
    u64 *R = proof + L.queries + (size_t)q * L.query_words;
    for (int o = 0; o < 4 && holds_leaf(c, idx[q]); o++) {
      u32 nc = oracles[o]->ncols;
      memcpy(R + L.q_init_off[o], h.data() + o_leaf[o] + (size_t)q * nc, nc * 8);
      memcpy(R + L.q_init_off[o] + nc, h.data() + o_sib[o] + (size_t)q * L.q_init_sib * 4, L.q_init_sib * 32);
    }
  }
  fri_scatter_layers(w, h.data(), side, proof + L.queries, L.query_words, L.q_step_off, [&](u32 q) { return !holds_leaf(c, idx[q]); });
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
  lcp2_ctx *ctx = c->ctx; FriOpenState &fo = c->fo;
  const ProofLayout L(c->p);
  const FriWork w = fri_work_of(c);
  // K8: the commit phase (layer 0 is committed already) down to the final polynomial; K9: proof of work, minimum witness
  LCP2_TRY(fri_commit_phase(ctx, w, fo.ch, true, proof + L.fri_caps, fo.fri_betas, proof + L.final_poly));
  LCP2_TRY(fri_proof_of_work(ctx, w, fo.ch, proof + L.pow_witness));
  fo.pow_witness = proof[L.pow_witness];
  LCP2_TRY(fri_query_indices(c, w));
  return fri_answer_queries(c, w, proof);
}
