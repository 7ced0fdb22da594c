// The stages before the opening: wires, permutation argument, quotient.  Each is a function of its inputs and
// of the commitments made by the stages before it (held by the circuit handle).
#include "circuit_state.hpp"

using namespace lcp2;

namespace {
// A proof in the row exchange form begins: nothing the handle holds of the previous proof counts any more, `wire_rows` (device,
// [num_wires][rows()]) are scanned for values >= p into the cleared flag, and the constants of this rank's rows are in cs_rows
int enter_rows_mode(lcp2_circuit *c, const u64 *wire_rows) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p; hipStream_t s = ctx->stream;
  c->rows_mode = true; c->perm_phase = 0; c->fo.phase = 0; c->stage = lcp2_circuit::ST_NONE;
  launch_set_words(s, c->small.u() + SMALL_NONCANON, SmallWords{}, 1);
  launch_canon_copy(s, wire_rows, nullptr, (u64)p.num_wires * c->rows(), (unsigned long long *)(c->small.u() + SMALL_NONCANON));
  if (!c->cs_rows_ready) {  // the gate check reads the constants with the stride of the wires
    const u64 R = c->rows();
    LCP2_HIP(ctx, c->cs_rows.ensure((size_t)p.num_constants * R * 8));
    launch_copy_2d(s, c->cs_rows.u(), R, c->cs_values.u() + c->row0(), 1ull << p.degree_bits, R, p.num_constants);
    c->cs_rows_ready = true;
  }
  return LCP2_OK;
}
}  // namespace

namespace lcp2 {
// PolynomialBatch::from_values on the witness (K1-K4).  d_coeffs (nullable, device): the coefficients of every wire column,
// already computed (a sharded proof runs the iNTT polynomial-parallel across the ranks and all-gathers the result).
// rows_only: `wires_in` is this rank's row block of the values, [num_wires][n / world] (device), see lcp2_commit_wires_rows.
int stage_wires(lcp2_circuit *c, const u64 *wires_in, lcp2_mem wires_mem, const u64 *d_coeffs, u64 *cap_out, bool rows_only) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; hipStream_t s = e.s;
  const u64 n = e.n; const u32 W = e.W;
  // The caller's buffer may hold non-canonical values (any u64): the transforms and K5 canonicalise what they load, the witness
  // check of the quotient stage does not.  The bit-reversal of the iNTT, which reads every value anyway, reports whether one is
  // >= p (no extra traffic); stage_perm_zs then takes a canonical copy before anything reads the values again.
  unsigned long long *d_flag = (unsigned long long *)(c->small.u() + SMALL_NONCANON);
  const u64 *d_wires = wires_in;
  if (rows_only) {
    if (!c->sharded() || !d_coeffs || wires_mem != LCP2_MEM_DEVICE || n < c->world())
      return ctx->fail(LCP2_E_INVALID, "lcp2_commit_wires_rows: needs a sharded circuit with at least one row per rank, device buffers");
    LCP2_TRY(enter_rows_mode(c, wires_in));
    LCP2_TRY(commit_coeffs_dev(ctx, d_coeffs, W, p.degree_bits, p.rate_bits, p.cap_height, &c->wires, true));
  } else {
    c->rows_mode = false; c->perm_phase = 0; c->fo.phase = 0;  // a new proof: an opening stage left half-way belongs to the previous one
    if (wires_mem == LCP2_MEM_HOST) {
      LCP2_HIP(ctx, c->wires_vals.ensure((size_t)W * n * 8));
      LCP2_HIP(ctx, hipMemcpyAsync(c->wires_vals.p, wires_in, (size_t)W * n * 8, hipMemcpyHostToDevice, s));
      d_wires = c->wires_vals.u();
    }
    c->stage = lcp2_circuit::ST_NONE;
    launch_set_words(s, c->small.u() + SMALL_NONCANON, SmallWords{}, 1);
    if (d_coeffs) {
      LCP2_TRY(commit_coeffs_dev(ctx, d_coeffs, W, p.degree_bits, p.rate_bits, p.cap_height, &c->wires, true));
      launch_canon_copy(s, d_wires, nullptr, (u64)W * c->rows(), d_flag);  // the values did not pass through an iNTT here: scan them
    } else {
      LCP2_TRY(commit_values_dev(ctx, d_wires, W, p.degree_bits, p.rate_bits, p.cap_height, &c->wires, d_flag));
    }
  }
  {  // the cap and the non-canonical flag with one synchronisation
    Download d(ctx);
    LCP2_TRY(queue_cap(d, c, c->wires.cap_dev(), cap_out));
    LCP2_TRY(d.add(&c->noncanon_host, d_flag, 8));
    LCP2_TRY(d.wait());
  }
  c->d_wires_cur = d_wires;
  c->stage = lcp2_circuit::ST_WIRES;
  return LCP2_OK;
}

// wires_permutation_partial_products_and_zs + commitment (K5, K1-K4), in three steps so that a sharded proof in the row
// exchange form can run K5 on its own rows: perm_begin (chunk products and their running product inside the block),
// perm_finish (Z and the partial products, times the product of the blocks before this one), perm_commit.
namespace {
PermArgs perm_args(lcp2_circuit *c, NttHost<DeviceNttBackend> &ntt, u64 *zs_out) {
  const lcp2_params &p = c->p;
  const u64 n = 1ull << p.degree_bits, R = c->rows();
  u64 *d_small = c->small.u();
  PermArgs a{};
  a.wires = c->d_wires_cur; a.wires_stride = R;
  a.sigmas = c->cs_values.u() + (u64)p.num_constants * n + c->row0(); a.sigma_stride = n;
  a.k_is = c->d_kis.u();
  a.subgroup = ntt.root_table(p.degree_bits, false);
  a.betas = d_small + SMALL_BETAS; a.gammas = d_small + SMALL_GAMMAS; a.prefix = nullptr;
  a.chunk_q = c->chunk_q.u(); a.row_tot = c->row_tot.u(); a.zs_out = zs_out;
  a.n = R; a.row0 = c->row0();
  a.num_routed = p.num_routed_wires; a.chunk = p.quotient_degree_factor; a.nchunks = npp_of(p) + 1; a.num_challenges = p.num_challenges;
  return a;
}
// where K5 writes: the value buffer of the commitment, or this rank's slot of the exchange buffer
u64 *perm_out(lcp2_circuit *c) {
  const u64 ncz = (u64)c->p.num_challenges * (1 + npp_of(c->p));
  return c->rows_mode ? c->zs_rows.u() + (u64)c->rank() * ncz * c->rows() : c->zs_vals.u();
}
}  // namespace

int perm_begin(lcp2_circuit *c, const u64 *betas, const u64 *gammas) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; hipStream_t s = e.s;
  const u32 W = e.W, NR = e.NR, CH = e.CH, npp = e.npp;
  if (c->stage < lcp2_circuit::ST_WIRES) return ctx->fail(LCP2_E_INVALID, "lcp2_perm_zs: the wires are not committed");
  const u64 R = c->rows();
  u64 *d_small = c->small.u();
  {  // the challenges travel in the kernel arguments (betas at SMALL_BETAS, gammas right behind them)
    static_assert(SMALL_GAMMAS == SMALL_BETAS + 4 && QUOTIENT_MAX_CH <= 4, "betas and gammas are set with one launch");
    SmallWords w{};
    for (u32 k = 0; k < CH; k++) { w.v[k] = gl_canon(betas[k]); w.v[4 + k] = gl_canon(gammas[k]); }
    launch_set_words(s, d_small + SMALL_BETAS, w, 8);
  }
  if (c->noncanon_host) {  // rare: a witness with values in [p, 2^64): continue from a canonical copy (stage_wires)
    LCP2_HIP(ctx, c->wires_vals.ensure((size_t)W * R * 8));
    launch_canon_copy(s, c->d_wires_cur, c->wires_vals.u(), (u64)W * R, nullptr);  // (a host witness is already the library's copy: in place)
    c->d_wires_cur = c->wires_vals.u();
  }
  if (c->rows_mode) LCP2_HIP(ctx, c->zs_rows.ensure((size_t)CH * (1 + npp) * e.n * 8));
  // ---- K5: the quotient chunks of every row and Z inside the block (exclusive prefix product of the row totals)
  u64 *zs_out = perm_out(c);
  PermArgs a = perm_args(c, e.ntt, zs_out);
  if (e.be.status) return e.be.status;
  {
    ProfScope ps(ctx, LCP2_K_PERM_Z, (double)R * 8.0 * (2.0 * NR + CH * (1.0 + npp)));
    launch_perm_chunks(s, a);
    launch_scan(s, true, c->row_tot.u(), zs_out, c->scan_tmp.u(), R, false, CH, R);
  }
  LCP2_HIP(ctx, hipGetLastError());
  return LCP2_OK;
}
// Z before the block's last row and that row's quotient, per challenge, into c->perm_wrap: queued behind whatever the caller
// downloads next (perm_finalize rescales zs_out in place only when a prefix is given, and then the caller has read these first)
int queue_perm_wrap(Download &d, lcp2_circuit *c) {
  const u64 R = c->rows();
  const u64 *zs_out = perm_out(c);
  for (u32 k = 0; k < c->p.num_challenges; k++) {
    LCP2_TRY(d.add(&c->perm_wrap[2 * k], zs_out + (u64)k * R + (R - 1), 8));
    LCP2_TRY(d.add(&c->perm_wrap[2 * k + 1], c->row_tot.u() + (u64)k * R + (R - 1), 8));
  }
  return LCP2_OK;
}

// prefix (nullable, host, [CH]): the product of the row blocks before this one
int perm_finish(lcp2_circuit *c, const u64 *prefix) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; hipStream_t s = e.s; const u32 CH = e.CH, npp = e.npp;
  PermArgs a = perm_args(c, e.ntt, perm_out(c));
  if (e.be.status) return e.be.status;
  if (prefix) {
    SmallWords w{};
    for (u32 k = 0; k < CH; k++) w.v[k] = prefix[k];
    launch_set_words(s, c->small.u() + SMALL_PERM_PREFIX, w, CH);
    a.prefix = c->small.u() + SMALL_PERM_PREFIX;
  }
  ProfScope ps(ctx, LCP2_K_PERM_Z, (double)c->rows() * 8.0 * CH * (1.0 + 2.0 * npp));
  launch_perm_finalize(s, a);
  LCP2_HIP(ctx, hipGetLastError());
  return LCP2_OK;
}

int perm_commit(lcp2_circuit *c, u64 *cap_out, bool with_wrap) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; const u32 ncz = e.CH * (1 + e.npp);
  if (c->rows_mode) {  // the exchange buffer holds every rank's rows, [rank][column][rows]: back to whole columns
    const u64 R = c->rows();
    for (u32 r = 0; r < c->world(); r++)
      launch_copy_2d(e.s, c->zs_vals.u() + (u64)r * R, e.n, c->zs_rows.u() + (u64)r * ncz * R, R, R, ncz);
  }
  LCP2_TRY(commit_values_dev(ctx, c->zs_vals.u(), ncz, p.degree_bits, p.rate_bits, p.cap_height, &c->zs));
  Download d(ctx);
  LCP2_TRY(queue_cap(d, c, c->zs.cap_dev(), cap_out));
  if (with_wrap) LCP2_TRY(queue_perm_wrap(d, c));  // (the commitment reads zs_vals, it does not change it)
  LCP2_TRY(d.wait());
  c->stage = lcp2_circuit::ST_ZS;
  return LCP2_OK;
}

int stage_perm_zs(lcp2_circuit *c, const u64 *betas, const u64 *gammas, u64 *cap_out) {
  if (c->rows_mode) return c->ctx->fail(LCP2_E_INVALID, "row exchange form: lcp2_perm_zs_rows_begin / _finish / lcp2_perm_zs_commit");
  LCP2_TRY(perm_begin(c, betas, gammas));
  LCP2_TRY(perm_finish(c, nullptr));
  LCP2_TRY(perm_commit(c, cap_out, true));  // one synchronisation: the cap and perm_wrap
  // Copy constraints: Z must come back to 1 after the last row, Z(g^(n-1)) * (row n-1's quotient) = 1, which holds for
  // every beta, gamma exactly when the wire values are constant on the cycles of sigma (up to the soundness error of the
  // argument itself).  plonky2 reports a broken copy constraint as an Err of prove(); so does this (LCP2_E_UNSAT).
  for (u32 k = 0; k < c->p.num_challenges; k++)
    if (gl_mul(c->perm_wrap[2 * k], c->perm_wrap[2 * k + 1]) != 1) {
      c->stage = lcp2_circuit::ST_WIRES;
      return c->ctx->fail(LCP2_E_UNSAT, "the witness violates a copy constraint (the permutation product does not return to 1)");
    }
  return LCP2_OK;
}

// Half tier of K6: every plane [bundles * CH][NQ] holds its values on the first NQ / 2 leaves; fill the second half.  The
// coefficients in between go through the quotient oracle's coefficient buffer (CH * NQ words = 2 CH half planes per batch): it
// is not written before stage_quotient_commit and nothing reads the previous proof's once a new proof has reached K6.
int tier_extend(lcp2_circuit *c, NttHost<DeviceNttBackend> &ntt) {
  lcp2_ctx *ctx = c->ctx; const lcp2_params &p = c->p;
  const u32 CH = p.num_challenges, lgNQ = p.degree_bits + c->qbits(), ncols = (u32)c->tiers.bundles.size() * CH, batch = 2 * CH;
  const u64 NQ = 1ull << lgNQ;
  LCP2_HIP(ctx, c->quot.coeffs.ensure((size_t)CH * NQ * 8));
  const u64 second = gl_mul(GL_GENERATOR, gl_root_of_unity(lgNQ));  // the odd points of 7 H_NQ are the coset 7 w_NQ H_{NQ/2}
  for (u32 first = 0; first < ncols; first += batch) {
    const u32 k = std::min(batch, ncols - first);
    u64 *pl = c->tier_planes.u() + (u64)first * NQ;
    ntt.inverse_bitrev_in(pl, NQ, c->quot.coeffs.u(), NQ / 2, lgNQ - 1, k, GL_GENERATOR);
    ntt.forward(c->quot.coeffs.u(), NQ / 2, pl + NQ / 2, NQ, lgNQ - 1, k, second, 0);
  }
  return LCP2_OK;
}

// compute_quotient_polys + commitment (K6, K1-K4)
// defer_check: leave the gate-check verdict on the device; stage_quotient_commit reads it together with the quotient cap
int stage_quotient_values(lcp2_circuit *c, const u64 *alphas, const u64 *pi_hash, bool defer_check) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; hipStream_t s = e.s; NttHost<DeviceNttBackend> &ntt = e.ntt;
  const u64 n = e.n, N = e.N;
  const u32 lgN = e.lgN, W = e.W, NR = e.NR, NC = e.NC, CH = e.CH, Q = e.Q, npp = e.npp, nchunks = e.nchunks, ncs = e.ncs;
  if (c->stage < lcp2_circuit::ST_ZS) return ctx->fail(LCP2_E_INVALID, "lcp2_quotient: Z / partial products are not committed");
  u64 *d_small = c->small.u();
  u64 *d_betas = d_small + SMALL_BETAS, *d_gammas = d_small + SMALL_GAMMAS, *d_alphas = d_small + SMALL_ALPHAS;
  const u32 NG = (u32)c->gates.size();
  {  // alphas, their inverses and powers, the limb table, the public-input hash, the check flag, alpha^(m_g - 1) per gate: computed
     // on the device from the challenges in the kernel arguments (k_quotient_setup)
    QuotientSetupArgs qs{};
    for (u32 k = 0; k < CH; k++) qs.alphas[k] = gl_canon(alphas[k]);
    for (u32 i = 0; i < 4; i++) qs.pi_hash[i] = gl_canon(pi_hash[i]);
    qs.num_challenges = CH; qs.num_gates = NG; qs.gates = (const GateDev *)c->d_gates.p; qs.small = d_small;
    LCP2_HIP(ctx, c->alpha_limbs.ensure((size_t)QUOTIENT_MAX_CH * QUOTIENT_TERM_POWS * 16));
    qs.limbs = (u32 *)c->alpha_limbs.p;
    launch_quotient_setup(s, qs);
  }
  // ---- K6: quotient values on the coset, coset iNTT, chunking, commitment.  The quotient lives on the 2^q n-point coset
  // 7 H_{2^q n}, q = ceil(log2 Q) <= rate_bits: a natural index j 2^(rate_bits - q) of the LDE is the leaf bitrev_{d+q}(j) < 2^q n,
  // so the first 2^q n leaves of every LDE are that coset in its own leaf order, and K6 reads them in place (column stride N)
  const u32 qb = c->qbits(), lgNQ = p.degree_bits + qb;
  const u64 NQ = n << qb;
  {
    QuotientArgs a{};
    a.wires = c->wires.lde.u(); a.consts = c->cs.lde.u(); a.zs = c->zs.lde.u(); a.l0 = c->d_l0.u(); a.zh_inv = c->d_zh_inv.u();
    u64 ls, hs;
    a.points = ntt.shift_table(gl_root_of_unity(lgNQ), lgNQ, 0, false, GL_GENERATOR, ls, hs);
    a.k_is = c->d_kis.u(); a.betas = d_betas; a.gammas = d_gammas; a.alphas = d_alphas; a.pis = d_small + SMALL_PI_HASH; a.imm = c->d_imm.u();
    a.kis_pow7 = 1;
    for (u32 j = 0; j < NR; j++) a.kis_pow7 &= c->k_is[j] == (j ? gl_mul(c->k_is[j - 1], 7) : 1);  // plonky2's coset shifts
    a.alpha_inv = d_small + SMALL_ALPHA_INV; a.gate_scale = d_small + SMALL_GATE_SCALE; a.alpha_pow = d_small + SMALL_ALPHA_POW;
    a.alpha_limbs = (const u32 *)c->alpha_limbs.p;
    a.code = (const u32 *)c->d_code.p; a.gates = (const GateDev *)c->d_gates.p; a.out = c->qvals.u();
    a.stage_list = (const u32 *)c->d_stage.p; a.num_wires = W; a.rc = ctx->d_rc;
    a.N = NQ; a.lgN = lgNQ; a.rate_bits = qb; a.num_gates = NG; a.num_selectors = c->num_selectors;
    a.num_constants = NC; a.num_routed = NR; a.chunk = Q; a.nchunks = nchunks; a.num_challenges = CH; a.num_regs = c->dev_regs;
    a.leaf0 = (u64)c->bf * n; a.count = c->sharded() ? (u64)c->nblocks() * n : NQ; a.stride = c->sharded() ? a.count : N;
    if (e.be.status) return e.be.status;
    // a sharded circuit fills its own leaf blocks and leaves zeros elsewhere: the ranks' buffers sum (or OR) to the values
    if (c->sharded()) LCP2_HIP(ctx, hipMemsetAsync(c->qvals.p, 0, (size_t)CH * NQ * 8, s));
    ProfScope ps(ctx, LCP2_K_QUOTIENT, (double)a.count * 8.0 * (W + ncs + CH * (1.0 + npp) + 2.0 + CH) + 8.0 * n * (W + NC));
    // the gate constraints on the n rows of H first (1/8 of the work below): a witness that violates one is the Err of prove()
    QuotientArgs h = a;
    h.wires = c->d_wires_cur; h.consts = c->rows_mode ? c->cs_rows.u() : c->cs_values.u(); h.leaf0 = 0; h.count = c->rows(); h.stride = c->rows();
    launch_gate_check(s, h, c->dev_gates, (unsigned long long *)(d_small + SMALL_CHECK));
    if (!c->tiers.on()) {
      launch_quotient(s, a, c->dev_gates);
    } else {
      // Half tier: the bundles' polynomials have degree < NQ / 2, so their values on the first NQ / 2 leaves (the coset 7 H_{NQ/2} in
      // its own leaf order) fix them; the second half of the prefix is the coset 7 w_NQ H_{NQ/2}, again in leaf order.
      u64 *planes = c->tier_planes.u();
      QuotientArgs hq = a;
      hq.count = NQ / 2; hq.half_mask = c->d_half_mask.u();
      launch_quotient_half_tier(s, hq, c->dev_gates, c->tiers, planes);
      LCP2_TRY(tier_extend(c, ntt));
      if (e.be.status) return e.be.status;
      const u32 launched = launch_quotient_full_tier(s, a, c->dev_gates, c->tiers);
      launch_tier_combine(s, a, c->tiers, planes, launched ? 1u : 0u);  // before k_q_perm: it divides by Z_H
      launch_quotient_perm(s, a, 1u);
    }
  }
  LCP2_HIP(ctx, hipGetLastError());
  if (c->local_quotient()) {  // block b is the coset of shift g w_N^bitrev(b), its values in bit-reversed order: interpolate in place
    ProfScope ps(ctx, LCP2_K_INTT, 16.0 * n * CH * c->nblocks());
    for (u32 b = c->bf; b < c->bf + c->nblocks(); b++) {
      const u64 shift = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(lgN), bitrev32(b, p.rate_bits)));
      ntt.inverse_bitrev_in(c->qvals.u() + (u64)b * n, N, c->qvals.u() + (u64)b * n, N, p.degree_bits, CH, shift);
    }
    if (e.be.status) return e.be.status;
  }
  c->check_pending = defer_check;
  if (!defer_check) {
    u64 bad_row = ~0ull;
    LCP2_TRY(download(ctx, &bad_row, d_small + SMALL_CHECK, 8));  // synchronises the stream
    if (bad_row != ~0ull) return ctx->fail(LCP2_E_UNSAT, "the witness violates a gate constraint on row " + std::to_string(bad_row - 1 + c->row0()));
  }
  c->stage = lcp2_circuit::ST_QVALS;
  return LCP2_OK;
}

// coset iNTT of the (complete) quotient values, chunking, commitment
int stage_quotient_commit(lcp2_circuit *c, u64 *cap_out) {
  StageEnv e(c);
  LCP2_TRY(e.status);
  lcp2_ctx *ctx = e.ctx; const lcp2_params &p = e.p; hipStream_t s = e.s; NttHost<DeviceNttBackend> &ntt = e.ntt;
  const u64 n = e.n, N = e.N; const u32 CH = e.CH, Q = e.Q;
  if (c->stage != lcp2_circuit::ST_QVALS) return ctx->fail(LCP2_E_INVALID, "lcp2_quotient_commit: no quotient values");
  const u32 qb = c->qbits();
  const u64 NQ = n << qb;
  const bool trim = Q != (1u << qb);  // Q chunks of the 2^q chunks: the coefficients from Q n to 2^q n must vanish
  LCP2_HIP(ctx, c->quot.coeffs.ensure((size_t)CH * NQ * 8));
  if (c->local_quotient()) {
    const u32 R = 1u << p.rate_bits;
    if (!c->q_combine.p) {
      // interpolant_b = sum_k (s_b^n)^k Q_k with s_b^n = g^n w_R^bitrev(b)  =>  Q_k = g^(-n k) / R * sum_b w_R^(-bitrev(b) k) interpolant_b
      std::vector<u64> m((size_t)R * R);
      const u64 gninv = gl_inv(gl_pow(GL_GENERATOR, n)), wrinv = gl_inv(gl_root_of_unity(p.rate_bits)), rinv = gl_inv(R);
      for (u32 k = 0; k < R; k++)
        for (u32 b = 0; b < R; b++)
          m[(size_t)k * R + b] = gl_mul(gl_mul(gl_pow(gninv, k), rinv), gl_pow(wrinv, (u64)bitrev32(b, p.rate_bits) * k));
      LCP2_TRY(upload(ctx, c->q_combine, m.data(), m.size() * 8));
      LCP2_HIP(ctx, hipStreamSynchronize(s));  // `m` is a stack-lifetime staging buffer
    }
    ProfScope ps(ctx, LCP2_K_INTT, 16.0 * N * CH);
    launch_quotient_combine(s, c->qvals.u(), c->quot.coeffs.u(), c->q_combine.u(), n, R, N, CH);
    LCP2_HIP(ctx, hipGetLastError());
  } else if (!trim) {
    ProfScope ps(ctx, LCP2_K_INTT, 16.0 * NQ * CH);
    ntt.inverse_bitrev_in(c->qvals.u(), NQ, c->quot.coeffs.u(), NQ, p.degree_bits + qb, CH, GL_GENERATOR);
  } else {  // plonky2's trim_to_len(quotient_degree): the check's verdict arrives with the cap, the first Q n coefficients move up
    ProfScope ps(ctx, LCP2_K_INTT, 16.0 * NQ * CH);
    ntt.inverse_bitrev_in(c->qvals.u(), NQ, c->qvals.u(), NQ, p.degree_bits + qb, CH, GL_GENERATOR);
    launch_set_words(s, c->small.u() + SMALL_TRIM, SmallWords{}, 1);
    launch_any_nonzero(s, c->qvals.u() + (u64)Q * n, NQ, NQ - (u64)Q * n, CH, (unsigned long long *)(c->small.u() + SMALL_TRIM));
    launch_copy_2d(s, c->quot.coeffs.u(), (u64)Q * n, c->qvals.u(), NQ, (u64)Q * n, CH);
    LCP2_HIP(ctx, hipGetLastError());
  }
  if (e.be.status) return e.be.status;
  // the Q n coefficients of challenge c are exactly its Q chunks of n coefficients, contiguous
  LCP2_TRY(commit_coeffs_dev(ctx, c->quot.coeffs.u(), CH * Q, p.degree_bits, p.rate_bits, p.cap_height, &c->quot, false));
  u64 bad_row = ~0ull, high = 0;
  {
    Download d(ctx);
    LCP2_TRY(queue_cap(d, c, c->quot.cap_dev(), cap_out));
    if (c->check_pending) LCP2_TRY(d.add(&bad_row, c->small.u() + SMALL_CHECK, 8));
    if (trim) LCP2_TRY(d.add(&high, c->small.u() + SMALL_TRIM, 8));
    LCP2_TRY(d.wait());
  }
  if (c->check_pending && bad_row != ~0ull) {  // plonky2 would have produced an invalid proof here; this is the Err of prove()
    c->check_pending = false;
    c->stage = lcp2_circuit::ST_ZS;
    return ctx->fail(LCP2_E_UNSAT, "the witness violates a gate constraint on row " + std::to_string(bad_row - 1 + c->row0()));
  }
  c->check_pending = false;
  if (high) {  // plonky2 panics in trim_to_len here: a gate's filtered constraints have a degree above Q + 1
    c->stage = lcp2_circuit::ST_ZS;
    return ctx->fail(LCP2_E_INVALID, "the constraint degree exceeds quotient_degree_factor + 1 (the quotient has more than quotient_degree_factor chunks)");
  }
  c->stage = lcp2_circuit::ST_QUOT;
  return LCP2_OK;
}

int stage_quotient(lcp2_circuit *c, const u64 *alphas, const u64 *pi_hash, u64 *cap_out) {
  if (c->sharded()) return c->ctx->fail(LCP2_E_INVALID, "sharded circuit: use lcp2_quotient_values, exchange the buffer, then lcp2_quotient_commit");
  LCP2_TRY(stage_quotient_values(c, alphas, pi_hash, true));  // the verdict of the gate check arrives with the cap: one synchronisation
  return stage_quotient_commit(c, cap_out);
}
}  // namespace lcp2

// ---- the chunked form of lcp2_commit_wires_rows (include/lcp2.h)
extern "C" int lcp2_commit_wires_rows_begin(lcp2_circuit *c, const uint64_t *wire_rows) {
  LCP2_TRY(entry_guard(c, {wire_rows}));
  lcp2_ctx *ctx = c->ctx;
  const lcp2_params &p = c->p;
  const u64 n = 1ull << p.degree_bits;
  if (!c->sharded() || n < c->world() || p.num_wires <= 4)
    return ctx->fail(LCP2_E_INVALID, "lcp2_commit_wires_rows_begin: needs a sharded circuit with at least one row per rank and more than 4 wires");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  LCP2_TRY(enter_rows_mode(c, (const u64 *)wire_rows));
  lcp2_oracle *o = &c->wires;
  o->ctx = ctx; o->ncols = p.num_wires; o->log_n = p.degree_bits; o->rate_bits = p.rate_bits; o->cap_height = p.cap_height;
  LCP2_HIP(ctx, o->coeffs.ensure((size_t)p.num_wires * n * 8));
  LCP2_HIP(ctx, o->lde.ensure((size_t)p.num_wires * o->nleaves() * 8));
  LCP2_TRY(merkle_alloc_dev(ctx, o));
  LCP2_HIP(ctx, c->leaf_state.ensure((size_t)12 * o->nleaves() * 8));
  c->d_wires_cur = (const u64 *)wire_rows;
  c->chunk_next = 0;
  return LCP2_OK;
}
extern "C" int lcp2_commit_wires_chunk(lcp2_circuit *c, const uint64_t *coeffs, uint32_t first_col, uint32_t ncols) {
  LCP2_TRY(entry_guard(c, {coeffs}));
  lcp2_ctx *ctx = c->ctx;
  const lcp2_params &p = c->p;
  if (c->chunk_next < 0 || (int)first_col != c->chunk_next) return ctx->fail(LCP2_E_INVALID, "lcp2_commit_wires_chunk: chunks come in column order after lcp2_commit_wires_rows_begin");
  if (ncols == 0 || first_col % 8 || first_col + ncols > p.num_wires || (ncols % 8 && first_col + ncols != p.num_wires))
    return ctx->fail(LCP2_E_INVALID, "lcp2_commit_wires_chunk: a chunk starts at a multiple of 8 columns and is a multiple of 8 long unless it is the last");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  lcp2_oracle *o = &c->wires;
  const u64 n = 1ull << p.degree_bits, N = o->nleaves();
  hipStream_t s = ctx->stream;
  u64 *dst = o->coeffs.u() + (size_t)first_col * n;
  if ((const u64 *)coeffs != dst) LCP2_HIP(ctx, hipMemcpyAsync(dst, coeffs, (size_t)ncols * n * 8, hipMemcpyDeviceToDevice, s));
  DeviceNttBackend be{ctx};
  NttHost<DeviceNttBackend> ntt(be);
  {
    ProfScope ps(ctx, LCP2_K_LDE, (double)ncols * (8.0 * n + 8.0 * N));
    ntt.forward(dst, n, o->lde.u() + (size_t)first_col * N, N, p.degree_bits, ncols, GL_GENERATOR, p.rate_bits, o->block_first, o->block_count);
  }
  if (be.status) return be.status;
  const bool last = first_col + ncols == p.num_wires;
  {
    ProfScope ps(ctx, LCP2_K_LEAF_HASH, (double)N * (8.0 * ncols + (last ? 32.0 : 0.0)));
    launch_hash_leaves_absorb(s, o->lde.u() + (size_t)first_col * N, N, ncols, N, c->leaf_state.u(), first_col == 0, last, o->digests.u(), ctx->d_rc);
  }
  LCP2_HIP(ctx, hipGetLastError());
  c->chunk_next = (int)(first_col + ncols);
  return LCP2_OK;
}
extern "C" int lcp2_commit_wires_rows_finish(lcp2_circuit *c, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {cap}));
  lcp2_ctx *ctx = c->ctx;
  if (c->chunk_next != (int)c->p.num_wires) return ctx->fail(LCP2_E_INVALID, "lcp2_commit_wires_rows_finish: not every column has been absorbed");
  c->chunk_next = -1;
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  LCP2_TRY(merkle_levels_dev(ctx, &c->wires));
  Download d(ctx);
  LCP2_TRY(queue_cap(d, c, c->wires.cap_dev(), (u64 *)cap));
  LCP2_TRY(d.add(&c->noncanon_host, c->small.u() + SMALL_NONCANON, 8));
  LCP2_TRY(d.wait());
  c->stage = lcp2_circuit::ST_WIRES;
  return LCP2_OK;
}
