// Openings of bare oracles: lcp2_fri_config_of, lcp2_oracle_eval, lcp2_fri_openings_words, lcp2_fri_prove_openings and
// lcp2_fri_verify_openings (include/lcp2.h).  PolynomialBatch::prove_openings for any FriInstanceInfo, without a circuit handle: the
// k_open_* kernels below compose and divide the instance's batches (fri_openings.hpp holds their text) and gather the query answers
// of all oracles.  Column evaluation and the whole FRI back end - layer commitments, commit phase, proof of work, query indices, the
// FRI-layer answers - are fri_commit.hip, the text the Plonk opening (prover_open.hip) runs too, over the work area carved here.
#include "fri_commit.hpp"
#include "fri_openings.hpp"

using namespace lcp2;

namespace lcp2 {

// ------------------------------------------------------------------ kernels
struct OpenPoints { u64 z[FO_MAX_POINTS][2]; };
// the two-level power tables of every point and of its inverse, from the points in the kernel arguments
__global__ __launch_bounds__(256) void k_open_tables(OpenPoints p, u32 num_points, u32 zh, u64 hi_count, u64 *__restrict__ T) {
  const u64 t = (u64)blockIdx.x * 256 + threadIdx.x, per_point = 2 * ((1ull << zh) + hi_count);
  const u32 b = (u32)(t / per_point);
  if (b >= num_points) return;
  const gl2 v = fo_table_entry(gl2_make(p.z[b][0], p.z[b][1]), zh, hi_count, t % per_point);
  T[2 * t] = v.c0; T[2 * t + 1] = v.c1;
}
// one lane per coefficient index: every listed column is loaded once (a coalesced 512-byte run per wave and column), the weight
// row of a column is wave-uniform, and the up to FO_MAX_POINTS extension sums stay in registers
__global__ __launch_bounds__(256) void k_open_compose(FoCompose a) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n) fo_compose_coeff(a, i);
}
// per point: the inverse power, the shift; the batches added up into the two planes of the committed polynomial
__global__ __launch_bounds__(256) void k_open_divide(FoCompose a, u64 *__restrict__ out0, u64 *__restrict__ out1) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n) fo_divide_coeff(a, i, out0, out1);
}
// the initial-tree part of every query round, in proof layout: block (q, o) copies the leaf of oracle o at index[q] and its siblings
struct OpenGather {
  const u64 *lde[FO_MAX_ORACLES], *digests[FO_MAX_ORACLES], *level_off[FO_MAX_ORACLES];
  u32 ncols[FO_MAX_ORACLES], out_off[FO_MAX_ORACLES];
  u64 nleaves;
  u32 nsib, query_words, num_queries;
};
__global__ __launch_bounds__(64) void k_open_gather_leaves(OpenGather g, const u64 *__restrict__ indices, u64 *__restrict__ out) {
  const u32 q = blockIdx.x, o = blockIdx.y;
  if (q >= g.num_queries) return;
  const u64 idx = indices[q];
  if (idx >= g.nleaves) return;
  u64 *dst = out + (u64)q * g.query_words + g.out_off[o];
  const u32 nc = g.ncols[o];
  for (u32 c = threadIdx.x; c < nc; c += blockDim.x) dst[c] = g.lde[o][(u64)c * g.nleaves + idx];
  for (u32 t = threadIdx.x; t < 4 * g.nsib; t += blockDim.x) {
    const u32 l = t >> 2;
    dst[nc + t] = g.digests[o][4 * (g.level_off[o][l] + ((idx >> l) ^ 1)) + (t & 3)];
  }
}

namespace {
// Host vectors that asynchronous copies read (pageable memory) must outlive those copies on EVERY way out of a call: declared
// after the vectors, this synchronises the stream before they are destroyed, on the error returns too.
struct SyncOnExit {
  hipStream_t s;
  ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};

// a bump allocator over one scratch slot, in words
struct Carve {
  u64 *base = nullptr;
  size_t words = 0;
  size_t take(size_t w) { const size_t at = words; words += (w + 1) & ~(size_t)1; return at; }
};
}  // namespace
}  // namespace lcp2

extern "C" int lcp2_fri_config_of(uint32_t log_n, uint32_t rate_bits, uint32_t cap_height, uint32_t pow_bits, uint32_t num_query_rounds,
                                  uint32_t arity_bits, uint32_t final_poly_bits, lcp2_fri_config *out) {
  if (!out) return LCP2_E_INVALID;
  lcp2_params p;  // the schedule, bounds and refusals are lcp2_params_config's
  LCP2_TRY(lcp2_params_config(log_n, 0, rate_bits, cap_height, pow_bits, num_query_rounds, arity_bits, final_poly_bits, &p));
  memset(out, 0, sizeof *out);
  out->rate_bits = p.rate_bits; out->cap_height = p.cap_height; out->proof_of_work_bits = p.proof_of_work_bits;
  out->num_query_rounds = p.num_query_rounds; out->num_fri_layers = p.num_fri_layers;
  memcpy(out->fri_arity_bits, p.fri_arity_bits, sizeof out->fri_arity_bits);
  return LCP2_OK;
}

extern "C" size_t lcp2_fri_openings_words(const lcp2_fri_config *cfg, uint32_t log_n, const uint32_t *oracle_cols, const lcp2_fri_instance *inst) {
  u32 point_polys[FO_MAX_POINTS] = {0};
  std::string why;
  if (fo_shape_problem(cfg, log_n, oracle_cols, inst, point_polys, why)) return 0;
  return (size_t)fo_make_layout(*cfg, log_n, oracle_cols, inst->num_oracles, point_polys, inst->num_points).total;
}

extern "C" int lcp2_fri_verify_openings(const uint64_t *const *caps, const uint32_t *oracle_cols, uint32_t log_n, const lcp2_fri_instance *inst,
                                        const uint64_t *points, const lcp2_fri_config *cfg, lcp2_challenger *ch, const uint64_t *proof,
                                        size_t proof_words, int32_t *failed_check) {
  std::string why;
  return fo_verify_openings((const u64 *const *)caps, oracle_cols, log_n, inst, (const u64 *)points, cfg, ch, (const u64 *)proof, proof_words,
                            failed_check, why);
}

extern "C" int lcp2_oracle_eval(lcp2_oracle *o, const uint64_t *points, size_t k, uint64_t *out) {
  if (!o || (k && (!points || !out))) return LCP2_E_INVALID;
  lcp2_ctx *ctx = o->ctx;
  if (o->block_count) return ctx->fail(LCP2_E_UNSUPPORTED, "lcp2_oracle_eval: a coset-sharded oracle");
  if (o->ncols == 0 || o->ncols > 65535) return ctx->fail(LCP2_E_INVALID, "lcp2_oracle_eval: column count outside [1, 65535]");
  if (!k) return LCP2_OK;
  LCP2_TRY(select_device(ctx));
  const u64 n = 1ull << o->log_n;
  const size_t nchunks = n / eval_chunk_len(n), per_point = 2 * (size_t)o->ncols;
  // the points go through in groups whose results fit the work area (64 MiB of results at the most): one copy back per group
  const size_t group = std::min<size_t>(k, std::max<size_t>(1, ((size_t)8 << 20) / per_point));
  Carve w;
  const size_t tab = w.take(eval_table_words(n)), partial = w.take(per_point * nchunks), res = w.take(per_point * group);
  LCP2_TRY(scratch_ensure(ctx, 0, w.words * 8, (void **)&w.base));
  for (size_t first = 0; first < k; first += group) {
    const size_t count = std::min(group, k - first);
    for (size_t i = 0; i < count; i++) {  // tables and partial sums are reused point after point: the stream orders them
      const gl2 z = gl2_make(points[2 * (first + i)] % GL_P, points[2 * (first + i) + 1] % GL_P);
      ProfScope ps(ctx, LCP2_K_OPENINGS, 8.0 * n * o->ncols);
      eval_tables(ctx->stream, n, z, w.base + tab);
      eval_columns(ctx->stream, o->coeffs.u(), o->ncols, n, z, w.base + tab, w.base + partial, w.base + res + i * per_point);
    }
    LCP2_HIP(ctx, hipGetLastError());
    LCP2_TRY(download(ctx, out + first * per_point, w.base + res, count * per_point * 8));
  }
  return LCP2_OK;
}

extern "C" int lcp2_fri_prove_openings(lcp2_ctx *ctx, lcp2_oracle *const *oracles, const lcp2_fri_instance *inst, const uint64_t *points_,
                                       const lcp2_fri_config *cfg, lcp2_challenger *chs, uint64_t *proof_, size_t proof_words) {
  if (!ctx) return LCP2_E_INVALID;
  if (!oracles || !inst || !points_ || !cfg || !chs || !proof_) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: null argument");
  if (inst->num_oracles < 1 || inst->num_oracles > FO_MAX_ORACLES) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: num_oracles outside [1, LCP2_FRI_MAX_ORACLES]");
  u32 oracle_cols[FO_MAX_ORACLES], point_polys[FO_MAX_POINTS] = {0};
  for (u32 o = 0; o < inst->num_oracles; o++) {
    if (!oracles[o] || oracles[o]->ctx != ctx) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: oracle " + std::to_string(o) + " is null or of another context");
    if (oracles[o]->block_count) return ctx->fail(LCP2_E_UNSUPPORTED, "lcp2_fri_prove_openings: oracle " + std::to_string(o) + " is coset-sharded");
    oracle_cols[o] = oracles[o]->ncols;
  }
  const u32 log_n = oracles[0]->log_n;
  for (u32 o = 0; o < inst->num_oracles; o++)
    if (oracles[o]->log_n != log_n || oracles[o]->rate_bits != cfg->rate_bits || oracles[o]->cap_height != cfg->cap_height)
      return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: oracle " + std::to_string(o) + " does not share log_n, rate_bits and cap_height with the config");
  std::string why;
  gl2 z[FO_MAX_POINTS];
  if (fo_shape_problem(cfg, log_n, oracle_cols, inst, point_polys, why) || fo_points_problem((const u64 *)points_, inst->num_points, z, why))
    return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: " + why);
  if (chs->input_len >= 8 || chs->output_len > 8) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: broken challenger state");
  const FoLayout L = fo_make_layout(*cfg, log_n, oracle_cols, inst->num_oracles, point_polys, inst->num_points);
  if (proof_words != L.total) return ctx->fail(LCP2_E_INVALID, "lcp2_fri_prove_openings: proof_words is not lcp2_fri_openings_words");
  LCP2_TRY(select_device(ctx));
  hipStream_t s = ctx->stream;
  u64 *proof = (u64 *)proof_;
  HostChallenger ch;
  ch.load((const u64 *)chs->sponge, (const u64 *)chs->input, chs->input_len, (const u64 *)chs->output, chs->output_len);
  const u64 n = 1ull << log_n, N = n << cfg->rate_bits;
  const u32 NP = inst->num_points, NO = inst->num_oracles, Qn = cfg->num_query_rounds, layers = cfg->num_fri_layers;
  u32 total_cols = 0, max_range = 0;
  for (u32 o = 0; o < NO; o++) total_cols += oracle_cols[o];
  for (u32 b = 0; b < NP; b++)
    for (u32 r = 0; r < inst->num_ranges[b]; r++) max_range = std::max(max_range, inst->ranges[b][r].num_polys);
  const u32 zh = (log_n + 1) / 2;
  const u64 hi_count = (n >> zh) + 1;

  // ---- the work area: slot 0 planes and values, slot 1 the FRI digests and their level offsets, slot 2 the small tables
  Carve A, D, T;
  const size_t nchunks = n / eval_chunk_len(n);
  const size_t a_planes = A.take(2 * (size_t)NP * n), a_scan = A.take(scan_scratch_words(n, 2 * NP)), a_c0 = A.take(2 * n), a_c1 = A.take(2 * n);
  size_t a_vals[LCP2_MAX_FRI_LAYERS], d_dig[LCP2_MAX_FRI_LAYERS], d_off[LCP2_MAX_FRI_LAYERS];
  // what asynchronous copies read from the host: level_off, weights, mask, idx - and the guard that keeps them alive long enough
  std::vector<u64> level_off[LCP2_MAX_FRI_LAYERS], weights, idx;
  std::vector<u32> mask;
  SyncOnExit outlive{s};
  {
    u64 m = n;
    for (u32 l = 0; l < layers; l++) {
      const u64 nvals = m << cfg->rate_bits, nleaves = nvals >> cfg->fri_arity_bits[l];
      a_vals[l] = A.take(2 * nvals);
      const u32 nlev = L.step_sib[l] + 1;
      u64 tot = 0;
      for (u32 k = 0; k < nlev; k++) { level_off[l].push_back(tot); tot += nleaves >> k; }
      d_dig[l] = D.take(4 * tot);
      d_off[l] = D.take(nlev);
      m >>= cfg->fri_arity_bits[l];
    }
  }
  const size_t t_tables = T.take(NP * fo_table_words(zh, hi_count)), t_weights = T.take((size_t)total_cols * 2 * FO_MAX_POINTS), t_mask = T.take((total_cols + 1) / 2);
  const size_t t_evtab = T.take(eval_table_words(n)), t_partial = T.take(2 * (size_t)max_range * nchunks), t_open = T.take(2 * (size_t)L.total_polys);
  const size_t t_idx = T.take((size_t)Qn * (1 + layers)), t_rounds = T.take((size_t)Qn * L.query_words), t_pow = T.take(1);
  // what fri_commit.hpp works on, first by its shape (the side buffer of the layer answers follows from it), then by its pointers
  FriWork w{};
  w.log_n = log_n; w.rate_bits = cfg->rate_bits; w.cap_height = cfg->cap_height; w.num_layers = layers;
  w.final_len = L.final_len; w.pow_bits = cfg->proof_of_work_bits; w.num_queries = Qn;
  for (u32 l = 0; l < layers; l++) { w.arity_bits[l] = L.arity_bits[l]; w.layer[l].nlevels = (u32)level_off[l].size(); }
  FriSide side_at;
  const size_t t_side = fri_side_layout(w, 0, side_at), t_sidebuf = T.take(t_side);
  LCP2_TRY(scratch_ensure(ctx, 0, A.words * 8, (void **)&A.base));
  LCP2_TRY(scratch_ensure(ctx, 1, D.words * 8 + 8, (void **)&D.base));
  LCP2_TRY(scratch_ensure(ctx, 2, T.words * 8, (void **)&T.base));
  w.fri_c[0] = A.base + a_c0; w.fri_c[1] = A.base + a_c1; w.d_pow = T.base + t_pow;
  for (u32 l = 0; l < layers; l++) {
    w.layer[l] = {A.base + a_vals[l], D.base + d_dig[l], D.base + d_off[l], level_off[l].data(), w.layer[l].nlevels};
    LCP2_HIP(ctx, hipMemcpyAsync(D.base + d_off[l], level_off[l].data(), level_off[l].size() * 8, hipMemcpyHostToDevice, s));
  }

  // ---- openings: every range of every point evaluated from the coefficients, one copy back
  memset(proof, 0, L.total * 8);
  {
    ProfScope ps(ctx, LCP2_K_OPENINGS, 8.0 * n * L.total_polys);
    for (u32 b = 0, at = 0; b < NP; b++) {
      eval_tables(s, n, z[b], T.base + t_evtab);  // once per point; the stream orders the reuse of the one table area
      for (u32 r = 0; r < inst->num_ranges[b]; r++) {
        const lcp2_fri_range &g = inst->ranges[b][r];
        eval_columns(s, oracles[g.oracle]->coeffs.u() + (size_t)g.first_poly * n, g.num_polys, n, z[b], T.base + t_evtab, T.base + t_partial,
                     T.base + t_open + 2 * (size_t)at);
        at += g.num_polys;
      }
    }
  }
  LCP2_HIP(ctx, hipGetLastError());
  LCP2_TRY(download(ctx, proof, T.base + t_open, 2 * (size_t)L.total_polys * 8));
  ch.observe_n(proof, 2 * (size_t)L.total_polys);
  const gl2 alpha = ch.get_ext();

  // ---- the committed polynomial: compose, suffix sums, divide
  FoCompose a{};
  fo_make_weights(*inst, oracle_cols, alpha, weights, mask, a.shift);
  LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_weights, weights.data(), weights.size() * 8, hipMemcpyHostToDevice, s));
  LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_mask, mask.data(), mask.size() * 4, hipMemcpyHostToDevice, s));
  for (u32 o = 0; o < NO; o++) { a.coeffs[o] = oracles[o]->coeffs.u(); a.ncols[o] = oracle_cols[o]; }
  a.num_oracles = NO; a.num_points = NP; a.n = n;
  a.weights = T.base + t_weights; a.mask = (const u32 *)(T.base + t_mask); a.tables = T.base + t_tables;
  a.zh = zh; a.hi_count = hi_count; a.planes = A.base + a_planes;
  {
    OpenPoints P{};
    for (u32 b = 0; b < NP; b++) { P.z[b][0] = z[b].c0; P.z[b][1] = z[b].c1; }
    const u64 entries = (u64)NP * 2 * ((1ull << zh) + hi_count);
    u32 listed = 0;  // columns that some point lists: what the compose kernel reads
    {
      std::vector<bool> seen(total_cols, false);
      u32 base[FO_MAX_ORACLES + 1] = {0};
      for (u32 o = 0; o < NO; o++) base[o + 1] = base[o] + oracle_cols[o];
      for (u32 b = 0; b < NP; b++)
        for (u32 r = 0; r < inst->num_ranges[b]; r++)
          for (u32 j = 0; j < inst->ranges[b][r].num_polys; j++) seen[base[inst->ranges[b][r].oracle] + inst->ranges[b][r].first_poly + j] = true;
      for (bool v : seen) listed += v;
    }
    ProfScope ps(ctx, LCP2_K_OPENINGS, 8.0 * n * listed + 16.0 * n * NP * 4 + 16.0 * n);
    hipLaunchKernelGGL(k_open_tables, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, P, NP, zh, hi_count, T.base + t_tables);
    hipLaunchKernelGGL(k_open_compose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    launch_scan(s, false, a.planes, a.planes, A.base + a_scan, n, true, 2 * NP, n);
    hipLaunchKernelGGL(k_open_divide, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, w.fri_c[0], w.fri_c[0] + n);
  }
  LCP2_HIP(ctx, hipGetLastError());

  // ---- the FRI back end: commit phase, proof of work (0 bits: witness 0, nothing launched), query indices
  LCP2_TRY(fri_commit_phase(ctx, w, ch, false, proof + L.fri_caps, nullptr, proof + L.final_poly));
  LCP2_TRY(fri_proof_of_work(ctx, w, ch, proof + L.pow_witness));
  fri_draw_indices(w, ch, idx);

  // ---- query answers
  u64 *d_idx = T.base + t_idx, *d_rounds = T.base + t_rounds, *d_side = T.base + t_sidebuf;
  LCP2_HIP(ctx, hipMemcpyAsync(d_idx, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, s));
  {
    OpenGather g{};
    for (u32 o = 0; o < NO; o++) {
      g.lde[o] = oracles[o]->lde.u(); g.digests[o] = oracles[o]->digests.u(); g.level_off[o] = oracles[o]->d_level_off.u();
      g.ncols[o] = oracle_cols[o]; g.out_off[o] = L.init_off[o];
    }
    g.nleaves = N; g.nsib = L.init_sib; g.query_words = (u32)L.query_words; g.num_queries = Qn;
    ProfScope ps(ctx, LCP2_K_OPENINGS, 8.0 * Qn * (total_cols + 4.0 * L.init_sib * NO));
    hipLaunchKernelGGL(k_open_gather_leaves, dim3(Qn, NO), dim3(64), 0, s, g, d_idx, d_rounds);
  }
  {
    const u64 *d_leaf[LCP2_MAX_FRI_LAYERS];
    for (u32 l = 0; l < layers; l++) d_leaf[l] = d_idx + (size_t)(1 + l) * Qn;
    fri_gather_layers(ctx, w, d_leaf, d_side, side_at);
  }
  LCP2_HIP(ctx, hipGetLastError());
  {
    std::vector<u64> side(t_side ? t_side : 1);
    Download d(ctx);
    LCP2_TRY(d.add(proof + L.queries, d_rounds, (size_t)Qn * L.query_words * 8));
    LCP2_TRY(d.add(side.data(), d_side, t_side * 8));
    LCP2_TRY(d.wait());  // also the end of every use of idx and level_off by the stream
    fri_scatter_layers(w, side.data(), side_at, proof + L.queries, L.query_words, L.step_off, [](u32) { return false; });
  }
  ch.save((u64 *)chs->sponge, (u64 *)chs->input, chs->input_len, (u64 *)chs->output, chs->output_len);
  return LCP2_OK;
}
