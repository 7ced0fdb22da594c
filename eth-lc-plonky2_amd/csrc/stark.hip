// AIR proofs over the openings of bare oracles: lcp2_stark_proof_words, lcp2_stark_prove and lcp2_stark_verify and their _perm
// forms (include/lcp2.h).  The kernels below run the per-point text of stark.hpp - k_stark_check over the rows of the trace as given,
// k_stark_quotient over the quotient coset of the trace LDE, and for a permutation argument k_stark_perm_ratio over the rows,
// k_stark_perm_close and the PERM instantiation of the quotient kernel; the running product is launch_scan, commitments go through
// commit_values_dev / commit_coeffs_dev, the transform of the quotient through the coset inverse NTT, the openings through
// lcp2_fri_prove_openings, and the transcript through the host challenger.
#include "circuit_state.hpp"
#include "stark.hpp"

using namespace lcp2;

namespace lcp2 {

// ------------------------------------------------------------------ kernels
// One lane per point, the registers of the interpreter in LDS (register r of lane t at lds[r * ST_THREADS + t]: conflict free),
// decode wave-uniform from the constant address space.  128 lanes: 64 registers fit the 64 KiB of dynamic LDS a launch may ask for.
constexpr u32 ST_THREADS = 128;
struct StLdsRegs {
  u64 *base;
  __device__ __forceinline__ u64 &operator[](u32 r) const { return base[r * ST_THREADS]; }
};
struct StarkQuotientArgs {
  StPrograms P;
  StCoset C;
  const u64 *lde;   // the trace LDE [width][N], leaf order
  u64 N, M;         // leaves of the LDE; points of the quotient coset (its first M leaves)
  u32 lgN, rate_bits;
  u64 alphas[ST_MAX_CH];
  u64 *out;         // [num_challenges][M]
  StPerm Pm;        // PERM only: the staged permutation and the LDE of the Z columns [numZ][N], leaf order
  const u64 *z_lde;
};
template <bool PERM>
__global__ __launch_bounds__(ST_THREADS) void k_stark_quotient(StarkQuotientArgs a) {
  extern __shared__ u64 st_lds[];
  const u64 i = (u64)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= a.M) return;
  st_quotient_point<PERM>(a.P, a.C, a.lde, a.N, a.lgN, a.rate_bits, a.alphas, i, StLdsRegs{st_lds + threadIdx.x}, a.out, &a.Pm, a.z_lde);
}
// the same constraint text over the n rows of the trace as given; *flag <- the smallest violation key (row_flag.hpp)
__global__ __launch_bounds__(ST_THREADS) void k_stark_check(StPrograms P, const u64 *__restrict__ trace, u64 n, unsigned long long *flag) {
  extern __shared__ u64 st_lds[];
  const u64 row = (u64)blockIdx.x * ST_THREADS + threadIdx.x;
  if (row >= n) return;
  const u64 key = st_check_row(P, trace, n, row, StLdsRegs{st_lds + threadIdx.x});
  if (key != ROW_NO_PROBLEM) atomicMin(flag, key);
}
// The per-row ratios of Z number blockIdx.y: a lane takes ST_PERM_ROWS rows ST_THREADS apart (adjacent lanes on adjacent rows: every
// column read is a coalesced run) and shares one inversion among them; ratio [numZ][n]
__global__ __launch_bounds__(ST_THREADS) void k_stark_perm_ratio(StPerm Pm, const u64 *__restrict__ trace, u64 n, u64 *__restrict__ ratio) {
  const u64 row0 = (u64)blockIdx.x * (ST_THREADS * ST_PERM_ROWS) + threadIdx.x;
  if (row0 >= n || blockIdx.y >= Pm.numZ) return;
  st_perm_ratio_rows(Pm, trace, n, row0, ST_THREADS, blockIdx.y, ratio);
}
// *flag <- the smallest z whose running product does not close; one lane per Z (numZ <= 64)
__global__ __launch_bounds__(64) void k_stark_perm_close(const u64 *__restrict__ zs, const u64 *__restrict__ ratio, u64 n, u32 numZ, unsigned long long *flag) {
  if (threadIdx.x < numZ && !st_perm_closes(zs, ratio, n, threadIdx.x)) atomicMin(flag, (unsigned long long)threadIdx.x);
}

namespace {
struct SyncOnExit {  // host vectors that asynchronous copies read must outlive those copies on every way out
  hipStream_t s;
  ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};
struct Carve {  // a bump allocator over one scratch slot, in words
  u64 *base = nullptr;
  size_t words = 0;
  size_t take(size_t w) { const size_t at = words; words += (w + 1) & ~(size_t)1; return at; }
};
}  // namespace
}  // namespace lcp2

extern "C" size_t lcp2_stark_perm_proof_words(const lcp2_stark_desc *d, const lcp2_stark_perm *perm) {
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  std::string why;
  if (st_desc_problem(d, point_polys, why, perm, &numZ)) return 0;
  return (size_t)st_make_layout(*d, point_polys, numZ).total;
}
extern "C" size_t lcp2_stark_proof_words(const lcp2_stark_desc *d) { return lcp2_stark_perm_proof_words(d, nullptr); }

extern "C" int lcp2_stark_verify_perm(const lcp2_stark_desc *d, const lcp2_stark_perm *perm, const uint64_t *public_inputs, lcp2_challenger *ch,
                                      const uint64_t *proof, size_t proof_words, int32_t *failed_check) {
  std::string why;
  return st_verify(d, (const u64 *)public_inputs, ch, (const u64 *)proof, proof_words, failed_check, why, perm);
}
extern "C" int lcp2_stark_verify(const lcp2_stark_desc *d, const uint64_t *public_inputs, lcp2_challenger *ch, const uint64_t *proof,
                                 size_t proof_words, int32_t *failed_check) {
  return lcp2_stark_verify_perm(d, nullptr, public_inputs, ch, proof, proof_words, failed_check);
}

// lcp2_stark_prove is this call without a permutation: numZ = 0 and every step of the argument is left out
extern "C" int lcp2_stark_prove_perm(lcp2_ctx *ctx, const lcp2_stark_desc *d, const lcp2_stark_perm *perm, const uint64_t *trace, lcp2_mem trace_mem,
                                     const uint64_t *public_inputs, lcp2_challenger *chs, uint64_t *proof_, size_t proof_words,
                                     lcp2_stark_violation *violation) {
  if (!ctx) return LCP2_E_INVALID;
  if (!d || !trace || !chs || !proof_ || (d->num_public_inputs && !public_inputs)) return ctx->fail(LCP2_E_INVALID, "lcp2_stark_prove: null argument");
  if (trace_mem != LCP2_MEM_HOST && trace_mem != LCP2_MEM_DEVICE) return ctx->fail(LCP2_E_INVALID, "lcp2_stark_prove: trace_mem above 1");
  u32 point_polys[FO_MAX_POINTS] = {0}, numZ = 0;
  std::string why;
  if (st_desc_problem(d, point_polys, why, perm, &numZ)) return ctx->fail(LCP2_E_INVALID, "lcp2_stark_prove: " + why);
  if (chs->input_len >= 8 || chs->output_len > 8) return ctx->fail(LCP2_E_INVALID, "lcp2_stark_prove: broken challenger state");
  const StLayout L = st_make_layout(*d, point_polys, numZ);
  if (proof_words != L.total) return ctx->fail(LCP2_E_INVALID, "lcp2_stark_prove: proof_words is not lcp2_stark_proof_words");
  LCP2_TRY(select_device(ctx));
  hipStream_t s = ctx->stream;
  u64 *proof = (u64 *)proof_;
  const u32 width = d->width, CH = d->num_challenges, q = d->quotient_degree_bits, lgM = d->log_n + q;
  const u64 n = 1ull << d->log_n, N = n << d->fri.rate_bits, M = n << q;

  // ---- what the kernels read, staged on the host: programs, immediates, public inputs, the coset's tables
  const StStaged S = st_stage(*d, (const u64 *)public_inputs);
  StCoset C = st_make_coset(d->log_n, q);
  std::vector<u64> x_tab((1ull << C.lo_bits) + (1ull << (lgM - C.lo_bits)));
  for (u64 j = 0; j < (1ull << C.lo_bits); j++) x_tab[j] = st_coset_lo(lgM, j);
  for (u64 j = 0; j < (1ull << (lgM - C.lo_bits)); j++) x_tab[(1ull << C.lo_bits) + j] = st_coset_hi(lgM, j);
  std::vector<u64> perm_tab;  // staged once the betas and gammas are drawn
  SyncOnExit outlive{s};

  // ---- the work area: slot 3 the tables, the flag and a host trace; slot 0 the quotient (the opening layer takes slots 0 to 2 later)
  Carve T, A;
  const size_t t_code = T.take(S.code.size()), t_imm = T.take(S.imm.size()), t_pis = T.take(S.pis.size()), t_x = T.take(x_tab.size()), t_flag = T.take(1);
  const size_t t_trace = T.take(trace_mem == LCP2_MEM_HOST ? (size_t)width * n : 0);
  const size_t perm_words = numZ ? 3 * (size_t)perm->num_pairs * CH + perm->num_column_pairs + 1 : 0;
  const size_t t_perm = T.take(perm_words), t_ratio = T.take((size_t)numZ * n), t_zs = T.take((size_t)numZ * n), t_scan = T.take(numZ ? scan_scratch_words(n, numZ) : 0);
  const size_t a_quot = A.take((size_t)CH * M);
  LCP2_TRY(scratch_ensure(ctx, 3, T.words * 8, (void **)&T.base));
  LCP2_TRY(scratch_ensure(ctx, 0, A.words * 8, (void **)&A.base));
  LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_code, S.code.data(), S.code.size() * 8, hipMemcpyHostToDevice, s));
  LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_imm, S.imm.data(), S.imm.size() * 8, hipMemcpyHostToDevice, s));
  LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_pis, S.pis.data(), S.pis.size() * 8, hipMemcpyHostToDevice, s));
  LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_x, x_tab.data(), x_tab.size() * 8, hipMemcpyHostToDevice, s));
  const u64 *d_trace = (const u64 *)trace;
  if (trace_mem == LCP2_MEM_HOST) {
    LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_trace, trace, (size_t)width * n * 8, hipMemcpyHostToDevice, s));
    d_trace = T.base + t_trace;
  }
  StPrograms P = S.view(*d);
  P.code = T.base + t_code; P.imm = T.base + t_imm; P.pis = T.base + t_pis;
  C.x_lo = T.base + t_x; C.x_hi = T.base + t_x + (1ull << C.lo_bits);
  const size_t lds_bytes = (size_t)std::max(d->num_regs, 1u) * ST_THREADS * sizeof(u64);

  // ---- the witness check, before anything is committed
  {
    SmallWords w{};
    w.v[0] = ROW_NO_PROBLEM;
    launch_set_words(s, T.base + t_flag, w, 1);
    ProfScope ps(ctx, LCP2_K_QUOTIENT, 8.0 * n * width);
    hipLaunchKernelGGL(k_stark_check, dim3((unsigned)((n + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), lds_bytes, s, P, d_trace, n,
                       (unsigned long long *)(T.base + t_flag));
  }
  LCP2_HIP(ctx, hipGetLastError());
  u64 key = ROW_NO_PROBLEM;
  LCP2_TRY(download(ctx, &key, T.base + t_flag, 8));
  if (key != ROW_NO_PROBLEM) {
    const lcp2_stark_violation v = st_violation_of(S.view(*d), key);
    if (violation) *violation = v;
    static const char *const names[3] = {"first_row", "transition", "last_row"};
    return ctx->fail(LCP2_E_UNSAT, std::string("lcp2_stark_prove: ") + names[v.kind] + " constraint " + std::to_string(v.constraint) + " is violated on row " + std::to_string(v.row));
  }

  // ---- trace commitment, alphas
  HostChallenger ch;
  ch.load((const u64 *)chs->sponge, (const u64 *)chs->input, chs->input_len, (const u64 *)chs->output, chs->output_len);
  lcp2_oracle trace_oracle, z_oracle, quot_oracle;
  LCP2_TRY(commit_values_dev(ctx, d_trace, width, d->log_n, d->fri.rate_bits, d->fri.cap_height, &trace_oracle));
  LCP2_TRY(download(ctx, proof + L.trace_cap, trace_oracle.cap_dev(), (size_t)L.capw * 8));
  StarkQuotientArgs qa{};
  st_observe_statement(ch, S, d->num_public_inputs, proof + L.trace_cap, L.capw);

  // ---- the permutation argument: betas and gammas, the ratios of every row, their running products Z, the closing check, the commitment
  if (numZ) {
    perm_tab = st_perm_stage(*d, *perm, st_draw_perm(ch, st_perm_draws(*d, *perm)).data(), &qa.Pm);
    LCP2_HIP(ctx, hipMemcpyAsync(T.base + t_perm, perm_tab.data(), perm_tab.size() * 8, hipMemcpyHostToDevice, s));
    qa.Pm.tab = T.base + t_perm;
    u64 *ratio = T.base + t_ratio, *zs = T.base + t_zs;
    SmallWords w{};
    w.v[0] = ROW_NO_PROBLEM;
    launch_set_words(s, T.base + t_flag, w, 1);
    {
      ProfScope ps(ctx, LCP2_K_QUOTIENT, 8.0 * n * (2.0 * perm->num_column_pairs * CH + numZ));
      hipLaunchKernelGGL(k_stark_perm_ratio, dim3((unsigned)((n + ST_THREADS * ST_PERM_ROWS - 1) / (ST_THREADS * ST_PERM_ROWS)), numZ), dim3(ST_THREADS), 0, s,
                         qa.Pm, d_trace, n, ratio);
    }
    {
      ProfScope ps(ctx, LCP2_K_PERM_Z, 16.0 * n * numZ);
      launch_scan(s, true, ratio, zs, T.base + t_scan, n, false, numZ, n);
    }
    {
      ProfScope ps(ctx, LCP2_K_QUOTIENT, 16.0 * numZ);
      hipLaunchKernelGGL(k_stark_perm_close, dim3(1), dim3(64), 0, s, zs, ratio, n, numZ, (unsigned long long *)(T.base + t_flag));
    }
    LCP2_HIP(ctx, hipGetLastError());
    u64 open_z = ROW_NO_PROBLEM;
    LCP2_TRY(download(ctx, &open_z, T.base + t_flag, 8));
    if (open_z != ROW_NO_PROBLEM) {
      if (violation) *violation = lcp2_stark_violation{ST_PERM, (u32)open_z, n - 1};
      return ctx->fail(LCP2_E_UNSAT, "lcp2_stark_prove: permutation constraint " + std::to_string(open_z) + " is violated on row " + std::to_string(n - 1) +
                                         ": the running product of Z " + std::to_string(open_z) + " does not close");
    }
    LCP2_TRY(commit_values_dev(ctx, zs, numZ, d->log_n, d->fri.rate_bits, d->fri.cap_height, &z_oracle));
    LCP2_TRY(download(ctx, proof + L.z_cap, z_oracle.cap_dev(), (size_t)L.capw * 8));
    qa.z_lde = z_oracle.lde.u();
  }
  st_draw_alphas(ch, numZ ? proof + L.z_cap : nullptr, L.capw, CH, qa.alphas);

  // ---- the quotient on the first M leaves, to coefficients, committed as CH * Q columns of n
  qa.P = P; qa.C = C; qa.lde = trace_oracle.lde.u(); qa.N = N; qa.M = M; qa.lgN = d->log_n + d->fri.rate_bits; qa.rate_bits = d->fri.rate_bits;
  qa.out = A.base + a_quot;
  {
    ProfScope ps(ctx, LCP2_K_QUOTIENT, 8.0 * M * (2.0 * width + 2.0 * numZ + CH));
    const dim3 grid((unsigned)((M + ST_THREADS - 1) / ST_THREADS));
    if (numZ) hipLaunchKernelGGL(k_stark_quotient<true>, grid, dim3(ST_THREADS), lds_bytes, s, qa);
    else hipLaunchKernelGGL(k_stark_quotient<false>, grid, dim3(ST_THREADS), lds_bytes, s, qa);
  }
  LCP2_HIP(ctx, hipGetLastError());
  DeviceNttBackend be{ctx};
  NttHost<DeviceNttBackend> ntt(be);
  {
    ProfScope ps(ctx, LCP2_K_INTT, 16.0 * M * CH);
    ntt.inverse_bitrev_in(qa.out, M, qa.out, M, lgM, CH, GL_GENERATOR);
  }
  if (be.status) return be.status;
  LCP2_HIP(ctx, hipGetLastError());
  LCP2_TRY(commit_coeffs_dev(ctx, qa.out, L.quot_cols, d->log_n, d->fri.rate_bits, d->fri.cap_height, &quot_oracle, true));
  LCP2_TRY(download(ctx, proof + L.quot_cap, quot_oracle.cap_dev(), (size_t)L.capw * 8));
  const gl2 zeta = st_draw_zeta(ch, proof + L.quot_cap, L.capw);

  // ---- the openings at zeta and g zeta
  u64 points[4];
  st_points(zeta, d->log_n, points);
  ch.save((u64 *)chs->sponge, (u64 *)chs->input, chs->input_len, (u64 *)chs->output, chs->output_len);
  const StInstance I(*d, numZ);
  lcp2_oracle *oracles[3] = {&trace_oracle, numZ ? &z_oracle : &quot_oracle, &quot_oracle};
  const int rc = lcp2_fri_prove_openings(ctx, oracles, &I.inst, (const uint64_t *)points, &d->fri, chs, (uint64_t *)(proof + L.openings), (size_t)L.fo.total);
  (void)hipStreamSynchronize(s);  // the oracles are released on return
  return rc;
}

extern "C" int lcp2_stark_prove(lcp2_ctx *ctx, const lcp2_stark_desc *d, const uint64_t *trace, lcp2_mem trace_mem, const uint64_t *public_inputs,
                                lcp2_challenger *chs, uint64_t *proof, size_t proof_words, lcp2_stark_violation *violation) {
  return lcp2_stark_prove_perm(ctx, d, nullptr, trace, trace_mem, public_inputs, chs, proof, proof_words, violation);
}
