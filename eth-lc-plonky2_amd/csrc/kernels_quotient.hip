// K6 for gfx950: the quotient polynomial values on the LDE coset (compute_quotient_polys + eval_vanishing_poly_base_batch of
// plonk/prover.rs, every gate's eval_unfiltered_base) - the host staging of the gate programs, the native PoseidonGate evaluator,
// the PoseidonGate / light-gate / permutation kernels, their launchers, the challenge-dependent setup and the combination of a
// coset-sharded proof.  The kernel skeleton and the interpreter are quotient_common.hpp; the native ArithmeticGate and BaseSumGate<2>
// are the one walk of light_gates.hpp (each alone, and both at once for the pair of a light list: build() holds all three forms to
// the gates' programs); the generated evaluators have kernels of their own (kernels_gates.hpp, kernels_gates_*.hip).
//
// The LDE matrices are indexed in their storage (= Merkle leaf) order, so all column reads are coalesced 512-byte runs per wave;
// the only gathers are the two Z(g x) values per point in k_q_perm.
#include <algorithm>
#include "gate_program.hpp"
#include "kernels_gates.hpp"
#include "light_gates.hpp"

namespace lcp2 {

// Host: the staged form of the programs (gate_staging.hpp has the text)
void stage_gate_programs(const std::vector<uint32_t> &code, std::vector<GateDev> &gates, u32 num_wires, u32 num_selectors,
                         std::vector<uint32_t> &out, std::vector<uint32_t> &lists) {
  stage_programs(code, gates, num_wires, num_selectors, out, lists);
}

// ---- native PoseidonGate (LCP2_GATE_NATIVE_POSEIDON): plonky2 gates/poseidon.rs::eval_unfiltered_base with the state in
// VGPRs (32-bit halves, lazily reduced, exactly the permutation of the hash kernels) instead of LDS registers and one
// interpreted instruction at a time.  Wires: input 0..12, output 12..24, swap 24, delta 25..29, S-box inputs of full rounds
// 1..3 at 29 + 12 (r - 1) + i, of the partial rounds at 65 + r, of full rounds 4..7 at 87 + 12 r + i.  The constraints come out
// first to last; acc is the Horner chain with 1 / alpha (rescaled by the caller), as for every EMIT_FORWARD gate.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void q_poseidon_native(const QuotientArgs &a, u64 i, u64 *lds, u32 T, u32 tid, QEmit &emit) {
  const_as<u64> rc = konst(a.rc);
  // the constraints come first to last: constraint j has the weight alpha^j (QTerms; no 1 / alpha, no rescaling)
  QEmit &E = emit;
  E.begin_terms();
  auto emit_term = [&](u64 x) { E.term(a, E.emitted++, x); };
  const u64 *W = a.wires + i;
  const u64 st = a.stride;
  u64 in[12], dl[4], swap;
#pragma unroll
  for (int j = 0; j < 12; j++) in[j] = W[(u64)j * st];
  swap = W[24 * st];
#pragma unroll
  for (int j = 0; j < 4; j++) dl[j] = W[(u64)(25 + j) * st];
  emit_term(gl_mul_nc(swap, gl_sub(swap, 1)));
#pragma unroll
  for (int j = 0; j < 4; j++) emit_term(gl_sub_nc(gl_mul_nc(swap, gl_sub(in[j + 4], in[j])), dl[j]));
  u32 lo[12], hi[12];
#pragma unroll
  for (int j = 0; j < 12; j++) {
    u64 v = j < 4 ? gl_add(in[j], dl[j]) : j < 8 ? gl_sub(in[j], dl[j - 4]) : in[j];
    v = gl_add_nc(v, rc[j]);
    lo[j] = (u32)v; hi[j] = (u32)(v >> 32);
  }
  auto constrain12 = [&](u32 first_wire) {  // state - sbox_in for the 12 lanes, state <- sbox_in
    u64 w[12];
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = W[(u64)(first_wire + j) * st];
#pragma unroll
    for (int j = 0; j < 12; j++) {
      emit_term(gl_sub_nc(((u64)hi[j] << 32) | lo[j], w[j]));
      lo[j] = (u32)w[j]; hi[j] = (u32)(w[j] >> 32);
    }
  };
  u32 round = 0;
#pragma unroll 1
  for (u32 r = 0; r < POS_FULL_HALF; r++, round++) {
    if (r) constrain12(29 + 12 * (r - 1));
#pragma unroll
    for (int j = 0; j < 12; j++) pos_sbox_h(lo[j], hi[j]);
    u64 nxt[12];
#pragma unroll
    for (int j = 0; j < 12; j++) nxt[j] = rc[(round + 1) * 12 + j];
    pos_mds_h(lo, hi, nxt);
  }
  // partial rounds, three at a time as in the hash kernels (poseidon.hpp pos_partial3_core): element 0 after every round is
  // emitted against the gate's S-box wire and the round continues from the wire.  The 22 S-box wires are fetched in groups of
  // QUOTIENT_STAGE through the staging slots (LDS; this kernel has no interpreter registers).
  static_assert(QUOTIENT_STAGE % POS_GROUP == 0, "a group of partial rounds must not straddle two staging batches");
  auto stage_sbox_wires = [&](u32 r) {
    u64 pw[QUOTIENT_STAGE];
#pragma unroll
    for (u32 j = 0; j < QUOTIENT_STAGE; j++) pw[j] = W[(u64)(65 + min(r + j, (u32)POS_PARTIAL - 1)) * st];
#pragma unroll
    for (u32 j = 0; j < QUOTIENT_STAGE; j++) lds[j * T + tid] = pw[j];
  };
  auto constrain0 = [&](u32 r, u32 &ul, u32 &uh) {  // element 0 - S-box wire of partial round r; element 0 <- the wire
    const u64 w = lds[(r % QUOTIENT_STAGE) * T + tid];
    emit_term(gl_sub_nc(((u64)uh << 32) | ul, w));
    ul = (u32)w; uh = (u32)(w >> 32);
  };
  u32 r = 0;
#pragma unroll 1
  for (u32 g = 0; g < POS_GROUPS; g++, r += POS_GROUP, round += POS_GROUP) {
    if (r % QUOTIENT_STAGE == 0) stage_sbox_wires(r);
    constrain0(r, lo[0], hi[0]);
    pos_partial3_core(lo, hi, &rc[POS_ROUNDS * POS_W + POS_GROUP_CONSTS * g], [&](int i, u32 &ul, u32 &uh) {
      constrain0(r + i, ul, uh);
      pos_sbox_h(ul, uh);
    });
  }
#pragma unroll 1
  for (; r < POS_PARTIAL; r++, round++) {  // the round the groups leave over
    if (r % QUOTIENT_STAGE == 0) stage_sbox_wires(r);
    constrain0(r, lo[0], hi[0]);
    pos_sbox_h(lo[0], hi[0]);
    u64 nxt[12];
#pragma unroll
    for (int j = 0; j < 12; j++) nxt[j] = rc[(round + 1) * 12 + j];
    pos_mds_h(lo, hi, nxt);
  }
#pragma unroll 1
  for (u32 r = 0; r < POS_FULL_HALF; r++, round++) {
    constrain12(87 + 12 * r);
#pragma unroll
    for (int j = 0; j < 12; j++) pos_sbox_h(lo[j], hi[j]);
    u64 nxt[12];
#pragma unroll
    for (int j = 0; j < 12; j++) nxt[j] = round + 1 < POS_ROUNDS ? rc[(round + 1) * 12 + j] : 0;
    pos_mds_h(lo, hi, nxt);
  }
  u64 out[12];
#pragma unroll
  for (int j = 0; j < 12; j++) out[j] = W[(u64)(12 + j) * st];
#pragma unroll
  for (int j = 0; j < 12; j++) emit_term(gl_sub_nc(((u64)hi[j] << 32) | lo[j], out[j]));
  E.finish_terms();
}
#endif

// the native evaluators as evaluator types (quotient_common.hpp q_gate_value)
#if defined(__HIP_DEVICE_COMPILE__)
struct QPoseidon {
  static __device__ __forceinline__ void run(const QuotientArgs &a, const GateDev &, u64 i, u64 *lds, u32 T, u32 tid, QEmit &emit) { q_poseidon_native(a, i, lds, T, tid, emit); }
};
// ArithmeticGate and BaseSumGate<2>: light_gates.hpp, one text for each gate alone and for the pair of a light list
struct QArithmetic {
  static __device__ __forceinline__ void run(const QuotientArgs &a, const GateDev &G, u64 i, u64 *, u32, u32, QEmit &emit) { q_arith_base_walk<true, false>(a, i, G.num_constraints, 0, emit, emit); }
};
struct QBaseSum2 {
  static __device__ __forceinline__ void run(const QuotientArgs &a, const GateDev &G, u64 i, u64 *, u32, u32, QEmit &emit) { q_arith_base_walk<false, true>(a, i, 0, G.num_constraints - 1, emit, emit); }
};
// ArithmeticGate gA and BaseSumGate<2> gB of one circuit in one walk over the wires: loaded once, they feed both evaluators
__device__ __forceinline__ void q_pair_values(const QuotientArgs &a, u32 gA, u32 gB, const GateDev &GA, const GateDev &GB, u64 i, u64 valA[QUOTIENT_MAX_CH], u64 valB[QUOTIENT_MAX_CH]) {
  QEmit eA, eB;
  q_emit_begin(a, GA, eA); q_emit_begin(a, GB, eB);
  q_arith_base_walk<true, true>(a, i, GA.num_constraints, GB.num_constraints - 1, eA, eB);
  q_gate_finish(a, gA, GA, i, eA, valA); q_gate_finish(a, gB, GB, i, eB, valB);
}
#else
struct QPoseidon; struct QArithmetic; struct QBaseSum2;
#endif
// The claim check of a pair (launch_native_check), g = gA | gB << 16: each gate's program against its value out of the shared walk
struct QArithBasePair;
template <>
__device__ __forceinline__ void q_claim_check<QArithBasePair>(const QuotientArgs &a, u32 g, u64 i, u64 *lds, u32 T, u32 tid, unsigned long long *flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  const u32 gA = g & 0xFFFFu, gB = g >> 16;
  const GateDev GA = q_load_gate(a, gA), GB = q_load_gate(a, gB);
  u64 pA[QUOTIENT_MAX_CH], pB[QUOTIENT_MAX_CH], vA[QUOTIENT_MAX_CH], vB[QUOTIENT_MAX_CH];
  q_gate_value<QInterpreted>(a, gA, GA, i, lds, T, tid, pA); q_gate_value<QInterpreted>(a, gB, GB, i, lds, T, tid, pB);
  q_pair_values(a, gA, gB, GA, GB, i, vA, vB);
  q_claim_compare(a, i, pA, vA, flag); q_claim_compare(a, i, pB, vB, flag);
#endif
}

// K6 is one launch per gate type plus the permutation pass: every kernel carries only the registers its gate needs (the native
// PoseidonGate wants ~120 VGPRs, the permutation pass ~90, an interpreted gate ~80), so none drags the others' occupancy down,
// and an interpreted gate's LDS registers are not allocated beside a native one.  A gate kernel adds filter * constraints into
// out[c][point] (the first one of a proof stores); the extra traffic is 32 bytes per point and launch, ~1.5 % of what K6 reads.
// The native PoseidonGate is the one plonky2 gate with a kernel to itself (NATIVE names it in the kernel's symbol, which profiles key
// on); the other native gates are light (k_q_light).  Skeleton: quotient_common.hpp.
template <u32 NATIVE, bool CHECK>
__global__ __launch_bounds__(QUOTIENT_THREADS, 2) void k_q_gate(QuotientArgs a, u32 g, u32 accumulate, unsigned long long *flag) {
  static_assert(NATIVE == LCP2_GATE_NATIVE_POSEIDON, "k_q_gate is the PoseidonGate kernel");
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  u64 i;
  if (!q_point<CHECK>(a, i)) return;
  const GateDev G = q_load_gate(a, g);
  if (!q_wave_holds<CHECK>(a, G, i)) return;
  u64 val[QUOTIENT_MAX_CH];
  q_gate_value<QPoseidon>(a, g, G, i, lds, QUOTIENT_THREADS, threadIdx.x, val);
  q_gate_store<CHECK>(a, i, val, accumulate, flag);
#endif
}

// x * 7 for any u64 x, lazy result: the 67-bit product from two multiply-adds, folded with two more (its high word times 2^64 mod p,
// and that sum's carry): 5 instructions of the 4.3-cycle kind against 12 for a general multiply
__device__ __forceinline__ u64 q_mul7_nc(u64 x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const u64 p0 = (u64)(u32)x * 7u, p1 = (u64)(u32)(x >> 32) * 7u + (p0 >> 32);
  u64 lo = (p1 << 32) | (u32)p0;
  const u32 hi = (u32)(p1 >> 32);
  u32 c;
  asm("v_mad_u64_u32 %0, vcc, %2, -1, %0\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e64 %1, 0, 1, vcc\n\t"
      "v_mad_u64_u32 %0, vcc, %1, -1, %0"
      : "+v"(lo), "=&v"(c) : "v"(hi) : "vcc");
  return lo;
#else
  return gl_mul_u32_nc(x, 7u);
#endif
}

// permutation argument + division by Z_H: out[c][point] holds the sum of the gate terms on entry, the quotient value on exit
__global__ __launch_bounds__(QUOTIENT_THREADS, 2) void k_q_perm(QuotientArgs a, u32 have_gates) {
  const u32 T = QUOTIENT_THREADS, tid = threadIdx.x;
  const u64 i = (u64)blockIdx.x * T + tid;  // local storage (leaf) index; global index = a.leaf0 + i
  if (i >= a.count) return;
  const u64 ig = a.leaf0 + i;
  const u32 CH = a.num_challenges;
  u64 res[QUOTIENT_MAX_CH];
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) res[c] = (c < CH && have_gates) ? a.out[(u64)c * a.N + ig] : 0;

  // ---- permutation argument terms, folded in front of the gate constraints:
  //   terms = [ L0 (Z_c - 1) ]_c ++ [ prev * prod num - next * prod den ]_{c,k} ;  out = sum_t alpha^t terms_t + alpha^nt * gates
  // The chunks are walked once for all challenges: the 8 wires and 8 sigmas of a batch and the next partial products are 18
  // loads issued back to back (one HBM round trip per batch instead of one per column) and every column is read once.  The
  // terms of challenge c2 then arrive first to last, so their block sum is a Horner chain with 1 / alpha, weighted afterwards
  // by the power of alpha at which the block starts (alpha_pow: host table; alpha = 0 leaves term 0 alone, handled below).
  const u32 lgN = a.lgN;
  const u64 jnat = bitrev32((u32)ig, lgN);
  const u64 x = two_level(a.points, jnat);  // 7 * w_N^bitrev(ig)
  const u64 inext = bitrev32((u32)((jnat + (1u << a.rate_bits)) & (a.N - 1)), lgN) - a.leaf0;  // same coset = same leaf block
  const u32 npp = a.nchunks - 1;
  u64 beta[QUOTIENT_MAX_CH], gamma[QUOTIENT_MAX_CH], bx[QUOTIENT_MAX_CH], prev[QUOTIENT_MAX_CH], z0[QUOTIENT_MAX_CH];
  u64 bxk[QUOTIENT_MAX_CH];  // beta x k_j of the next wire when k_j = 7^j (a.kis_pow7): lazy, carried with q_mul7_nc
  u64 hh[QUOTIENT_MAX_CH][QUOTIENT_MAX_CH];  // [c2][alpha challenge c]
  u64 ainv[QUOTIENT_MAX_CH];
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) {
    beta[c] = c < CH ? konst(a.betas)[c] : 0; gamma[c] = c < CH ? konst(a.gammas)[c] : 0;
    ainv[c] = c < CH ? konst(a.alpha_inv)[c] : 0;
    bx[c] = gl_mul(beta[c], x);
    bxk[c] = bx[c];
    z0[c] = c < CH ? a.zs[(u64)c * a.stride + i] : 0;
    prev[c] = z0[c];
#pragma unroll
    for (u32 d = 0; d < QUOTIENT_MAX_CH; d++) hh[c][d] = 0;
  }
  for (u32 k = 0; k < a.nchunks; k++) {
    u64 pn[QUOTIENT_MAX_CH], pd[QUOTIENT_MAX_CH], nx[QUOTIENT_MAX_CH];
#pragma unroll
    for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) {
      pn[c] = 1; pd[c] = 1;
      nx[c] = c < CH ? (k < npp ? a.zs[((u64)CH + (u64)c * npp + k) * a.stride + i] : a.zs[(u64)c * a.stride + inext]) : 0;
    }
    const u32 jend = min((k + 1) * a.chunk, a.num_routed);
    for (u32 j0 = k * a.chunk; j0 < jend; j0 += 8) {
      u64 w[8], sg[8];
#pragma unroll
      for (u32 jj = 0; jj < 8; jj++) {  // lanes past the end of the chunk repeat its last column
        const u32 j = min(j0 + jj, jend - 1);
        w[jj] = a.wires[(u64)j * a.stride + i];
        sg[jj] = a.consts[(u64)(a.num_constants + j) * a.stride + i];
      }
#pragma unroll
      for (u32 jj = 0; jj < 8; jj++) {
        if (j0 + jj < jend) {
          const u64 kj = konst(a.k_is)[j0 + jj];
#pragma unroll
          for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
            if (c < CH) {
              // lazy values (any u64 congruent to the element) through the products: gl_mul_nc takes them, and the chunk
              // products only meet canonical arithmetic in the gl_mul of the term below
              const u64 wg = gl_add(w[jj], gamma[c]);
              const u64 bk = a.kis_pow7 ? bxk[c] : gl_mul_nc(bx[c], kj);
              if (a.kis_pow7) bxk[c] = q_mul7_nc(bxk[c]);
              pn[c] = gl_mul_nc(pn[c], gl_add_nc(bk, wg));
              pd[c] = gl_mul_nc(pd[c], gl_add_nc(gl_mul_nc(beta[c], sg[jj]), wg));
            }
        }
      }
    }
#pragma unroll
    for (u32 c2 = 0; c2 < QUOTIENT_MAX_CH; c2++)
      if (c2 < CH) {
        const u64 term = gl_sub(gl_mul(prev[c2], pn[c2]), gl_mul(nx[c2], pd[c2]));
        prev[c2] = nx[c2];
#pragma unroll
        for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
          if (c < CH) hh[c2][c] = gl_add(gl_mul(hh[c2][c], ainv[c]), term);
      }
  }
  const u64 l0 = a.l0[ig];
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
    if (c < CH) {
      const_as<u64> pw = konst(a.alpha_pow) + c * QUOTIENT_ALPHA_POWS;
      u64 l0t[QUOTIENT_MAX_CH];
#pragma unroll
      for (u32 c2 = 0; c2 < QUOTIENT_MAX_CH; c2++) l0t[c2] = c2 < CH ? gl_mul(l0, gl_sub(z0[c2], 1)) : 0;
      if (ainv[c] == 0) { res[c] = l0t[0]; continue; }  // alpha = 0: only the term of weight alpha^0 survives
      u64 r = gl_mul(res[c], pw[CH + CH * a.nchunks]);
#pragma unroll
      for (u32 c2 = 0; c2 < QUOTIENT_MAX_CH; c2++)
        if (c2 < CH) {
          r = gl_add(r, gl_mul(hh[c2][c], pw[CH + c2 * a.nchunks + a.nchunks - 1]));
          r = gl_add(r, gl_mul(l0t[c2], pw[c2]));
        }
      res[c] = r;
    }
  const u64 zhi = a.zh_inv[ig >> (lgN - a.rate_bits)];
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
    if (c < CH) a.out[(u64)c * a.N + ig] = gl_mul(res[c], zhi);
}

// The light gates of a circuit in ONE launch: interpreted gates (Constant, PublicInput and whatever else has no native form) and
// the native ArithmeticGate / BaseSumGate, evaluated one after the other by the same thread with a single update of `out`.  Alone
// each of them is a latency-bound kernel of a few hundred to a few thousand instructions per point (one instruction per 5 - 8
// cycles against 3.7 for the heavy gates); together their loads overlap and three read-modify-write passes over `out` go away.
// pair_a / pair_b: the positions in g[] of the first ArithmeticGate and the first BaseSumGate<2> when the list has both (they share
// one walk over the wires: q_pair_values), LIGHT_NO_PAIR otherwise; chosen on the host (launch_gates)
constexpr u32 LIGHT_NO_PAIR = ~0u;
struct LightGates { u32 count; u32 g[8]; u32 pair_a, pair_b; };
template <bool CHECK>
__global__ __launch_bounds__(QUOTIENT_THREADS, 2) void k_q_light(QuotientArgs a, LightGates L, u32 accumulate, unsigned long long *flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  const u32 T = QUOTIENT_THREADS, tid = threadIdx.x;
  u64 i;
  if (!q_point<CHECK>(a, i)) return;
  u64 sum[QUOTIENT_MAX_CH];
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) sum[c] = 0;
  const u32 ka = L.pair_a, kb = L.pair_b;
  const bool pair = ka != LIGHT_NO_PAIR;
  if (pair) {
    const GateDev GA = q_load_gate(a, L.g[ka]), GB = q_load_gate(a, L.g[kb]);
    if (q_wave_holds<CHECK>(a, GA, i) || q_wave_holds<CHECK>(a, GB, i)) {
      u64 va[QUOTIENT_MAX_CH], vb[QUOTIENT_MAX_CH];
      q_pair_values(a, L.g[ka], L.g[kb], GA, GB, i, va, vb);
#pragma unroll
      for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
        if (c < a.num_challenges) sum[c] = gl_add(va[c], vb[c]);
    }
  }
  for (u32 k = 0; k < L.count; k++) {
    if (pair && (k == ka || k == kb)) continue;
    const u32 g = L.g[k];
    const GateDev G = q_load_gate(a, g);
    if (!q_wave_holds<CHECK>(a, G, i)) continue;
    u64 val[QUOTIENT_MAX_CH];
    switch (G.flags & LCP2_GATE_NATIVE_MASK) {  // wave-uniform
      case LCP2_GATE_NATIVE_ARITHMETIC: q_gate_value<QArithmetic>(a, g, G, i, lds, T, tid, val); break;
      case LCP2_GATE_NATIVE_BASE_SUM2: q_gate_value<QBaseSum2>(a, g, G, i, lds, T, tid, val); break;
      default: q_gate_value<QInterpreted>(a, g, G, i, lds, T, tid, val); break;
    }
#pragma unroll
    for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
      if (c < a.num_challenges) sum[c] = gl_add(sum[c], val[c]);
  }
  // CHECK: on a row of H only the row's own gate has a non-zero filter, so the sum is that gate's value
  q_gate_store<CHECK>(a, i, sum, accumulate, flag);
#endif
}

// a generated evaluator lives in one of the kernels_gates_*.hip units: ask them in turn
static bool launch_generated(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode) {
  return launch_generated_sha(s, a, k, g, accumulate, flag, mode) || launch_generated_u32a(s, a, k, g, accumulate, flag, mode) ||
         launch_generated_u32b(s, a, k, g, accumulate, flag, mode) || launch_generated_reca(s, a, k, g, accumulate, flag, mode) ||
         launch_generated_recb(s, a, k, g, accumulate, flag, mode);
}
namespace {
// a gate with a launch to itself: a generated evaluator or the native PoseidonGate
template <bool CHECK>
void launch_gate(hipStream_t s, const QuotientArgs &a, const GateDev &G, u32 g, u32 accumulate, unsigned long long *flag) {
  const u32 kind = G.flags & LCP2_GATE_NATIVE_MASK;
  if (kind & 0x8000u) {  // validate_programs has bounded the index
    launch_generated(s, a, (kind >> 8) & 0x7Fu, g, accumulate, flag, CHECK ? GEN_ROW_CHECK : GEN_QUOTIENT);
    return;
  }
  const size_t stage = (size_t)QUOTIENT_STAGE * QUOTIENT_THREADS * sizeof(u64);  // the S-box wires of the partial rounds
  hipLaunchKernelGGL((k_q_gate<LCP2_GATE_NATIVE_POSEIDON, CHECK>), q_grid(a), dim3(QUOTIENT_THREADS), stage, s, a, g, accumulate, flag);
}
// a gate that goes into the light-gate launch: no native form, or one of the two small native ones
bool is_light(const GateDev &G) {
  const u32 k = G.flags & LCP2_GATE_NATIVE_MASK;
  return k == 0 || k == LCP2_GATE_NATIVE_ARITHMETIC || k == LCP2_GATE_NATIVE_BASE_SUM2;
}
// the claim check names a pair in one word, gA | gB << 16 (launch_native_check): a gate index that does not fit is never paired
bool pairable(u32 g) { return g < (1u << 16); }
// tier (nullable): only the gates g with tier[g] == want (the full tier is -1, a bundle its index); nullptr: every gate
template <bool CHECK>
u32 launch_gates(hipStream_t s, const QuotientArgs &a, const std::vector<GateDev> &host_gates, unsigned long long *flag, const int *tier = nullptr, int want = -1) {
  u32 launched = 0;
  const LightGates none{0, {}, LIGHT_NO_PAIR, LIGHT_NO_PAIR};
  LightGates L = none;
  auto flush = [&] {
    if (!L.count) return;
    if (L.pair_a == LIGHT_NO_PAIR || L.pair_b == LIGHT_NO_PAIR) L.pair_a = L.pair_b = LIGHT_NO_PAIR;  // one of the two alone: no pair
    hipLaunchKernelGGL((k_q_light<CHECK>), q_grid(a), dim3(QUOTIENT_THREADS), q_interp_lds_bytes(a), s, a, L, launched ? 1u : 0u, flag);
    launched++;
    L = none;
  };
  for (u32 g = 0; g < host_gates.size(); g++) {
    if (host_gates[g].num_constraints == 0 || (tier && tier[g] != want)) continue;
    if (is_light(host_gates[g])) {
      const u32 kind = host_gates[g].flags & LCP2_GATE_NATIVE_MASK;
      if (kind == LCP2_GATE_NATIVE_ARITHMETIC && L.pair_a == LIGHT_NO_PAIR && pairable(g)) L.pair_a = L.count;
      if (kind == LCP2_GATE_NATIVE_BASE_SUM2 && L.pair_b == LIGHT_NO_PAIR && pairable(g)) L.pair_b = L.count;
      L.g[L.count++] = g;
      if (L.count == 8) flush();
      continue;
    }
    launch_gate<CHECK>(s, a, host_gates[g], g, launched ? 1u : 0u, flag);
    launched++;
  }
  flush();
  return launched;
}
}  // namespace

// host_gates: the gate table as uploaded (staged code offsets); gates without constraints are skipped
void launch_quotient(hipStream_t s, const QuotientArgs &a, const std::vector<GateDev> &host_gates) {
  const u32 launched = launch_gates<false>(s, a, host_gates, nullptr);
  launch_quotient_perm(s, a, launched ? 1u : 0u);
}
void launch_quotient_perm(hipStream_t s, const QuotientArgs &a, u32 have_gates) {
  hipLaunchKernelGGL(k_q_perm, q_grid(a), dim3(QUOTIENT_THREADS), 0, s, a, have_gates);
}
u32 launch_quotient_full_tier(hipStream_t s, const QuotientArgs &a, const std::vector<GateDev> &host_gates, const QuotientTiers &t) {
  return launch_gates<false>(s, a, host_gates, nullptr, t.bundle_of.data(), -1);
}
void launch_quotient_half_tier(hipStream_t s, const QuotientArgs &a, const std::vector<GateDev> &host_gates, const QuotientTiers &t, u64 *planes) {
  for (size_t b = 0; b < t.bundles.size(); b++) {  // the first launch of a bundle stores its planes, the others accumulate
    QuotientArgs ab = a;
    ab.out = planes + (u64)b * a.num_challenges * a.N;
    launch_gates<false>(s, ab, host_gates, nullptr, t.bundle_of.data(), (int)b);
  }
}

// Half tier, last step: the planes of up to 8 bundles (extended to the whole coset) times what their gates' filters left out
struct TierCombine { u32 count; u32 selector_index[8], group_start[8], group_end[8]; u64 mask[8]; };
__global__ __launch_bounds__(256) void k_q_tier_combine(QuotientArgs a, const u64 *__restrict__ planes, TierCombine T, u32 accumulate) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.count) return;
  const u32 CH = a.num_challenges;
  const u64 ig = a.leaf0 + i;
  u64 acc[QUOTIENT_MAX_CH];
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) acc[c] = (c < CH && accumulate) ? a.out[(u64)c * a.N + ig] : 0;
  for (u32 b = 0; b < T.count; b++) {
    const u32 gs = T.group_start[b], ge = T.group_end[b];
    const u64 mask = T.mask[b];
    const u64 s = a.consts[(u64)T.selector_index[b] * a.stride + i];
    u64 v[QUOTIENT_MAX_CH];
#pragma unroll
    for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) v[c] = c < CH ? planes[((u64)b * CH + c) * a.N + ig] : 0;
    u64 f = 1;
    for (u32 j = gs; j < ge; j++) {
      const bool in_bundle = (mask >> ((j - gs) & 63)) & 1;  // groups of <= 64 values (form_bundles)
      if (!in_bundle) f = gl_mul(f, gl_sub((u64)j, s));
    }
    if (a.num_selectors > 1) f = gl_mul(f, gl_sub(0xFFFFFFFFull, s));
#pragma unroll
    for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
      if (c < CH) acc[c] = gl_add(acc[c], gl_mul(f, v[c]));
  }
#pragma unroll
  for (u32 c = 0; c < QUOTIENT_MAX_CH; c++)
    if (c < CH) a.out[(u64)c * a.N + ig] = acc[c];
}
void launch_tier_combine(hipStream_t s, const QuotientArgs &a, const QuotientTiers &t, const u64 *planes, u32 accumulate) {
  for (size_t b0 = 0; b0 < t.bundles.size(); b0 += 8) {
    TierCombine T{};
    T.count = (u32)std::min<size_t>(8, t.bundles.size() - b0);
    for (u32 k = 0; k < T.count; k++) {
      const QuotientBundle &B = t.bundles[b0 + k];
      T.selector_index[k] = B.selector_index; T.group_start[k] = B.group_start; T.group_end[k] = B.group_end; T.mask[k] = B.mask;
    }
    hipLaunchKernelGGL(k_q_tier_combine, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, s, a, planes + (u64)b0 * a.num_challenges * a.N, T, b0 ? 1u : accumulate);
  }
}
void launch_gate_check(hipStream_t s, const QuotientArgs &a, const std::vector<GateDev> &host_gates, unsigned long long *flag) {
  launch_gates<true>(s, a, host_gates, flag);
}
// Every claim against its program on the points of `a`: the generated evaluators, the native PoseidonGate, ArithmeticGate and
// BaseSumGate<2> each alone, and every ArithmeticGate with every BaseSumGate<2> (whichever two a tier's light list pairs) out of
// the shared walk, each gate against its own program.  Compared: filter * sum_j alpha^j c_j per challenge, that is constraint
// values, their weights and the filter.  Not compared: the kernels' wave votes and stores (the proofs' parity tests hold those).
void launch_native_check(hipStream_t s, const QuotientArgs &a, const std::vector<GateDev> &host_gates, unsigned long long *flag) {
  auto kind_of = [&](u32 g) { return host_gates[g].flags & LCP2_GATE_NATIVE_MASK; };
  for (u32 g = 0; g < host_gates.size(); g++) {
    const u32 kind = kind_of(g);
    if (kind & 0x8000u) { launch_generated(s, a, (kind >> 8) & 0x7Fu, g, 0, flag, GEN_CLAIM_CHECK); continue; }
    switch (kind) {
      case LCP2_GATE_NATIVE_POSEIDON: launch_claim_check<QPoseidon>(s, a, g, flag); break;
      case LCP2_GATE_NATIVE_ARITHMETIC: launch_claim_check<QArithmetic>(s, a, g, flag);
        for (u32 gB = 0; gB < host_gates.size() && pairable(g) && pairable(gB); gB++)  // an ArithmeticGate only: its pairs
          if (kind_of(gB) == LCP2_GATE_NATIVE_BASE_SUM2) launch_claim_check<QArithBasePair>(s, a, g | gB << 16, flag);
        break;
      case LCP2_GATE_NATIVE_BASE_SUM2: launch_claim_check<QBaseSum2>(s, a, g, flag); break;
      default: break;
    }
  }
}

// ------------------------------------------------------------------ challenge-dependent setup of K6 (prover_kernels.hpp)
__global__ __launch_bounds__(256) void k_quotient_setup(QuotientSetupArgs a) {
  const u32 t = threadIdx.x, CH = a.num_challenges;
  if (t < QUOTIENT_TERM_POWS) {  // alpha_c^t: the limb table and the first QUOTIENT_ALPHA_POWS plain powers
    for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) {
      const u64 pw = c < CH ? gl_pow(a.alphas[c], t) : 0;
      u32 *w = a.limbs + ((size_t)c * QUOTIENT_TERM_POWS + t) * 4;
      w[0] = (u32)(pw & 0x3FFFFF); w[1] = (u32)((pw >> 22) & 0x3FFFFF); w[2] = (u32)(pw >> 44); w[3] = 0;
      if (t < QUOTIENT_ALPHA_POWS) a.small[SMALL_ALPHA_POW + (size_t)c * QUOTIENT_ALPHA_POWS + t] = pw;
    }
  } else if (t < 255) {          // alpha_c^(m_g - 1) for every gate g
    for (u32 g = t - QUOTIENT_TERM_POWS; g < a.num_gates; g += 255 - QUOTIENT_TERM_POWS) {
      const u32 m = konst((const u32 *)a.gates)[(size_t)g * GW_WORDS + GW_NUM_CONSTRAINTS];
      for (u32 c = 0; c < QUOTIENT_MAX_CH; c++) a.small[SMALL_GATE_SCALE + (size_t)g * QUOTIENT_MAX_CH + c] = c < CH ? (m ? gl_pow(a.alphas[c], m - 1) : 1) : 0;
    }
  } else {                       // the scalars
    for (u32 c = 0; c < 4; c++) {
      const u64 al = c < CH ? a.alphas[c] : 0;
      a.small[SMALL_ALPHAS + c] = al;
      a.small[SMALL_ALPHA_INV + c] = al ? gl_inv(al) : 0;
      a.small[SMALL_PI_HASH + c] = a.pi_hash[c];
    }
    a.small[SMALL_CHECK] = ~0ull;
  }
}
void launch_quotient_setup(hipStream_t s, const QuotientSetupArgs &a) {
  static_assert(QUOTIENT_TERM_POWS < 255 && QUOTIENT_MAX_CH <= 4 && QUOTIENT_ALPHA_POWS <= QUOTIENT_TERM_POWS, "k_quotient_setup's thread map");
  hipLaunchKernelGGL(k_quotient_setup, dim3(1), dim3(256), 0, s, a);
}

// Coset-sharded proof: the quotient chunks out of the per-coset interpolants.  in[c][b * n + l] is coefficient l of the polynomial
// of degree < n that agrees with challenge c's quotient on leaf block b (the coset of shift s_b); the quotient is
// sum_k x^(k n) Q_k(x) and x^n = s_b^n on that coset, so the interpolants are a size-R transform of the chunks Q_k, coefficient by
// coefficient, and out[c][k * n + l] = sum_b m[k][b] in[c][b * n + l] with the inverse matrix m (prover_stages.hip).
__global__ __launch_bounds__(256) void k_quotient_combine(const u64 *__restrict__ in, u64 *__restrict__ out, const u64 *__restrict__ m, u64 n, u32 R, u64 plane) {
  const u64 l = (u64)blockIdx.x * 256 + threadIdx.x;
  if (l >= n) return;
  const u64 base = (u64)blockIdx.y * plane + l;
  u64 r[8];
#pragma unroll
  for (u32 b = 0; b < 8; b++) r[b] = b < R ? in[base + (u64)b * n] : 0;
  for (u32 k = 0; k < R; k++) {
    u64 acc = 0;
#pragma unroll
    for (u32 b = 0; b < 8; b++)
      if (b < R) acc = gl_add(acc, gl_mul(m[k * R + b], r[b]));
    out[base + (u64)k * n] = acc;
  }
}
void launch_quotient_combine(hipStream_t s, const u64 *in, u64 *out, const u64 *m, u64 n, u32 R, u64 plane, u32 num_challenges) {
  hipLaunchKernelGGL(k_quotient_combine, dim3((unsigned)((n + 255) / 256), num_challenges), dim3(256), 0, s, in, out, m, n, R, plane);
}
}  // namespace lcp2
