// Kernels of the generated straight-line gate evaluators (csrc/generated_gates_<unit>.hpp, tools/gen/gen_native_gates.cpp).  Every
// compile unit kernels_gates_<unit>.hip includes its own generated header and this file and defines, through
// LCP2_DEFINE_GENERATED_UNIT, the launcher of its programs; kernels_quotient.hip asks the units one after the other
// (launch_generated).  One kernel per program and mode: the quotient values on the LDE points, the same evaluation over the rows of H
// (LCP2_E_UNSAT check), and the build()-time check of the LCP2_GATE_NATIVE_GENERATED claim against the interpreted program
// (k_claim_check: the one kernel of that kind, kernels_quotient.hip instantiates it for the native plonky2 gates too).
#pragma once
#include <utility>
#include "quotient_common.hpp"

namespace lcp2 {

enum GeneratedMode : u32 { GEN_QUOTIENT = 0, GEN_ROW_CHECK = 1, GEN_CLAIM_CHECK = 2 };

#if defined(__HIP_DEVICE_COMPILE__)
template <u32 K> struct QGenerated {
  static __device__ __forceinline__ void run(const QuotientArgs &a, const GateDev &, u64 i, u64 *, u32, u32, QEmit &emit) { q_generated<K>(a, i, emit); }
};
#else
template <u32 K> struct QGenerated;
#endif

// the skeleton of quotient_common.hpp around generated program K
template <u32 K, bool CHECK>
__global__ __launch_bounds__(QUOTIENT_THREADS, Q_GENERATED_WAVES[K]) void k_q_gen(QuotientArgs a, u32 g, u32 accumulate, unsigned long long *flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  const u32 T = QUOTIENT_THREADS, tid = threadIdx.x;
  u64 i;
  const bool live = q_point<CHECK>(a, i);
  q_stage_limbs(a, lds, T, tid);  // ends in a barrier: every thread comes here
  if (!live) return;
  const GateDev G = q_load_gate(a, g);
  if (!q_wave_holds<CHECK>(a, G, i)) return;
  u64 val[QUOTIENT_MAX_CH];
  q_gate_value<QGenerated<K>>(a, g, G, i, lds, T, tid, val);
  q_gate_store<CHECK>(a, i, val, accumulate, flag);
#endif
}

// build()-time check of a claim: program (interpreted) against evaluator EVAL on random points in a.wires / a.consts.  The alpha-limb
// table sits in LDS behind the interpreter's registers and staging slots (a.limbs_lds_word), whether EVAL reads it there or not.
template <class EVAL>
__global__ __launch_bounds__(QUOTIENT_THREADS, 2) void k_claim_check(QuotientArgs a, u32 g, unsigned long long *flag) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  const u32 T = QUOTIENT_THREADS, tid = threadIdx.x;
  const u64 i = (u64)blockIdx.x * T + tid;
  q_stage_limbs(a, lds, T, tid);
  if (i >= a.count) return;
  q_claim_check<EVAL>(a, g, i, lds, T, tid, flag);
}
template <class EVAL>
void launch_claim_check(hipStream_t s, const QuotientArgs &a, u32 g, unsigned long long *flag) {
  QuotientArgs ag = a;
  ag.limbs_lds_word = (a.num_regs + QUOTIENT_STAGE) * QUOTIENT_THREADS;
  hipLaunchKernelGGL((k_claim_check<EVAL>), q_grid(a), dim3(QUOTIENT_THREADS), q_interp_lds_bytes(a) + Q_LIMB_WORDS32 * 4, s, ag, g, flag);
}

// a: the arguments of the launch as the caller built them (limbs_lds_word / dynamic LDS are set here)
template <u32 K>
void launch_generated_one(hipStream_t s, const QuotientArgs &a, u32 g, u32 accumulate, unsigned long long *flag, u32 mode) {
  if (mode == GEN_CLAIM_CHECK) { launch_claim_check<QGenerated<K>>(s, a, g, flag); return; }
  const dim3 block(QUOTIENT_THREADS);
  const size_t limbs = Q_LIMB_WORDS32 * 4;  // the LDS copy of the alpha-limb table
  QuotientArgs ag = a;
  ag.limbs_lds_word = 0;
  if (mode == GEN_ROW_CHECK) hipLaunchKernelGGL((k_q_gen<K, true>), q_grid(a), block, limbs, s, ag, g, accumulate, flag);
  else hipLaunchKernelGGL((k_q_gen<K, false>), q_grid(a), block, limbs, s, ag, g, accumulate, flag);
}

template <u32 FIRST, size_t... I>
bool launch_generated_unit(std::index_sequence<I...>, hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode) {
  bool hit = false;
  ((k == FIRST + I ? (launch_generated_one<FIRST + (u32)I>(s, a, g, accumulate, flag, mode), hit = true) : false), ...);
  return hit;
}

// true if program k belongs to this unit (and has been launched)
#define LCP2_DEFINE_GENERATED_UNIT(name, FIRST, COUNT)                                                                                          \
  bool launch_generated_##name(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode) {       \
    return launch_generated_unit<FIRST>(std::make_index_sequence<COUNT>{}, s, a, k, g, accumulate, flag, mode);                                 \
  }

bool launch_generated_sha(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode);
bool launch_generated_u32a(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode);
bool launch_generated_u32b(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode);
bool launch_generated_reca(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode);
bool launch_generated_recb(hipStream_t s, const QuotientArgs &a, u32 k, u32 g, u32 accumulate, unsigned long long *flag, u32 mode);

}  // namespace lcp2
