// The two light native plonky2 gates of K6 as ONE walk over the wires (both read them from index 0 up):
//   ArithmeticGate { num_ops } (gates/arithmetic_base.rs): constraint k = output - (c0 * m0 * m1 + c1 * addend), wires 4k .. 4k+3
//   BaseSumGate<2> { num_limbs } (gates/base_sum.rs): constraint 0 = sum_l 2^l limb_l - wire 0, constraint 1 + l = limb_l^2 - limb_l
// q_arith_base_walk<true, true> is the pair branch of k_q_light (kernels_quotient.hip), a gate alone the same text with the other
// half compiled out (QArithmetic, QBaseSum2); tests/emu/emu_gates.cpp compiles all three for the CPU.  Portable: gl_* of gl64.hpp
// and begin_terms / term / finish_terms of the caller's QEmit.  Constraint j has the weight alpha^j from the table, in whatever
// order the walk meets it, so a gate has at most QUOTIENT_TERM_POWS constraints (validate_programs, prover_build.hip).
#pragma once
#include "gl64.hpp"

namespace lcp2 {

// The wires come 16 at a time from the top, in 16-aligned batches [hi - 16, hi); a batch that reaches past wire num_wires - 1
// re-reads that wire and guards what it emits.  The sum is recomposed on the way (Horner from the top limb down).
template <bool A, bool B, class Args, class Emit>
LCP2_HD void q_arith_base_walk(const Args &a, u64 i, u32 ops, u32 limbs, Emit &eA, Emit &eB) {
  if (A) eA.begin_terms();
  if (B) eB.begin_terms();
  const int num_ops = A ? (int)ops : 0, num_limbs = B ? (int)limbs : 0;
  const u64 *W = a.wires + i;
  const u64 st = a.stride;
  const u64 c0 = A ? a.consts[(u64)a.num_selectors * st + i] : 0, c1 = A ? a.consts[(u64)(a.num_selectors + 1) * st + i] : 0;
  const int wires_b = B ? num_limbs + 1 : 0, top_wire = 4 * num_ops > wires_b ? 4 * num_ops : wires_b, last_wire = (int)a.num_wires - 1;
  u64 sum = 0, w0 = 0;
  for (int hi = (top_wire + 15) & ~15; hi > 0; hi -= 16) {  // wires [hi - 16, hi)
    u64 w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = W[(u64)(hi - 16 + j < last_wire ? hi - 16 + j : last_wire) * st];
#pragma unroll
    for (int kk = 3; kk >= 0; kk--) {
      if (A && (hi - 16) / 4 + kk < num_ops) {
        const u64 comp = gl_add(gl_mul(gl_mul(w[4 * kk], w[4 * kk + 1]), c0), gl_mul(w[4 * kk + 2], c1));
        eA.term(a, (u32)((hi - 16) / 4 + kk), gl_sub(w[4 * kk + 3], comp));
      }
    }
#pragma unroll
    for (int j = 15; j >= 0; j--) {
      const int limb = hi - 16 + j - 1;  // wire 0 is the sum, limb l sits on wire l + 1
      if (B && limb >= 0 && limb < num_limbs) {
        eB.term(a, (u32)(1 + limb), gl_mul_nc(w[j], gl_sub(w[j], 1)));
        sum = gl_add(gl_add(sum, sum), w[j]);
      }
    }
    if (hi == 16) w0 = w[0];
  }
  if (B) eB.term(a, 0, gl_sub(sum, w0));
  if (A) eA.finish_terms();
  if (B) eB.finish_terms();
}

}  // namespace lcp2
