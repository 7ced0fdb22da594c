// Micro-benchmark of the 64 x 64 -> 64 Goldilocks multiply (csrc/gl64.hpp gl_mul_halves), four forms, results compared:
//   current   the carry-chain form of rounds 2-4: four v_mad_u64_u32, the 128-bit product summed by add-with-carry, the reduction on carry
//             chains (17 instructions)
//   chained   the partial products ride in the 64-bit addend of v_mad_u64_u32 (p = a0 b0; t = a0 b1 + p_hi; u = a1 b0 + t (carry c);
//             v = a1 b1 + (u_hi + c 2^32)): the three add-with-carry of the product become register moves
//   chained2  + both conditional corrections of the reduction as multiply-adds of a selected factor (selects in VOP2, constants in VGPRs)
//   chained3  + selects in VOP3 with inline constants, no constant VGPRs: what gl_mul_halves is now (12 instructions + 2 moves)
//   branch    chained3 without the borrow correction of t = lo - hi1 on the hot path (one operand pair in 2^32 needs it): the borrow
//             leaves v_subbrev_co in an SGPR pair, a scalar test of the pair guards a cold block that applies the correction to the
//             lanes of the mask (10 instructions + 2 moves + the scalar compare and branch)
// 12 independent chains of dependent multiplies per lane (x <- x * y, the shape of a full round's S-box layer).
// Then the unit Poseidon uses, x <- x^7 (four multiplies), 12 independent chains, three forms:
//   exact     four gl_mul_halves (pos_sbox_exact_h)
//   branch4   four multiplies of the form `branch` above: a scalar test per multiply
//   spec      four gl_mul_halves_spec, their borrow masks OR-ed, one scalar test per x^7; the cold path recomputes with `exact`
//             (pos_sbox_h, csrc/poseidon.hpp)
// Random operands never borrow here, so the cold paths are compiled and never run; tests/test_rare_borrow.py runs them.
//     hipcc --offload-arch=gfx950 -O3 -o tools/ubench/mulchain tools/ubench/mulchain.hip && tools/ubench/mulchain [waves per SIMD: 1 2 3 4 8]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/poseidon.hpp"
using namespace lcp2;
#define ITER 512
#define CH 12

#if defined(__HIP_DEVICE_COMPILE__)
// the carry-chain form of rounds 2-4 (17 instructions), kept here as the baseline
__device__ __forceinline__ void mul_carry_chain(u32 a0, u32 a1, u32 b0, u32 b1, u32 &r0, u32 &r1, u32 k1, u32 km1) {
  u64 p = (u64)a0 * b0, m = (u64)a0 * b1, h = (u64)a1 * b1;
  u32 c;
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %1, 0, %4, vcc"
      : "+v"(m), "=v"(c) : "v"(a1), "v"(b0), "v"(k1) : "vcc");
  const u32 p0 = (u32)p, p1 = (u32)(p >> 32), m0 = (u32)m, m1 = (u32)(m >> 32), h0 = (u32)h, h1 = (u32)(h >> 32);
  u32 lo1, hi0, hi1;  // 128-bit product = (hi1:hi0:lo1:p0)
  asm("v_add_co_u32 %0, vcc, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, vcc, %5, %6, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %2, vcc, %7, %8, vcc"
      : "=&v"(lo1), "=&v"(hi0), "=&v"(hi1) : "v"(p1), "v"(m0), "v"(h0), "v"(m1), "v"(h1), "v"(c) : "vcc");
  u32 t0, t1, e;  // t = lo - hi1 ; on borrow t -= 2^32 - 1
  asm("v_sub_co_u32 %0, vcc, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %5, vcc\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %2, 0, %6, vcc\n\t"
      "v_sub_co_u32 %0, vcc, %0, %2\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %1, vcc"
      : "=&v"(t0), "=&v"(t1), "=&v"(e) : "v"(p0), "v"(hi1), "v"(lo1), "v"(km1) : "vcc");
  u64 t = ((u64)t1 << 32) | t0, r;  // r = hi0 * (2^32 - 1) + t ; on carry r += 2^32 - 1
  u32 e2;
  asm("v_mad_u64_u32 %0, vcc, %2, -1, %3\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %1, 0, %4, vcc"
      : "=&v"(r), "=v"(e2) : "v"(hi0), "v"(t), "v"(km1) : "vcc");
  u32 q0 = (u32)r, q1 = (u32)(r >> 32);
  asm("v_add_co_u32 %0, vcc, %2, %4\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, vcc, 0, %3, vcc"
      : "=&v"(r0), "=&v"(r1) : "v"(q0), "v"(q1), "v"(e2) : "vcc");
}

__device__ __forceinline__ void mul_chained(u32 a0, u32 a1, u32 b0, u32 b1, u32 &r0, u32 &r1, u32 k1, u32 km1) {
  const u64 p = (u64)a0 * b0;
  const u64 t = (u64)a0 * b1 + (p >> 32);  // < 2^64: (2^32 - 1)^2 + 2^32 - 1
  u64 u;
  u32 c;
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %1, 0, %5, vcc"
      : "=&v"(u), "=&v"(c) : "v"(a1), "v"(b0), "v"(t), "v"(k1) : "vcc");
  const u64 v = (u64)a1 * b1 + (((u64)c << 32) | (u32)(u >> 32));  // < 2^64
  const u32 p0 = (u32)p, lo1 = (u32)u, hi0 = (u32)v, hi1 = (u32)(v >> 32);
  u32 t0, t1, e;  // t = lo - hi1 ; on borrow t -= 2^32 - 1
  asm("v_sub_co_u32 %0, vcc, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %5, vcc\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %2, 0, %6, vcc\n\t"
      "v_sub_co_u32 %0, vcc, %0, %2\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %1, vcc"
      : "=&v"(t0), "=&v"(t1), "=&v"(e) : "v"(p0), "v"(hi1), "v"(lo1), "v"(km1) : "vcc");
  u64 tt = ((u64)t1 << 32) | t0, r;
  u32 e2;
  asm("v_mad_u64_u32 %0, vcc, %2, -1, %3\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %1, 0, %4, vcc"
      : "=&v"(r), "=v"(e2) : "v"(hi0), "v"(tt), "v"(km1) : "vcc");
  u32 q0 = (u32)r, q1 = (u32)(r >> 32);
  asm("v_add_co_u32 %0, vcc, %2, %4\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, vcc, 0, %3, vcc"
      : "=&v"(r0), "=&v"(r1) : "v"(q0), "v"(q1), "v"(e2) : "vcc");
}
// variant 2: chained product, and the two conditional corrections of the reduction as multiply-adds:
//   t -= (2^32 - 1) on borrow   ==  t + sel * 65537 with sel = borrow ? -65535 : 0   (v_mad_i64_i32: -65535 * 65537 = -(2^32 - 1))
//   r += (2^32 - 1) on carry    ==  r + c * (2^32 - 1)  with c = carry ? 1 : 0        (v_mad_u64_u32)
__device__ __forceinline__ void mul_chained2(u32 a0, u32 a1, u32 b0, u32 b1, u32 &r0, u32 &r1, u32 k1, u32 km1, u32 kn, u32 sk) {
  const u64 p = (u64)a0 * b0;
  const u64 t = (u64)a0 * b1 + (p >> 32);
  u64 u;
  u32 c;
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %1, 0, %5, vcc"
      : "=&v"(u), "=&v"(c) : "v"(a1), "v"(b0), "v"(t), "v"(k1) : "vcc");
  const u64 v = (u64)a1 * b1 + (((u64)c << 32) | (u32)(u >> 32));
  const u32 p0 = (u32)p, lo1 = (u32)u, hi0 = (u32)v, hi1 = (u32)(v >> 32);
  u32 t0, t1, sel;
  asm("v_sub_co_u32 %0, vcc, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %5, vcc\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %2, 0, %6, vcc"
      : "=&v"(t0), "=&v"(t1), "=&v"(sel) : "v"(p0), "v"(hi1), "v"(lo1), "v"(kn) : "vcc");
  u64 tt = ((u64)t1 << 32) | t0, r;
  u32 c2;
  asm("v_mad_i64_i32 %0, vcc, %2, %3, %0\n\t"
      "v_mad_u64_u32 %0, vcc, %4, -1, %0\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e32 %1, 0, %5, vcc"
      : "+v"(tt), "=&v"(c2) : "v"(sel), "s"(sk), "v"(hi0), "v"(k1) : "vcc");
  asm("v_mad_u64_u32 %0, vcc, %1, -1, %2" : "=v"(r) : "v"(c2), "v"(tt) : "vcc");
  r0 = (u32)r; r1 = (u32)(r >> 32);
}
// variant 3: variant 2 with the selects in the VOP3 encoding (inline constants 1 and -15, 0x11111111 in an SGPR): no constant VGPRs
__device__ __forceinline__ void mul_chained3(u32 a0, u32 a1, u32 b0, u32 b1, u32 &r0, u32 &r1, u32 sk) {
  const u64 p = (u64)a0 * b0;
  const u64 t = (u64)a0 * b1 + (p >> 32);
  u64 u;
  u32 c;
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e64 %1, 0, 1, vcc"
      : "=&v"(u), "=&v"(c) : "v"(a1), "v"(b0), "v"(t) : "vcc");
  const u64 v = (u64)a1 * b1 + (((u64)c << 32) | (u32)(u >> 32));
  const u32 p0 = (u32)p, lo1 = (u32)u, hi0 = (u32)v, hi1 = (u32)(v >> 32);
  u32 t0, t1, sel;
  asm("v_sub_co_u32 %0, vcc, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %5, vcc\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e64 %2, 0, -15, vcc"
      : "=&v"(t0), "=&v"(t1), "=&v"(sel) : "v"(p0), "v"(hi1), "v"(lo1) : "vcc");
  u64 tt = ((u64)t1 << 32) | t0, r;
  u32 c2;
  asm("v_mad_i64_i32 %0, vcc, %2, %3, %0\n\t"
      "v_mad_u64_u32 %0, vcc, %4, -1, %0\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e64 %1, 0, 1, vcc"
      : "+v"(tt), "=&v"(c2) : "v"(sel), "s"(sk), "v"(hi0) : "vcc");
  asm("v_mad_u64_u32 %0, vcc, %1, -1, %2" : "=v"(r) : "v"(c2), "v"(tt) : "vcc");
  r0 = (u32)r; r1 = (u32)(r >> 32);
}
// form (a): the borrow in an SGPR pair, a scalar branch per multiply, today's correction in the cold block
__device__ __forceinline__ void mul_branch(u32 a0, u32 a1, u32 b0, u32 b1, u32 &r0, u32 &r1, u32 sk) {
  const u64 p = (u64)a0 * b0;
  const u64 t = (u64)a0 * b1 + (p >> 32);
  u64 u;
  u32 c;
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e64 %1, 0, 1, vcc"
      : "=&v"(u), "=&v"(c) : "v"(a1), "v"(b0), "v"(t) : "vcc");
  const u64 v = (u64)a1 * b1 + (((u64)c << 32) | (u32)(u >> 32));
  const u32 p0 = (u32)p, lo1 = (u32)u, hi0 = (u32)v, hi1 = (u32)(v >> 32);
  u32 t0, t1;
  u64 bm;
  asm("v_sub_co_u32 %0, vcc, %3, %4\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32_e64 %1, %2, 0, %5, vcc"
      : "=&v"(t0), "=&v"(t1), "=s"(bm) : "v"(p0), "v"(hi1), "v"(lo1) : "vcc");
  u64 tt = ((u64)t1 << 32) | t0, r;
  if (__builtin_expect(bm != 0, 0)) {
    u32 sel;
    asm("s_nop 1\n\t"
        "v_cndmask_b32_e64 %1, 0, -15, %2\n\t"
        "v_mad_i64_i32 %0, vcc, %1, %3, %0"
        : "+v"(tt), "=&v"(sel) : "s"(bm), "s"(sk) : "vcc");
  }
  u32 c2;
  asm("v_mad_u64_u32 %0, vcc, %2, -1, %0\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_e64 %1, 0, 1, vcc"
      : "+v"(tt), "=&v"(c2) : "v"(hi0) : "vcc");
  asm("v_mad_u64_u32 %0, vcc, %1, -1, %2" : "=v"(r) : "v"(c2), "v"(tt) : "vcc");
  r0 = (u32)r; r1 = (u32)(r >> 32);
}
__device__ __forceinline__ void sbox_branch4(u32 &x0, u32 &x1, u32 sk) {
  u32 a0, a1, b0, b1, c0, c1;
  mul_branch(x0, x1, x0, x1, a0, a1, sk);
  mul_branch(a0, a1, a0, a1, b0, b1, sk);
  mul_branch(x0, x1, a0, a1, c0, c1, sk);
  mul_branch(c0, c1, b0, b1, x0, x1, sk);
}
#endif

#define NMUL 5
#define NX7 3
static const char *const MUL_NAME[NMUL] = {"current", "chained", "chained2", "chained3", "branch"};
static const char *const X7_NAME[NX7] = {"x7 exact", "x7 branch4", "x7 spec"};

template <int V>
__global__ __launch_bounds__(256) void k_chain(u64 *out, u64 seed) {
  extern __shared__ u64 lds_pad[];  // only there to limit the waves per SIMD
  if (seed == 1) lds_pad[threadIdx.x] = seed;
#if defined(__HIP_DEVICE_COMPILE__)
  u32 k1, km1;
  asm volatile("v_mov_b32 %0, 1\n\tv_mov_b32 %1, -1" : "=v"(k1), "=v"(km1));
  u32 kn, sk;
  asm volatile("v_mov_b32 %0, 0xffff0001\n\ts_mov_b32 %1, 0x10001" : "=v"(kn), "=s"(sk));
  u32 sk3;
  asm volatile("s_mov_b32 %0, 0x11111111" : "=s"(sk3));
  u32 x0[CH], x1[CH], y0[CH], y1[CH];
  for (int i = 0; i < CH; i++) {
    const u64 a = seed * (2 * i + 3) + threadIdx.x * 0x9E3779B97F4A7C15ull + blockIdx.x, b = seed * (2 * i + 5) ^ (a >> 7);
    x0[i] = (u32)a; x1[i] = (u32)(a >> 32); y0[i] = (u32)b; y1[i] = (u32)(b >> 32);
  }
#pragma unroll 1
  for (int it = 0; it < ITER; it++) {
#pragma unroll
    for (int i = 0; i < CH; i++) {
      if (V == 0) mul_carry_chain(x0[i], x1[i], y0[i], y1[i], x0[i], x1[i], k1, km1);
      else if (V == 1) mul_chained(x0[i], x1[i], y0[i], y1[i], x0[i], x1[i], k1, km1);
      else if (V == 2) mul_chained2(x0[i], x1[i], y0[i], y1[i], x0[i], x1[i], k1, km1, kn, sk);
      else if (V == 3) mul_chained3(x0[i], x1[i], y0[i], y1[i], x0[i], x1[i], sk3);
      else mul_branch(x0[i], x1[i], y0[i], y1[i], x0[i], x1[i], sk3);
    }
  }
  u64 s = 0;
  for (int i = 0; i < CH; i++) s ^= gl_canon(((u64)x1[i] << 32) | x0[i]) * (i + 1);
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
#endif
}

// x <- x^7, ITER / 4 times: as many multiplies as k_chain
template <int V>
__global__ __launch_bounds__(256) void k_x7(u64 *out, u64 seed) {
  extern __shared__ u64 lds_pad[];
  if (seed == 1) lds_pad[threadIdx.x] = seed;
#if defined(__HIP_DEVICE_COMPILE__)
  u32 sk3;
  asm volatile("s_mov_b32 %0, 0x11111111" : "=s"(sk3));
  u32 x0[CH], x1[CH];
  for (int i = 0; i < CH; i++) {
    const u64 a = seed * (2 * i + 3) + threadIdx.x * 0x9E3779B97F4A7C15ull + blockIdx.x;
    x0[i] = (u32)a; x1[i] = (u32)(a >> 32);
  }
#pragma unroll 1
  for (int it = 0; it < ITER / 4; it++) {
#pragma unroll
    for (int i = 0; i < CH; i++) {
      if (V == 0) pos_sbox_exact_h(x0[i], x1[i]);
      else if (V == 1) sbox_branch4(x0[i], x1[i], sk3);
      else pos_sbox_h(x0[i], x1[i]);
    }
  }
  u64 s = 0;
  for (int i = 0; i < CH; i++) s ^= gl_canon(((u64)x1[i] << 32) | x0[i]) * (i + 1);
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
#endif
}

template <class K>
static void launch(K kernel, int blocks, int threads, size_t lds, u64 *d) {
  hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, 0, d, 12345ull);
}

int main(int argc, char **argv) {
  const int blocks = 256 * 8, threads = 256, reps = 16, warm = 8;
  const int waves = argc > 1 ? atoi(argv[1]) : 8;  // waves per SIMD, set through the LDS a block asks for
  const size_t lds = waves >= 8 ? 0 : (size_t)(160 * 1024 / waves) & ~(size_t)255;
  printf("%d waves per SIMD (%zu bytes of LDS per 4-wave block), 524288 lanes\n", waves, lds);
  typedef void (*kern_t)(u64 *, u64);
  const kern_t kern[NMUL + NX7] = {k_chain<0>, k_chain<1>, k_chain<2>, k_chain<3>, k_chain<4>, k_x7<0>, k_x7<1>, k_x7<2>};
  u64 *d[NMUL + NX7];
  std::vector<u64> h[NMUL + NX7];
  for (int v = 0; v < NMUL + NX7; v++) { hipMalloc(&d[v], (size_t)blocks * threads * 8); h[v].resize((size_t)blocks * threads); }
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  double cyc[NMUL + NX7][reps];
  for (int rep = 0; rep < reps; rep++)
    for (int v = 0; v < NMUL + NX7; v++) {
      hipEventRecord(a);
      launch(kern[v], blocks, threads, lds, d[v]);
      hipEventRecord(b);
      hipEventSynchronize(b);
      float ms = 0;
      hipEventElapsedTime(&ms, a, b);
      const double mults = (double)blocks * threads * CH * ITER, wmults = mults / 64;
      cyc[v][rep] = ms * 1e-3 * 2.4e9 * 1024 / wmults;
    }
  // the first repeats bring the clocks up; the spread is max - min of the others
  for (int v = 0; v < NMUL + NX7; v++) {
    double lo = cyc[v][warm], hi = cyc[v][warm];
    for (int rep = warm + 1; rep < reps; rep++) { lo = cyc[v][rep] < lo ? cyc[v][rep] : lo; hi = cyc[v][rep] > hi ? cyc[v][rep] : hi; }
    printf("%-10s %6.2f cycles per wave-multiply per SIMD @2.4GHz (min of %d repeats, spread %.2f)\n", v < NMUL ? MUL_NAME[v] : X7_NAME[v - NMUL], lo, reps - warm, hi - lo);
  }
  for (int v = 0; v < NMUL + NX7; v++) hipMemcpy(h[v].data(), d[v], h[v].size() * 8, hipMemcpyDeviceToHost);
  size_t bad = 0;
  for (size_t i = 0; i < h[0].size(); i++) {
    for (int v = 1; v < NMUL; v++) bad += h[0][i] != h[v][i];
    for (int v = 1; v < NX7; v++) bad += h[NMUL][i] != h[NMUL + v][i];
  }
  printf("results %s (%zu differ; %zu lanes)\n", bad ? "DIFFER" : "equal", bad, h[0].size());
  return bad != 0;
}
