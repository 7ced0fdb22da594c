// Prover kernels K5, K7 - K9 for gfx950 (rows a7 - a13 of SURVEY.md section 8) and the small utilities; K6, the quotient, is
// kernels_quotient.hip (+ kernels_gates_*.hip).
//
//  K5  k_perm_chunks / scan / k_perm_finalize   wires_permutation_partial_products_and_zs  (plonk/prover.rs)
//  K7  k_eval_polys / k_compose / k_divide_*     OpeningSet::new, PolynomialBatch::prove_openings (fri/oracle.rs)
//  K8  k_fri_fold (+ NTT, hash kernels)          fri_committed_trees (fri/prover.rs)
//  K9  k_pow_search                              fri_proof_of_work, deterministic minimum witness
//
// Every kernel indexes the LDE matrices in their storage (= Merkle leaf) order, so all column reads are coalesced 512-byte runs per wave.
#include "internal.hpp"
#include "poseidon.hpp"
#include "prover_kernels.hpp"

namespace lcp2 {

// ------------------------------------------------------------------ generic exclusive scan (field add / mul)
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;

template <bool MUL> __device__ __forceinline__ u64 scan_op(u64 a, u64 b) { return MUL ? gl_mul(a, b) : gl_add(a, b); }
template <bool MUL> __device__ __forceinline__ u64 scan_id() { return MUL ? 1 : 0; }

// out[i] = op over logical predecessors of i (exclusive); logical index = reverse ? n-1-i : i; batch = blockIdx.y
template <bool MUL>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_block(const u64 *__restrict__ in, u64 *__restrict__ out, u64 *__restrict__ block_tot,
                                                             u64 n, int reverse, u64 batch_stride, u64 nblocks) {
  __shared__ u64 sh[SCAN_THREADS];
  const u64 *src = in + blockIdx.y * batch_stride;
  u64 *dst = out + blockIdx.y * batch_stride;
  u64 base = (u64)blockIdx.x * SCAN_BLOCK + (u64)threadIdx.x * SCAN_ITEMS;
  u64 v[SCAN_ITEMS];
  u64 run = scan_id<MUL>();
#pragma unroll
  for (int e = 0; e < SCAN_ITEMS; e++) {
    u64 li = base + e;
    u64 x = scan_id<MUL>();
    if (li < n) x = src[reverse ? n - 1 - li : li];
    v[e] = run;  // exclusive inside the thread
    run = scan_op<MUL>(run, x);
  }
  sh[threadIdx.x] = run;
  __syncthreads();
  // Hillis-Steele inclusive scan of the 256 thread totals
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {
    u64 t = sh[threadIdx.x];
    u64 o = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : scan_id<MUL>();
    __syncthreads();
    sh[threadIdx.x] = scan_op<MUL>(o, t);
    __syncthreads();
  }
  u64 prefix = threadIdx.x ? sh[threadIdx.x - 1] : scan_id<MUL>();
#pragma unroll
  for (int e = 0; e < SCAN_ITEMS; e++) {
    u64 li = base + e;
    if (li < n) dst[reverse ? n - 1 - li : li] = scan_op<MUL>(prefix, v[e]);
  }
  if (threadIdx.x == SCAN_THREADS - 1) block_tot[blockIdx.y * nblocks + blockIdx.x] = sh[SCAN_THREADS - 1];
}
// exclusive scan of the block totals, one workgroup per batch (sequential over 256-wide tiles)
template <bool MUL>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_totals(u64 *__restrict__ block_tot, u64 nblocks) {
  __shared__ u64 sh[SCAN_THREADS];
  u64 *t = block_tot + blockIdx.x * nblocks;
  u64 carry = scan_id<MUL>();
  for (u64 base = 0; base < nblocks; base += SCAN_THREADS) {
    u64 i = base + threadIdx.x;
    u64 x = i < nblocks ? t[i] : scan_id<MUL>();
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
      u64 cur = sh[threadIdx.x];
      u64 o = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : scan_id<MUL>();
      __syncthreads();
      sh[threadIdx.x] = scan_op<MUL>(o, cur);
      __syncthreads();
    }
    u64 excl = threadIdx.x ? sh[threadIdx.x - 1] : scan_id<MUL>();
    u64 total = sh[SCAN_THREADS - 1];
    if (i < nblocks) t[i] = scan_op<MUL>(carry, excl);
    carry = scan_op<MUL>(carry, total);
    __syncthreads();
  }
}
template <bool MUL>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(u64 *__restrict__ out, const u64 *__restrict__ block_tot, u64 n, int reverse,
                                                             u64 batch_stride, u64 nblocks) {
  u64 *dst = out + blockIdx.y * batch_stride;
  u64 pre = block_tot[blockIdx.y * nblocks + blockIdx.x];
  u64 base = (u64)blockIdx.x * SCAN_BLOCK;
  for (u32 e = threadIdx.x; e < SCAN_BLOCK; e += SCAN_THREADS) {
    u64 li = base + e;
    if (li < n) { u64 ph = reverse ? n - 1 - li : li; dst[ph] = scan_op<MUL>(pre, dst[ph]); }
  }
}

void launch_scan(hipStream_t s, bool mul, const u64 *in, u64 *out, u64 *block_tot, u64 n, bool reverse, u32 batches, u64 batch_stride) {
  u64 nblocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  dim3 grid((unsigned)nblocks, batches);
  if (mul) {
    hipLaunchKernelGGL(k_scan_block<true>, grid, dim3(SCAN_THREADS), 0, s, in, out, block_tot, n, (int)reverse, batch_stride, nblocks);
    hipLaunchKernelGGL(k_scan_totals<true>, dim3(batches), dim3(SCAN_THREADS), 0, s, block_tot, nblocks);
    hipLaunchKernelGGL(k_scan_apply<true>, grid, dim3(SCAN_THREADS), 0, s, out, block_tot, n, (int)reverse, batch_stride, nblocks);
  } else {
    hipLaunchKernelGGL(k_scan_block<false>, grid, dim3(SCAN_THREADS), 0, s, in, out, block_tot, n, (int)reverse, batch_stride, nblocks);
    hipLaunchKernelGGL(k_scan_totals<false>, dim3(batches), dim3(SCAN_THREADS), 0, s, block_tot, nblocks);
    hipLaunchKernelGGL(k_scan_apply<false>, grid, dim3(SCAN_THREADS), 0, s, out, block_tot, n, (int)reverse, batch_stride, nblocks);
  }
}
u64 scan_scratch_words(u64 n, u32 batches) { return ((n + SCAN_BLOCK - 1) / SCAN_BLOCK) * batches; }

// ------------------------------------------------------------------ K5: permutation argument on H
// One thread per (row, challenge): the NCHUNK quotient-chunk products  prod_j num_j / den_j  and their product.
__global__ __launch_bounds__(256) void k_perm_chunks(PermArgs a) {
  u32 rb = blockIdx.x, ch = blockIdx.y;
  if (gridDim.x % 8 == 0) {
    // XCD-aware mapping (speed only; blocks b and b + 8 share an XCD's L2): the challenges of one row block run back to back on
    // one XCD, so the wires and sigmas they both read come from HBM once
    const u32 lin = blockIdx.x + gridDim.x * blockIdx.y, x = lin & 7, j = lin >> 3;
    ch = j % gridDim.y;
    rb = (j / gridDim.y) * 8 + x;
  }
  u64 row = (u64)rb * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  const u64 beta = a.betas[ch], gamma = a.gammas[ch];
  u64 x = two_level(a.subgroup, a.row0 + row);
  u64 bx = gl_mul(beta, x);
  u64 pn[PERM_MAX_CHUNKS], pd[PERM_MAX_CHUNKS];
#pragma unroll
  for (u32 k = 0; k < PERM_MAX_CHUNKS; k++) {
    pn[k] = 1; pd[k] = 1;
    if (k < a.nchunks) {
      for (u32 j = k * a.chunk; j < a.num_routed && j < (k + 1) * a.chunk; j++) {
        u64 w = gl_canon(a.wires[(u64)j * a.wires_stride + row]);
        u64 wg = gl_add(w, gamma);
        // lazy through the products (any u64 congruent to the element); the batch inversion below multiplies canonically
        pn[k] = gl_mul_nc(pn[k], gl_add_nc(gl_mul_nc(bx, a.k_is[j]), wg));
        pd[k] = gl_mul_nc(pd[k], gl_add_nc(gl_mul_nc(beta, a.sigmas[(u64)j * a.sigma_stride + row]), wg));
      }
    }
  }
  // Montgomery batch inversion of the chunk denominators
  u64 pre[PERM_MAX_CHUNKS];
  u64 acc = 1;
#pragma unroll
  for (u32 k = 0; k < PERM_MAX_CHUNKS; k++) { pre[k] = acc; acc = gl_mul(acc, pd[k]); }
  u64 inv = gl_inv(acc);
  u64 tot = 1;
#pragma unroll
  for (int k = PERM_MAX_CHUNKS - 1; k >= 0; k--) {
    u64 dinv = gl_mul(inv, pre[k]);
    inv = gl_mul(inv, pd[k]);
    pn[k] = gl_mul(pn[k], dinv);  // quotient chunk product
  }
#pragma unroll
  for (u32 k = 0; k < PERM_MAX_CHUNKS; k++)
    if (k < a.nchunks) { a.chunk_q[((u64)ch * a.nchunks + k) * a.n + row] = pn[k]; tot = gl_mul(tot, pn[k]); }
  a.row_tot[(u64)ch * a.n + row] = tot;
}
// Z (exclusive prefix product of the row totals) is in zs[ch]; partial products pp_k = Z * q_0 .. q_k
__global__ __launch_bounds__(256) void k_perm_finalize(PermArgs a) {
  u64 row = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  u32 ch = blockIdx.y;
  if (row >= a.n) return;
  u64 acc = a.zs_out[(u64)ch * a.n + row];
  if (a.prefix) {
    acc = gl_mul(acc, a.prefix[ch]);
    a.zs_out[(u64)ch * a.n + row] = acc;
  }
  u32 npp = a.nchunks - 1;
  for (u32 k = 0; k < npp; k++) {
    acc = gl_mul(acc, a.chunk_q[((u64)ch * a.nchunks + k) * a.n + row]);
    a.zs_out[((u64)a.num_challenges + (u64)ch * npp + k) * a.n + row] = acc;
  }
}

void launch_perm_chunks(hipStream_t s, const PermArgs &a) {
  hipLaunchKernelGGL(k_perm_chunks, dim3((unsigned)((a.n + 255) / 256), a.num_challenges), dim3(256), 0, s, a);
}
void launch_perm_finalize(hipStream_t s, const PermArgs &a) {
  hipLaunchKernelGGL(k_perm_finalize, dim3((unsigned)((a.n + 255) / 256), a.num_challenges), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ K7a: evaluate coefficient polynomials at an extension point
// grid (chunks, polys); a chunk is EVAL_CHUNK coefficients; thread t owns coefficients t, t+256, ...
// partial[poly][chunk] = z^(chunk*EVAL_CHUNK) * sum_t z^t * Horner_m(c[t + 256 m]; z^256)
__global__ __launch_bounds__(256) void k_eval_polys(EvalArgs a) {
  __shared__ u64 sh0[256], sh1[256];
  const u32 t = threadIdx.x, chunk = blockIdx.x, poly = blockIdx.y;
  const u64 *c = a.coeffs + (u64)poly * a.col_stride + (u64)chunk * a.chunk_len;
  // Horner in lazy arithmetic: acc = acc * z^256 + c with acc any u64 pair congruent to the value (gl_mul_nc takes it), one
  // canonical product per component so that gl_add_nc has its canonical operand, and 7 z_1 hoisted out of the loop
  gl2 acc = gl2_make(0, 0);
  const u64 z0 = a.zstep[0], z1 = a.zstep[1], z1w = gl_mul(GL_W, z1);
  for (int m = (int)a.items - 1; m >= 0; m--) {
    u32 idx = t + 256u * (u32)m;
    const u64 coeff = idx < a.chunk_len ? c[idx] : 0;  // canonical: the coefficient buffers are the library's own
    const u64 n0 = gl_add_nc(gl_add_nc(gl_mul_nc(acc.c0, z0), gl_mul(acc.c1, z1w)), coeff);
    const u64 n1 = gl_add_nc(gl_mul_nc(acc.c0, z1), gl_mul(acc.c1, z0));
    acc = gl2_make(n0, n1);
  }
  acc = gl2_mul(gl2_make(gl_canon(acc.c0), gl_canon(acc.c1)), gl2_make(a.zpow_t[2 * t], a.zpow_t[2 * t + 1]));
  sh0[t] = acc.c0; sh1[t] = acc.c1;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < (u32)off) { sh0[t] = gl_add(sh0[t], sh0[t + off]); sh1[t] = gl_add(sh1[t], sh1[t + off]); }
    __syncthreads();
  }
  if (t == 0) {
    gl2 r = gl2_mul(gl2_make(sh0[0], sh1[0]), gl2_make(a.zpow_chunk[2 * chunk], a.zpow_chunk[2 * chunk + 1]));
    a.partial[2 * ((u64)poly * a.nchunks + chunk)] = r.c0;
    a.partial[2 * ((u64)poly * a.nchunks + chunk) + 1] = r.c1;
  }
}
__global__ void k_eval_reduce(const u64 *__restrict__ partial, u32 nchunks, u32 npolys, u64 *__restrict__ out) {
  u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npolys) return;
  gl2 s = gl2_make(0, 0);
  for (u32 k = 0; k < nchunks; k++) s = gl2_add(s, gl2_make(partial[2 * ((u64)p * nchunks + k)], partial[2 * ((u64)p * nchunks + k) + 1]));
  out[2 * p] = s.c0; out[2 * p + 1] = s.c1;
}
void launch_eval_polys(hipStream_t s, const EvalArgs &a, u32 npolys, u64 *out) {
  hipLaunchKernelGGL(k_eval_polys, dim3(a.nchunks, npolys), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_eval_reduce, dim3((npolys + 63) / 64), dim3(64), 0, s, a.partial, a.nchunks, npolys, out);
}

// ------------------------------------------------------------------ K7b: composition polynomial and division by (X - z)
// t0_i = (sum_j alpha^j f_j[i]) * zeta^i over every committed polynomial, t1_i = (sum_{j<CH} alpha^j Z_j[i]) * (g zeta)^i
// planes: [t0.c0, t0.c1, t1.c0, t1.c1][n]
__global__ __launch_bounds__(256) void k_compose(ComposeArgs a) {
  u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  gl2 f0 = gl2_make(0, 0);
  u32 j = 0;
  for (u32 o = 0; o < 4; o++) {
    const u64 *cf = a.coeffs[o];
    for (u32 c = 0; c < a.ncols[o]; c++, j++) {
      u64 v = cf[(u64)c * a.n + i];
      f0.c0 = gl_add(f0.c0, gl_mul(a.alpha_pows[2 * j], v));
      f0.c1 = gl_add(f0.c1, gl_mul(a.alpha_pows[2 * j + 1], v));
    }
  }
  gl2 f1 = gl2_make(0, 0);
  for (u32 c = 0; c < a.num_challenges; c++) {
    u64 v = a.coeffs[2][(u64)c * a.n + i];
    f1.c0 = gl_add(f1.c0, gl_mul(a.alpha_pows[2 * c], v));
    f1.c1 = gl_add(f1.c1, gl_mul(a.alpha_pows[2 * c + 1], v));
  }
  gl2 z0 = gl2_mul(gl2_make(a.z0_lo[2 * (i & a.zmask)], a.z0_lo[2 * (i & a.zmask) + 1]), gl2_make(a.z0_hi[2 * (i >> a.zh)], a.z0_hi[2 * (i >> a.zh) + 1]));
  gl2 z1 = gl2_mul(gl2_make(a.z1_lo[2 * (i & a.zmask)], a.z1_lo[2 * (i & a.zmask) + 1]), gl2_make(a.z1_hi[2 * (i >> a.zh)], a.z1_hi[2 * (i >> a.zh) + 1]));
  gl2 t0 = gl2_mul(f0, z0), t1 = gl2_mul(f1, z1);
  a.planes[i] = t0.c0; a.planes[a.n + i] = t0.c1; a.planes[2 * a.n + i] = t1.c0; a.planes[3 * a.n + i] = t1.c1;
}
// planes now hold the exclusive suffix sums S_{i+1}; final_i = alpha^CH * zeta^-(i+1) S0_{i+1} + (g zeta)^-(i+1) S1_{i+1}
__global__ __launch_bounds__(256) void k_divide_finalize(ComposeArgs a, u64 *__restrict__ out0, u64 *__restrict__ out1) {
  u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  u64 e = i + 1;  // <= n; the inverse tables cover n+1 exponents through the hi table
  gl2 zi0 = gl2_mul(gl2_make(a.zi0_lo[2 * (e & a.zmask)], a.zi0_lo[2 * (e & a.zmask) + 1]), gl2_make(a.zi0_hi[2 * (e >> a.zh)], a.zi0_hi[2 * (e >> a.zh) + 1]));
  gl2 zi1 = gl2_mul(gl2_make(a.zi1_lo[2 * (e & a.zmask)], a.zi1_lo[2 * (e & a.zmask) + 1]), gl2_make(a.zi1_hi[2 * (e >> a.zh)], a.zi1_hi[2 * (e >> a.zh) + 1]));
  gl2 s0 = gl2_make(a.planes[i], a.planes[a.n + i]), s1 = gl2_make(a.planes[2 * a.n + i], a.planes[3 * a.n + i]);
  gl2 q0 = gl2_mul(gl2_mul(s0, zi0), gl2_make(a.alpha_shift[0], a.alpha_shift[1]));
  gl2 q1 = gl2_mul(s1, zi1);
  gl2 r = gl2_add(q0, q1);
  out0[i] = r.c0; out1[i] = r.c1;
}
void launch_compose(hipStream_t s, const ComposeArgs &a) {
  hipLaunchKernelGGL(k_compose, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_divide_finalize(hipStream_t s, const ComposeArgs &a, u64 *out0, u64 *out1) {
  hipLaunchKernelGGL(k_divide_finalize, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, out0, out1);
}

// ------------------------------------------------------------------ K8: FRI fold  new[k] = sum_j beta^j c[arity k + j]
__global__ __launch_bounds__(256) void k_fri_fold(const u64 *__restrict__ c0, const u64 *__restrict__ c1, u64 *__restrict__ o0,
                                                   u64 *__restrict__ o1, u64 nout, u32 arity, u64 b0, u64 b1) {
  u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nout) return;
  const gl2 beta = gl2_make(b0, b1);
  gl2 acc = gl2_make(0, 0);
  for (int j = (int)arity - 1; j >= 0; j--) acc = gl2_add(gl2_mul(acc, beta), gl2_make(c0[k * arity + j], c1[k * arity + j]));
  o0[k] = acc.c0; o1[k] = acc.c1;
}
void launch_fri_fold(hipStream_t s, const u64 *c0, const u64 *c1, u64 *o0, u64 *o1, u64 nout, u32 arity, u64 b0, u64 b1) {
  hipLaunchKernelGGL(k_fri_fold, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, c0, c1, o0, o1, nout, arity, b0, b1);
}
// FRI query: out[q][2j + e] = plane_e[leaf * arity + j]
__global__ void k_gather_ext_leaves(const u64 *__restrict__ p0, const u64 *__restrict__ p1, u32 arity, const u64 *__restrict__ leaf_idx,
                                    u32 k, u64 *__restrict__ out) {
  u32 q = blockIdx.x;
  if (q >= k) return;
  u64 leaf = leaf_idx[q];
  for (u32 t = threadIdx.x; t < 2 * arity; t += blockDim.x) out[(u64)q * 2 * arity + t] = (t & 1 ? p1 : p0)[leaf * arity + (t >> 1)];
}
void launch_gather_ext_leaves(hipStream_t s, const u64 *p0, const u64 *p1, u32 arity, const u64 *leaf_idx, u32 k, u64 *out) {
  if (!k) return;
  hipLaunchKernelGGL(k_gather_ext_leaves, dim3(k), dim3(64), 0, s, p0, p1, arity, leaf_idx, k, out);
}

// ------------------------------------------------------------------ K9: proof of work (minimum witness)
__global__ __launch_bounds__(256) void k_pow_search(PowArgs a) {
  u64 w = a.start + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  u64 s[12];
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = a.state[i];
#pragma unroll
  for (int i = 0; i < 12; i++)
    if (i == (int)a.pos) s[i] = w;
  pos_permute(s, a.rc);
  if (w < GL_P && (s[7] >> (64 - a.bits)) == 0) atomicMin((unsigned long long *)a.result, (unsigned long long)w);
}
void launch_pow_search(hipStream_t s, const PowArgs &a, u64 count) {
  hipLaunchKernelGGL(k_pow_search, dim3((unsigned)(count / 256)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ challenge-dependent setup (prover_kernels.hpp)
__global__ void k_set_words(u64 *dst, SmallWords w, u32 n) {
  if (threadIdx.x < n) dst[threadIdx.x] = w.v[threadIdx.x];
}
void launch_set_words(hipStream_t s, u64 *dst, const SmallWords &w, u32 n) {
  hipLaunchKernelGGL(k_set_words, dim3(1), dim3(16), 0, s, dst, w, n);
}

__global__ __launch_bounds__(256) void k_eval_tables(u64 z0, u64 z1, u32 chunk_len, u32 nchunks, u64 *tab) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  const gl2 z = gl2_make(z0, z1);
  if (t < 256) { const gl2 v = gl2_pow(z, t); tab[2 * t] = v.c0; tab[2 * t + 1] = v.c1; }
  else if (t - 256 < nchunks) { const u32 k = t - 256; const gl2 v = gl2_pow(z, (u64)chunk_len * k); tab[512 + 2 * k] = v.c0; tab[513 + 2 * k] = v.c1; }
}
void launch_eval_tables(hipStream_t s, u64 z0, u64 z1, u32 chunk_len, u32 nchunks, u64 *tab) {
  hipLaunchKernelGGL(k_eval_tables, dim3((256 + nchunks + 255) / 256), dim3(256), 0, s, z0, z1, chunk_len, nchunks, tab);
}

__global__ __launch_bounds__(256) void k_compose_tables(u64 a0, u64 a1, u64 z0, u64 z1, u64 g, u32 total_polys, u32 h, u64 hi_count, u64 *T) {
  const u64 t = (u64)blockIdx.x * 256 + threadIdx.x, per = (1ull << h) + hi_count;
  gl2 v;
  if (t < total_polys) v = gl2_pow(gl2_make(a0, a1), t);
  else {
    const u64 r = t - total_polys, b = r / per, j = r % per;
    if (b >= 4) return;
    gl2 base = gl2_make(z0, z1);
    if (b & 1) base = gl2_scale(base, g);
    if (b & 2) base = gl2_inv(base);
    v = j < (1ull << h) ? gl2_pow(base, j) : gl2_pow(base, (j - (1ull << h)) << h);
  }
  T[2 * t] = v.c0; T[2 * t + 1] = v.c1;
}
void launch_compose_tables(hipStream_t s, u64 a0, u64 a1, u64 z0, u64 z1, u64 g, u32 total_polys, u32 h, u64 hi_count, u64 *T) {
  const u64 entries = total_polys + 4 * ((1ull << h) + hi_count);
  hipLaunchKernelGGL(k_compose_tables, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, a0, a1, z0, z1, g, total_polys, h, hi_count, T);
}

__global__ void k_fill(u64 *p, u64 n, u64 v) {
  u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
void launch_fill(hipStream_t s, u64 *p, u64 n, u64 v) {
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

// the trim check of a quotient with Q < 2^q chunks: row blockIdx.y, a grid-stride walk over its `width` words
__global__ __launch_bounds__(256) void k_any_nonzero(const u64 *p, u64 pitch, u64 width, unsigned long long *flag) {
  const u64 *row = p + (u64)blockIdx.y * pitch;
  bool any = false;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < width; i += (u64)gridDim.x * blockDim.x) any = any || gl_canon(row[i]) != 0;
  if (any) *flag = 1;  // every writer writes the same word
}
void launch_any_nonzero(hipStream_t s, const u64 *p, u64 pitch, u64 width, u32 rows, unsigned long long *flag) {
  if (!width || !rows) return;
  const u64 want = (width + 255) / 256;
  hipLaunchKernelGGL(k_any_nonzero, dim3((unsigned)(want < 1024 ? want : 1024), rows), dim3(256), 0, s, p, pitch, width, flag);
}

}  // namespace lcp2
