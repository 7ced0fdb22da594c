// One two_to_one_sha256, from its 16 message words to every cell of its 310 rows (lcp2_sha256_witness), and one scattered cell
// (lcp2_scatter_cells).
//
// The lanes of the two SHA-256 witness kernels as functions: sha_job_record is the lane of k_sha_jobs_level (message gather, then
// sha_words_record: both compressions, the 336-word record of sha_layout.hpp; k_sha_plan_jobs and sha_plan.hpp share the latter), sha_row_cells the lane of k_sha_fill_rows (one circuit row of the record
// as (column, value) pairs through a store callback), sha_jobs_problem the validation lcp2_sha256_witness (witness_rows.hip) runs
// on the host before anything is launched.  kernels_witness.hip calls the lanes with stores into the column-major witness
// matrix; tests/emu/emu_sha.cpp compiles the same text for the CPU and runs the grids as loops.  The row layout is the one of
// host/gates.cpp (prog_sha_*) and host/builder.cpp (two_to_one_sha256); tests/sha_rows_ref.py states it over Python integers.
// The K / IV / padding-schedule tables are __constant__ on the device and plain constants on the CPU; the lanes are device
// functions under hipcc (they read those tables), the validation is host code everywhere.
#pragma once
#include <stddef.h>
#include "gl64.hpp"
#include "sha_layout.hpp"

#if defined(__HIPCC__)
#define LCP2_SHA_TABLE static __device__ __constant__
#define LCP2_SHA_LANE __device__ __forceinline__
#else
#define LCP2_SHA_TABLE static const
#define LCP2_SHA_LANE inline
#endif

namespace lcp2 {

LCP2_SHA_TABLE uint32_t WSHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
LCP2_SHA_TABLE uint32_t WSHA_IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
// message schedule of the constant padding block (0x80000000, 0, ..., 0, 512) of a 64-byte message
LCP2_SHA_TABLE uint32_t WSHA_PAD_W[64] = {0x80000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000000, 0x00000200, 0x80000000, 0x01400000, 0x00205000, 0x00005088, 0x22000800, 0x22550014, 0x05089742, 0xa0000020, 0x5a880000, 0x005c9400, 0x0016d49d, 0xfa801f00, 0xd33225d0, 0x11675959, 0xf6e6bfda, 0xb30c1549, 0x08b2b050, 0x9d7c4c27, 0x0ce2a393, 0x88e6e1ea, 0xa52b4335, 0x67a16f49, 0xd732016f, 0x4eeb2e91, 0x5dbf55e5, 0x8eee2335, 0xe2bc5ec2, 0xa83f4394, 0x45ad78f7, 0x36f3d0cd, 0xd99c05e8, 0xb0511dc7, 0x69bc7ac4, 0xbd11375b, 0xe3ba71e5, 0x3b209ff2, 0x18feee17, 0xe25ad9e7, 0x13375046, 0x0515089d, 0x4f0d0f04, 0x2627484e, 0x310128d2, 0xc668b434, 0x420841cc, 0x62d311b8, 0xe59ba771, 0x85a7a484};

LCP2_SHA_LANE uint32_t wrotr(uint32_t x, int r) {  // 0 < r < 32
#if defined(__HIPCC__)
  return __builtin_rotateright32(x, r);
#else
  return (x >> r) | (x << (32 - r));
#endif
}

// ------------------------------------------------------------------ validation (host, before any launch)
constexpr u32 SHA_OK = 0, SHA_LEVELS_DO_NOT_COVER = 1, SHA_LEVELS_NOT_MONOTONE = 2, SHA_ROWS_OUT_OF_RANGE = 3, SHA_BAD_SOURCE = 4,
              SHA_NO_LEVELS = 5;
struct ShaProblem {
  u32 problem;  // SHA_OK: the kernels can neither read nor write out of range
  u32 job;      // the job that was refused (SHA_ROWS_OUT_OF_RANGE, SHA_BAD_SOURCE), else the level, else 0
};
inline const char *sha_problem_str(u32 problem) {
  switch (problem) {
    case SHA_LEVELS_DO_NOT_COVER: return "sha witness: level table does not cover the jobs";
    case SHA_LEVELS_NOT_MONOTONE: return "sha witness: level table not monotone";
    case SHA_ROWS_OUT_OF_RANGE: return "sha witness: rows out of range";
    case SHA_BAD_SOURCE: return "sha witness: bad message source";
    case SHA_NO_LEVELS: return "sha witness: jobs without levels";
    default: return "ok";
  }
}
// level_start: nlevels + 1 entries.  A level may be empty; a source may name a word of words_in or a digest word of a job of ANY
// earlier level.  A table entry above njobs is reported as not monotone (the last entry is njobs) before a job behind the list is
// looked at.
inline ShaProblem sha_jobs_problem(const ShaJobDev *jobs, size_t njobs, const uint32_t *level_start, uint32_t nlevels, size_t nwords, u64 n) {
  if (njobs == 0) return {SHA_OK, 0};
  if (nlevels == 0) return {SHA_NO_LEVELS, 0};
  if (level_start[0] != 0 || level_start[nlevels] != njobs) return {SHA_LEVELS_DO_NOT_COVER, 0};
  for (uint32_t l = 0; l < nlevels; l++) {
    if (level_start[l] > level_start[l + 1] || level_start[l + 1] > njobs) return {SHA_LEVELS_NOT_MONOTONE, l};
    for (uint32_t j = level_start[l]; j < level_start[l + 1]; j++) {
      if ((u64)jobs[j].first_row + SHA_ROWS > n) return {SHA_ROWS_OUT_OF_RANGE, j};
      for (int i = 0; i < 16; i++) {
        const int32_t s = jobs[j].in_src[i];
        if (s >= 0 ? (size_t)s >= nwords : (uint32_t)((~s) >> 3) >= level_start[l]) return {SHA_BAD_SOURCE, j};
      }
    }
  }
  return {SHA_OK, 0};
}

// ------------------------------------------------------------------ the lane of k_sha_jobs_level
// From 16 message words to the whole record R (SHA_REC_WORDS words): the compression of the data block and of the constant padding
// block.  msg may be R + SHA_REC_IN itself (k_sha_plan_jobs gathers the words into the record first): every word is read before
// the first store.
LCP2_SHA_LANE void sha_words_record(const uint32_t *msg, uint32_t *R) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = msg[i];
#pragma unroll
  for (int i = 0; i < 16; i++) R[SHA_REC_IN + i] = w[i];
  uint32_t chain[8];
#pragma unroll
  for (int i = 0; i < 8; i++) chain[i] = WSHA_IV[i];
  for (int c = 0; c < 2; c++) {
    uint32_t a = chain[0], b = chain[1], cc = chain[2], d = chain[3], e = chain[4], f = chain[5], g = chain[6], h = chain[7];
    if (c == 1) {
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = 0;
      w[0] = 0x80000000u; w[15] = 512;
    }
    uint32_t *AE = R + (c == 0 ? SHA_REC_AE0 : SHA_REC_AE1);
#pragma unroll 1
    for (int t0 = 0; t0 < 64; t0 += 16) {
#pragma unroll
     for (int ti = 0; ti < 16; ti++) {
      const int t = t0 + ti;
      uint32_t wt;
      if (t0 == 0) wt = w[ti];
      else {
        uint32_t w15 = w[(ti + 1) & 15], w2 = w[(ti + 14) & 15];
        uint32_t s0 = wrotr(w15, 7) ^ wrotr(w15, 18) ^ (w15 >> 3), s1 = wrotr(w2, 17) ^ wrotr(w2, 19) ^ (w2 >> 10);
        wt = w[ti] + s0 + w[(ti + 9) & 15] + s1;
        w[ti] = wt;
        if (c == 0) R[SHA_REC_SCHED + t - 16] = wt;
      }
      uint32_t S1 = wrotr(e, 6) ^ wrotr(e, 11) ^ wrotr(e, 25), ch = (e & f) ^ (~e & g);
      uint32_t t1 = h + S1 + ch + WSHA_K[t] + wt;
      uint32_t S0 = wrotr(a, 2) ^ wrotr(a, 13) ^ wrotr(a, 22), mj = (a & b) ^ (a & cc) ^ (b & cc);
      h = g; g = f; f = e; e = d + t1; d = cc; cc = b; b = a; a = t1 + S0 + mj;
      AE[2 * t] = a; AE[2 * t + 1] = e;
     }
    }
    chain[0] += a; chain[1] += b; chain[2] += cc; chain[3] += d; chain[4] += e; chain[5] += f; chain[6] += g; chain[7] += h;
    uint32_t *O = R + (c == 0 ? SHA_REC_MID : SHA_REC_DIGEST);
#pragma unroll
    for (int i = 0; i < 8; i++) O[i] = chain[i];
  }
}
// Job j of a level: gathers its 16 message words (words_in, or digests in the records of jobs of earlier levels) and writes
// record j of `rec` from them (sha_words_record).
LCP2_SHA_LANE void sha_job_record(const ShaJobDev &job, u32 j, const uint32_t *words_in, uint32_t *rec) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    int s = job.in_src[i];
    w[i] = s >= 0 ? words_in[s] : rec[(u64)((~s) >> 3) * SHA_REC_WORDS + SHA_REC_DIGEST + ((~s) & 7)];
  }
  sha_words_record(w, rec + (u64)j * SHA_REC_WORDS);
}

// state word helpers on a record: a_t / e_t = register a / e AFTER round t of compression c; negative t = chaining input
LCP2_SHA_LANE uint32_t rec_a(const uint32_t *R, int c, int t) {
  if (t >= 0) return R[(c == 0 ? SHA_REC_AE0 : SHA_REC_AE1) + 2 * t];
  return c == 0 ? WSHA_IV[-1 - t] : R[SHA_REC_MID + (-1 - t)];  // t = -1 -> a, -2 -> b, -3 -> c, -4 -> d
}
LCP2_SHA_LANE uint32_t rec_e(const uint32_t *R, int c, int t) {
  if (t >= 0) return R[(c == 0 ? SHA_REC_AE0 : SHA_REC_AE1) + 2 * t + 1];
  return c == 0 ? WSHA_IV[4 + (-1 - t)] : R[SHA_REC_MID + 4 + (-1 - t)];
}

// ------------------------------------------------------------------ the lane of k_sha_fill_rows
// Row lr (0 .. SHA_ROWS - 1) of the hash whose record is R: put(column, value) for EVERY column 0 .. SHA_ROW_COLUMNS - 1 (unused
// ones with 0), so a reused witness buffer needs no clearing; nothing else is written.
constexpr u32 SHA_ROW_COLUMNS = 108;
template <class Put>
LCP2_SHA_LANE void sha_row_cells(const uint32_t *R, u32 lr, Put put) {
  auto bits = [&](u32 base, uint32_t x) {
    for (int i = 0; i < 32; i++) put(base + i, (x >> i) & 1);
  };
  auto msg = [&](int t) -> uint32_t { return t < 16 ? R[SHA_REC_IN + t] : R[SHA_REC_SCHED + t - 16]; };
  if (lr < SHA_ROW_ROUNDS0) {  // schedule row for W_t, t = 16 + lr
    const int t = 16 + (int)lr;
    uint32_t w2 = msg(t - 2), w7 = msg(t - 7), w15 = msg(t - 15), w16 = msg(t - 16);
    uint32_t s0 = wrotr(w15, 7) ^ wrotr(w15, 18) ^ (w15 >> 3), s1 = wrotr(w2, 17) ^ wrotr(w2, 19) ^ (w2 >> 10);
    u64 sum = (u64)s1 + w7 + s0 + w16;
    put(0, w2); put(1, w7); put(2, w15); put(3, w16); put(4, (uint32_t)sum); put(5, 0); put(6, 0); put(7, 0);
    bits(8, w2); bits(40, w15);
    for (u32 c = 72; c < 104; c++) put(c, 0);
    put(104, (sum >> 32) & 1); put(105, (sum >> 33) & 1); put(106, 0); put(107, 0);
    return;
  }
  u32 q = lr - SHA_ROW_ROUNDS0;
  int c = 0;
  if (q >= 128 + 3) { q -= 128 + 3; c = 1; }
  if (q < 128) {
    const int t = (int)(q >> 1);
    if ((q & 1) == 0) {  // round E row
      uint32_t e = rec_e(R, c, t - 1), f = rec_e(R, c, t - 2), g = rec_e(R, c, t - 3), h = rec_e(R, c, t - 4), d = rec_a(R, c, t - 4);
      uint32_t wv = c == 0 ? msg(t) : 0;
      u64 kw = WSHA_K[t];
      if (c == 1) kw += WSHA_PAD_W[t];
      uint32_t S1 = wrotr(e, 6) ^ wrotr(e, 11) ^ wrotr(e, 25), ch = (e & f) ^ (~e & g);
      u64 sum1 = (u64)h + S1 + ch + kw + wv;
      uint32_t t1 = (uint32_t)sum1;
      u64 sume = (u64)d + t1;
      put(0, e); put(1, f); put(2, g); put(3, h); put(4, d); put(5, wv); put(6, (uint32_t)sume); put(7, t1);
      bits(8, e); bits(40, f); bits(72, g);
      u64 k1 = sum1 >> 32;
      put(104, k1 & 1); put(105, (k1 >> 1) & 1); put(106, (k1 >> 2) & 1); put(107, sume >> 32);
    } else {  // round A row
      uint32_t a = rec_a(R, c, t - 1), b = rec_a(R, c, t - 2), cc = rec_a(R, c, t - 3);
      // t1 of this round = a_t - S0(a) - Maj(a,b,c)  (mod 2^32)
      uint32_t S0 = wrotr(a, 2) ^ wrotr(a, 13) ^ wrotr(a, 22), mj = (a & b) ^ (a & cc) ^ (b & cc);
      uint32_t a_new = rec_a(R, c, t);
      uint32_t t1 = a_new - S0 - mj;
      u64 suma = (u64)t1 + S0 + mj;
      put(0, a); put(1, b); put(2, cc); put(3, t1); put(4, a_new); put(5, 0); put(6, 0); put(7, 0);
      bits(8, a); bits(40, b); bits(72, cc);
      u64 k2 = suma >> 32;
      put(104, k2 & 1); put(105, (k2 >> 1) & 1); put(106, 0); put(107, 0);
    }
    return;
  }
  // addition rows: out_i = chain_i + state_i, three per row
  const u32 ar = q - 128;
  for (u32 col = 0; col < SHA_ROW_COLUMNS; col++) put(col, 0);
  for (int jj = 0; jj < 3; jj++) {
    int i = (int)ar * 3 + jj;
    if (i >= 8) break;
    uint32_t chain = c == 0 ? WSHA_IV[i] : R[SHA_REC_MID + i];
    uint32_t st = i < 4 ? rec_a(R, c, 63 - i) : rec_e(R, c, 63 - (i - 4));
    u64 sum = (u64)chain + st;
    put(3 * jj, chain); put(3 * jj + 1, st); put(3 * jj + 2, (uint32_t)sum);
    bits(9 + 33 * jj, (uint32_t)sum);
    put(9 + 33 * jj + 32, sum >> 32);
  }
}

// ------------------------------------------------------------------ lcp2_scatter_cells
// the index of the first cell whose row is not below n, ncells when there is none; the column is the caller's duty (the call does
// not know how many columns the matrix has)
inline size_t scatter_cells_problem(const CellDev *cells, size_t ncells, u64 n) {
  for (size_t i = 0; i < ncells; i++)
    if (cells[i].row >= n) return i;
  return ncells;
}
// the lane of k_scatter_cells: the value as given, canonical or not
LCP2_HD void scatter_cell_lane(const CellDev *__restrict__ cells, u64 ncells, u64 i, u64 *__restrict__ wires, u64 n) {
  if (i >= ncells) return;
  const CellDev c = cells[i];
  wires[(u64)c.col * n + c.row] = c.value;
}

}  // namespace lcp2
