// K10, second half: SHA-256 witness generation on the device (row a15 of SURVEY.md section 8).
//
// The reference fills the wires of every SHA-256 row on one host thread (plonky2's generator worklist running
// plonky2_crypto's U32 / SHA-256 generators).  Here a circuit built from the SHA-256 row layout of
// eth-lc-plonky2_amd/host/gates.cpp is filled in HBM by two kernels:
//   k_sha_jobs_level  one lane per two_to_one_sha256 of a dependency level: gathers its 16 message words (host
//                     supplied leaves or digests of earlier levels), runs both compressions and stores a 336-word
//                     record (message, schedule, per-round (a, e), chaining values)
//   k_sha_fill_rows   one lane per circuit ROW (310 per hash): expands the record into that row's cells (words, bit
//                     decompositions, carries) with column-major stores, so lanes of a wave write runs of a column
// plus k_scatter_cells for the handful of non-SHA cells (constants, arithmetic glue, public inputs), and, for a hash that is a job of
// a recorded witness plan, k_sha_plan_jobs: both steps fused, one wave per hash, the record in LDS (further down, with the other
// kernels of a plan's levels).
#include "internal.hpp"
#include "sha_layout.hpp"
#include "sha_rows.hpp"
#include "pos_rows.hpp"
#include "prover_kernels.hpp"
#include "u32_rows.hpp"
#include "rec_rows.hpp"
#include "pos_plan.hpp"
#include "u32_plan.hpp"
#include "sha_plan.hpp"

namespace lcp2 {

// One lane per two_to_one_sha256 of a dependency level (sha_rows.hpp sha_job_record: the text tests/emu/emu_sha.cpp runs on the CPU)
__global__ __launch_bounds__(64) void k_sha_jobs_level(const ShaJobDev *__restrict__ jobs, u32 first, u32 count,
                                                        const uint32_t *__restrict__ words_in, uint32_t *__restrict__ rec) {
  u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const u32 j = first + k;
  const ShaJobDev job = jobs[j];
  sha_job_record(job, j, words_in, rec);
}

// One lane per circuit row, 310 per hash (sha_rows.hpp sha_row_cells): every cell of the row, column-major stores
__global__ __launch_bounds__(256) void k_sha_fill_rows(const ShaJobDev *__restrict__ jobs, u32 njobs, const uint32_t *__restrict__ rec,
                                                        u64 *__restrict__ wires, u64 n) {
  u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (u64)njobs * SHA_ROWS) return;
  const u32 j = (u32)(gid / SHA_ROWS), lr = (u32)(gid % SHA_ROWS);
  const uint32_t *R = rec + (u64)j * SHA_REC_WORDS;
  const u64 row = (u64)jobs[j].first_row + lr;
  u64 *Wp = wires + row;
  sha_row_cells(R, lr, [&](u32 col, u64 v) { Wp[(u64)col * n] = v; });
}

__global__ void k_scatter_cells(const CellDev *__restrict__ cells, u64 ncells, u64 *__restrict__ wires, u64 n) {
  scatter_cell_lane(cells, ncells, (u64)blockIdx.x * blockDim.x + threadIdx.x, wires, n);
}

// One lane per PoseidonGate row (pos_rows.hpp pos_row_cells: the text tests/emu/emu_pos.cpp runs on the CPU and the host's
// poseidon_gate_row calls).  A few thousand rows per light-client proof (the recursive verifier's Merkle paths, its Challenger and
// the sponge over the inner proof's public inputs): canonical arithmetic throughout, speed is irrelevant here.
__global__ void k_poseidon_gate_rows(const PoseidonRowDev *__restrict__ rows, u64 nrows, u64 *__restrict__ wires, u64 n, const u64 *__restrict__ rc) {
  pos_rows_lane(rows, nrows, (u64)blockIdx.x * blockDim.x + threadIdx.x, wires, n, rc);
}
void launch_poseidon_gate_rows(hipStream_t s, const PoseidonRowDev *rows, u64 nrows, u64 *wires, u64 n, const u64 *rc) {
  if (!nrows) return;
  hipLaunchKernelGGL(k_poseidon_gate_rows, dim3((unsigned)((nrows + 63) / 64)), dim3(64), 0, s, rows, nrows, wires, n, rc);
}

// One lane per job of lcp2_u32_gate_rows: one operation of a U32Arithmetic / U32AddMany / U32Subtraction / U32RangeCheck /
// Comparison row, all of its cells (u32_rows.hpp u32_job_cells: the text tests/emu/emu_u32.cpp runs on the CPU).  Every cell is
// one 8-byte store into a column of the column-major matrix, so a store instruction of a wave is contiguous - 512 bytes, four
// whole 128-byte lines - exactly when its 64 jobs are 64 consecutive rows of one (kind, op): the order the header calls fast.
// Jobs in any other order write the same cells, one 8-byte piece of a line per lane.  Nothing is read but the job (24 bytes per
// lane, contiguous); blocks of 256 keep four waves' stores in flight per CU and a wave never mixes kinds in a sorted list, so the
// switch does not diverge except at the few boundaries between kinds.  A refused job folds its index and problem into the flag
// word (row_flag.hpp); a valid one never touches it.
constexpr u32 U32_ROWS_THREADS = 256;
__global__ __launch_bounds__(U32_ROWS_THREADS) void k_u32_gate_rows(const U32JobDev *__restrict__ jobs, u64 njobs, u64 *__restrict__ wires,
                                                                     u64 n, u64 *__restrict__ flag) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (const u32 problem = u32_rows_lane(jobs, njobs, i, wires, n)) atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(i, problem));
}
void launch_u32_gate_rows(hipStream_t s, const U32JobDev *jobs, u64 njobs, u64 *wires, u64 n, u64 *flag) {
  if (!njobs) return;
  hipLaunchKernelGGL(k_u32_gate_rows, dim3((unsigned)((njobs + U32_ROWS_THREADS - 1) / U32_ROWS_THREADS)), dim3(U32_ROWS_THREADS), 0, s,
                     jobs, njobs, wires, n, flag);
}

// One lane per job of one LEVEL of lcp2_rec_gate_rows: one operation of a recursion-gate row (rec_rows.hpp rec_job_cells: the text
// tests/emu/emu_rec.cpp runs on the CPU).  A lane reads its 16-byte job, then its operands one after the other as the per-kind
// function asks for them - an IMM operand is the 16-byte record itself, a CELL operand one more 8-byte load from the matrix - and
// writes each cell with one 8-byte store into its column; as in k_u32_gate_rows a store of a wave is contiguous when its 64 jobs
// are consecutive rows of one (kind, op).  The operands do NOT go through LDS: a lane's operand records are read once, by that
// lane alone, in order (no reuse across lanes or waves to stage for), the long kinds hold at most two extension elements between
// operands, and the records of one lane are consecutive, so the 16-byte loads of a lane walk whole cache lines; a round trip
// through LDS would add instructions and a barrier to a kernel whose long kinds are bound by 43 / 66 / 16 DEPENDENT extension
// multiplies per lane, which LDS cannot shorten.  The long kinds stay one lane per job; a sorted list keeps a wave on one kind.
// The flag word is folded with a minimum (row_flag.hpp), so it names the first refused job; lanes of a level after that job's return
// at once.
constexpr u32 REC_ROWS_THREADS = 256;
__global__ __launch_bounds__(REC_ROWS_THREADS) void k_rec_gate_rows(const RecJobDev *__restrict__ jobs, u64 base, u64 begin, u64 end,
                                                                     const RecOperandDev *__restrict__ operands, u64 noperands, u64 *wires,
                                                                     u32 ncols, u64 n, u64 *flag, int check_structure) {
  const u64 i = begin + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 problem = rec_rows_lane(jobs, base, begin, end, i, operands, noperands, wires, ncols, n, flag, check_structure != 0);
  if (problem) atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(i, problem));
}
void launch_rec_gate_rows(hipStream_t s, const RecJobDev *jobs, u64 base, u64 begin, u64 end, const RecOperandDev *operands, u64 noperands,
                          u64 *wires, u32 ncols, u64 n, u64 *flag, bool check_structure) {
  if (begin >= end) return;
  hipLaunchKernelGGL(k_rec_gate_rows, dim3((unsigned)((end - begin + REC_ROWS_THREADS - 1) / REC_ROWS_THREADS)), dim3(REC_ROWS_THREADS), 0, s,
                     jobs, base, begin, end, operands, noperands, wires, ncols, n, flag, check_structure ? 1 : 0);
}

// PoseidonGate CHAINS of one level of lcp2_witness_plan_rows (pos_plan.hpp: pos_plan_chain_lane is the one-lane reference of this
// kernel and writes the same cells).  A chain is a sequence of dependent permutations, so it is latency bound and runs in the
// lane-cooperative form of poseidon.hpp (pos_permute_coop_hooked): ONE 16-LANE GROUP PER CHAIN, four chains per wave, 16 per block;
// lane j < 12 owns state element j, lane 12 the swap flag, lanes 13..15 ride along with lane 12's operand and store nothing.
// Per row: every lane reads the 8-byte job (one address per group) and ITS operand record (16 bytes; lanes 0..11 neighbouring
// records), checks it before any index of it is used, and loads its cell (8 bytes) if it is a CELL; a PREV operand is one shuffle
// of the outputs the group kept in registers from the row before - they are never re-read from the matrix, so a chain has no
// store-then-load dependency inside the launch.  The group's verdict is a minimum over its 16 lanes in pos_plan_problem's order
// (structure by operand index, then the swap value); the swap flag is one shuffle from lane 12, the four deltas one shuffle between
// lanes j and j ^ 4; the 30 rounds take their constants from LDS.  Lane j stores input j, output j and what enters S-box j of the
// full rounds that have a wire, lane 0 the 22 partial-round values, lanes 0..3 the deltas, lane 12 the swap flag: all canonical.
// Control flow: the shuffles read only the group's own lanes, and all 16 lanes of a group enter and leave the row loop together
// (every condition that leaves it - the chain's end, a refusal - is the same in the whole group).  Groups of a wave walk chains of
// different lengths, so nothing in the row loop waits for another group: the only barrier is the one after the constants are
// staged, before the loop.  A refused row folds its job into flags[1] and the family bit into flags[0] (row_flag.hpp).
constexpr u32 PLAN_CHAIN_THREADS = 256;
__device__ __forceinline__ u64 group_read64(u32 byte_index, u64 v) {
  const u32 lo = (u32)__builtin_amdgcn_ds_bpermute((int)byte_index, (int)(u32)v), hi = (u32)__builtin_amdgcn_ds_bpermute((int)byte_index, (int)(u32)(v >> 32));
  return ((u64)hi << 32) | lo;
}
__global__ __launch_bounds__(PLAN_CHAIN_THREADS) void k_pos_plan_chains(const PosJobDev *__restrict__ jobs, u64 npos, const u32 *__restrict__ chain_ends,
                                                                         u64 chain_begin, u64 chain_end, const RecOperandDev *__restrict__ operands,
                                                                         u64 noperands, u64 *wires, u32 ncols, u64 n, const u64 *__restrict__ rc,
                                                                         u64 *flags, u64 gate, u64 marker) {
  __shared__ u64 rcs[POS_ROUNDS * POS_W];
  for (u32 i = threadIdx.x; i < POS_ROUNDS * POS_W; i += PLAN_CHAIN_THREADS) rcs[i] = rc[i];
  __syncthreads();
  const u64 t = (u64)blockIdx.x * PLAN_CHAIN_THREADS + threadIdx.x, chain = chain_begin + (t >> 4);
  const u32 j = (u32)t & 15, base = (__lane_id() - j) << 2;  // base: the byte index of the group's lane 0 for ds_bpermute
  if (chain >= chain_end) return;      // whole groups
  if ((flags[0] >> 8) < gate) return;  // a job of an earlier level was refused: this level writes nothing
  u64 begin, end;
  pos_plan_chain_range(chain_ends, chain, npos, begin, end);
  const u32 k = j < 12 ? j + 1 : 0;  // the operand this lane fetches
  u64 prev = 0;                      // output j of the row before
  for (u64 r = begin; r < end; r++) {
    const PosJobDev job = jobs[r];
    u32 problem = pos_plan_job_problem(job, noperands, n);
    RecOperandDev o = {0, 0, PLAN_IMM};
    if (!problem) {
      o = operands[(u64)job.first_operand + k];
      problem = pos_plan_operand_problem(o, k, r == begin, ncols, n);
    }
    u64 v = o.v;
    if (!problem && o.src == PLAN_CELL) v = wires[(u64)o.col * n + o.v];
    const u64 carried = group_read64(base + ((o.col & 15) << 2), prev);  // every lane shuffles; a valid PREV column is below 12
    if (o.src == PLAN_PREV) v = carried;
    v = gl_canon(v);
    if (!problem && k == 0) problem = pos_plan_swap_problem(v);
    u32 verdict = problem ? ((problem == POS_PLAN_SWAP_NOT_BOOLEAN ? POS_PLAN_OPERANDS : k) << 8 | problem) : 0xFFFFu;
#pragma unroll
    for (u32 m = 1; m < 16; m <<= 1) verdict = min(verdict, (u32)__shfl_xor((int)verdict, (int)m, 16));
    if (verdict != 0xFFFFu) {
      if (j == 0) {
        atomicMin((unsigned long long *)flags + 1, (unsigned long long)row_refusal(r, verdict & 0xFF));
        atomicMin((unsigned long long *)flags, (unsigned long long)row_refusal(marker, ROW_OTHER_FAMILY));
      }
      break;
    }
    const bool swap = __builtin_amdgcn_ds_bpermute((int)(base + (12 << 2)), (int)(u32)v) != 0;
    const u64 other = group_read64(base + ((j < 8 ? j ^ 4 : j) << 2), v);  // lanes 0..3 and 4..7 exchange their inputs
    u64 *W = wires + job.row;
    u64 s = 0;
    if (j < 12) {
      W[(u64)(POS_WIRE_INPUT + j) * n] = v;
      s = v;
      if (j < 8) {
        const u64 delta = swap ? (j < 4 ? gl_sub(other, v) : gl_sub(v, other)) : 0;
        s = j < 4 ? gl_add(v, delta) : gl_sub(v, delta);
        if (j < 4) W[(u64)(POS_WIRE_DELTA + j) * n] = delta;
      }
    } else if (j == 12) {
      W[(u64)POS_WIRE_SWAP * n] = v;
    }
    const u64 out = pos_permute_coop_hooked(s, j, rcs, [&](int round, u32 lo, u32 hi) {
      const bool first_half = round >= 1 && round < POS_FULL_HALF, second_half = round >= POS_FULL_HALF + POS_PARTIAL;
      const bool partial = round >= POS_FULL_HALF && round < POS_FULL_HALF + POS_PARTIAL;
      if (j < 12 && (first_half || second_half || (partial && j == 0))) {
        const u32 col = first_half ? POS_WIRE_FULL_0 + 12 * (round - 1) + j
                      : partial   ? POS_WIRE_PARTIAL + (round - POS_FULL_HALF)
                                  : POS_WIRE_FULL_1 + 12 * (round - POS_FULL_HALF - POS_PARTIAL) + j;
        W[(u64)col * n] = gl_canon(((u64)hi << 32) | lo);
      }
    });
    if (j < 12) W[(u64)(POS_WIRE_OUTPUT + j) * n] = out;
    prev = out;
  }
}
void launch_pos_plan_chains(hipStream_t s, const PosJobDev *jobs, u64 npos, const u32 *chain_ends, u64 chain_begin, u64 chain_end,
                            const RecOperandDev *operands, u64 noperands, u64 *wires, u32 ncols, u64 n, const u64 *rc, u64 *flags, u64 gate,
                            u64 marker) {
  if (chain_begin >= chain_end) return;
  const u64 threads = (chain_end - chain_begin) * 16;
  hipLaunchKernelGGL(k_pos_plan_chains, dim3((unsigned)((threads + PLAN_CHAIN_THREADS - 1) / PLAN_CHAIN_THREADS)), dim3(PLAN_CHAIN_THREADS), 0, s,
                     jobs, npos, chain_ends, chain_begin, chain_end, operands, noperands, wires, ncols, n, rc, flags, gate, marker);
}

// One lane per u32 job of one LEVEL of lcp2_witness_plan_rows_u32 (u32_plan.hpp u32_plan_lane: the text tests/emu/emu_plan_u32.cpp
// runs on the CPU).  A lane reads its 16-byte job (contiguous over the wave), then its 1 to 4 operand records - 16 bytes each,
// consecutive for a lane; in a plan packed in job order the records of a wave are one contiguous run, so the loads walk whole cache
// lines - then the cells of its CELL operands, one gathered 8-byte load each, all issued before the first value is looked at.  The
// operands do not go through LDS: each record is read once, by one lane.  The values are checked, the inputs become a U32JobDev in
// registers, and u32_job_cells stores exactly as in k_u32_gate_rows: one 8-byte store per cell into its column, contiguous over the
// wave - 512 bytes - when its 64 jobs are consecutive rows of one (kind, op).  In that order a wave stays on one kind; only
// ARITHMETIC lanes run the one field inversion.  A refused job folds its shifted index into flags[2] and the family marker into
// flags[0] (row_flag.hpp); lanes of a level after a refused job's return at once.
constexpr u32 U32_PLAN_THREADS = 256;
__global__ __launch_bounds__(U32_PLAN_THREADS) void k_u32_plan_rows(const U32PlanJobDev *__restrict__ jobs, u64 base, u64 begin, u64 end,
                                                                     const RecOperandDev *__restrict__ operands, u64 noperands, u64 *wires,
                                                                     u32 ncols, u64 n, u64 *flags, u64 gate, u64 marker) {
  const u64 i = begin + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (const u32 problem = u32_plan_lane(jobs, base, begin, end, i, operands, noperands, wires, ncols, n, flags, gate)) {
    atomicMin((unsigned long long *)flags + 2, (unsigned long long)row_refusal(i, problem));
    atomicMin((unsigned long long *)flags, (unsigned long long)row_refusal(marker, ROW_U32_FAMILY));
  }
}
void launch_u32_plan_rows(hipStream_t s, const U32PlanJobDev *jobs, u64 base, u64 begin, u64 end, const RecOperandDev *operands, u64 noperands,
                          u64 *wires, u32 ncols, u64 n, u64 *flags, u64 gate, u64 marker) {
  if (begin >= end) return;
  hipLaunchKernelGGL(k_u32_plan_rows, dim3((unsigned)((end - begin + U32_PLAN_THREADS - 1) / U32_PLAN_THREADS)), dim3(U32_PLAN_THREADS), 0, s,
                     jobs, base, begin, end, operands, noperands, wires, ncols, n, flags, gate, marker);
}

// One 64-LANE WAVE per SHA-256 job of one LEVEL of lcp2_witness_plan_rows_sha, record and rows fused (sha_plan.hpp
// sha_plan_job_lane is the one-lane reference of this kernel and writes the same cells; tests/emu/emu_plan_sha.cpp runs it on the
// CPU).  The pair k_sha_jobs_level / k_sha_fill_rows would need a second launch per level, 1 344 bytes of record scratch per job and
// a per-job "valid" word; here the record lives in LDS for the life of the block and digests travel between levels only through the
// matrix.  A block is one wave, so the barriers below are the wave's own and a refused wave leaves nobody waiting.
//   load and check  every lane reads the 8-byte job (one address) and tests it; lane k < 16 reads operand record k (16 neighbouring
//                   records, 256 bytes), checks it before any index of it is used, loads its cell if it is a CELL, canonicalises
//                   and applies the value check.  The verdict is a minimum over the wave in the order of the reference - structure
//                   by operand index, then values by operand index - and is the same in every lane: a refused wave leaves together,
//                   after lane 0 has folded the job into flags[3] and the family marker into flags[0] (row_flag.hpp).
//   compress        the 16 words go into the record in LDS, lane 0 runs both compressions into it (sha_rows.hpp sha_words_record:
//                   336 words, the text of k_sha_jobs_level); the other lanes wait at the barrier.
//   fill            lane t writes rows t, t + 64, .. below 310 through sha_row_cells, as k_sha_fill_rows does from HBM: a store of
//                   the wave covers 64 consecutive rows of one column, 512 contiguous bytes.
// All 16 operands are loaded before the first store, so a CELL inside the job's own rows yields the word from before the call.
constexpr u32 SHA_PLAN_THREADS = 64;
__global__ __launch_bounds__(SHA_PLAN_THREADS) void k_sha_plan_jobs(const ShaPlanJobDev *__restrict__ jobs, u64 base, u64 begin, u64 end,
                                                                     const RecOperandDev *__restrict__ operands, u64 noperands, u64 *wires,
                                                                     u32 ncols, u64 n, u64 *flags, u64 gate, u64 marker) {
  __shared__ uint32_t rec[SHA_REC_WORDS];
  const u64 i = begin + blockIdx.x;
  const u32 lane = threadIdx.x;
  if (i >= end) return;
  if ((flags[0] >> 8) < gate) return;  // a job of an earlier level was refused: this level writes nothing
  const ShaPlanJobDev job = jobs[i - base];
  u32 problem = sha_plan_job_problem(job, noperands, n);  // the same in every lane
  u32 verdict = problem ? problem : 0xFFFFu;
  u64 v = 0;
  if (!problem && lane < SHA_PLAN_OPERANDS) {
    const RecOperandDev o = operands[(u64)job.first_operand + lane];
    problem = sha_plan_operand_problem(o, ncols, n);
    if (problem) verdict = lane << 8 | problem;
    else {
      v = gl_canon(o.src == PLAN_CELL ? wires[(u64)o.col * n + o.v] : o.v);
      if ((problem = sha_plan_value_problem(v)) != 0) verdict = (SHA_PLAN_OPERANDS + lane) << 8 | problem;
    }
  }
#pragma unroll
  for (u32 m = 1; m < 64; m <<= 1) verdict = min(verdict, (u32)__shfl_xor((int)verdict, (int)m, 64));
  if (verdict != 0xFFFFu) {
    if (lane == 0) {
      atomicMin((unsigned long long *)flags + 3, (unsigned long long)row_refusal(i, verdict & 0xFF));
      atomicMin((unsigned long long *)flags, (unsigned long long)row_refusal(marker, ROW_SHA_FAMILY));
    }
    return;
  }
  if (lane < SHA_PLAN_OPERANDS) rec[SHA_REC_IN + lane] = (uint32_t)v;
  __syncthreads();
  if (lane == 0) sha_words_record(rec + SHA_REC_IN, rec);
  __syncthreads();
  for (u32 lr = lane; lr < SHA_ROWS; lr += SHA_PLAN_THREADS) {
    u64 *W = wires + job.first_row + lr;
    sha_row_cells(rec, lr, [&](u32 col, u64 x) { W[(u64)col * n] = x; });
  }
}
void launch_sha_plan_jobs(hipStream_t s, const ShaPlanJobDev *jobs, u64 base, u64 begin, u64 end, const RecOperandDev *operands, u64 noperands,
                          u64 *wires, u32 ncols, u64 n, u64 *flags, u64 gate, u64 marker) {
  if (begin >= end) return;
  hipLaunchKernelGGL(k_sha_plan_jobs, dim3((unsigned)(end - begin)), dim3(SHA_PLAN_THREADS), 0, s, jobs, base, begin, end, operands, noperands,
                     wires, ncols, n, flags, gate, marker);
}

void launch_sha_jobs_level(hipStream_t s, const ShaJobDev *jobs, u32 first, u32 count, const uint32_t *words_in, uint32_t *rec) {
  if (!count) return;
  hipLaunchKernelGGL(k_sha_jobs_level, dim3((count + 63) / 64), dim3(64), 0, s, jobs, first, count, words_in, rec);
}
void launch_sha_fill_rows(hipStream_t s, const ShaJobDev *jobs, u32 njobs, const uint32_t *rec, u64 *wires, u64 n) {
  if (!njobs) return;
  u64 threads = (u64)njobs * SHA_ROWS;
  hipLaunchKernelGGL(k_sha_fill_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, jobs, njobs, rec, wires, n);
}
void launch_scatter_cells(hipStream_t s, const CellDev *cells, u64 ncells, u64 *wires, u64 n) {
  if (!ncells) return;
  hipLaunchKernelGGL(k_scatter_cells, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, s, cells, ncells, wires, n);
}

}  // namespace lcp2
