// PoseidonGate rows inside a recorded witness plan (lcp2_witness_plan_rows): CHAINS of rows whose inputs are immediates, cells of
// the witness matrix, or outputs of the previous row of the same chain.
//
// A job is (row, first_operand) and takes 13 operands of the plan's one operand list (rec_rows.hpp RecOperandDev): the swap flag,
// then the 12 inputs.  src PLAN_IMM / PLAN_CELL are REC_IMM / REC_CELL; PLAN_PREV with col = j < 12 is output j of the previous job
// of the chain, carried in registers and never re-read from the matrix.  Chain g is the jobs [chain_ends[g-1], chain_ends[g]).
// This header is the portable text: the validation (pos_plan_problem), one job from its operands to the 135 cells of its row
// (pos_plan_job_cells, which ends in pos_rows.hpp pos_row_cells), and one chain walked by ONE lane (pos_plan_chain_lane) - what
// lcp2_witness_plan_rows validates a host list with, what tests/emu/emu_plan.cpp runs on the CPU, and the reference for
// k_pos_plan_chains (kernels_witness.hip), which walks a chain with a 16-lane group instead and writes the same cells.
#pragma once
#include "pos_rows.hpp"
#include "rec_rows.hpp"

namespace lcp2 {

constexpr u32 PLAN_IMM = REC_IMM, PLAN_CELL = REC_CELL, PLAN_PREV = 2;
constexpr u32 POS_PLAN_OPERANDS = 13;  // swap, in[0..11]
constexpr u32 POS_PLAN_SWAP_NOT_BOOLEAN = 9;

struct PosJobDev {  // = lcp2_pos_job
  uint32_t row, first_operand;
};

// Structure, in the order pos_plan_problem_str lists it.  The job's own fields, then operand k of it (first: the chain's first job)
LCP2_HD u32 pos_plan_job_problem(const PosJobDev &j, u64 noperands, u64 n) {
  if (j.row >= n) return 1;
  if ((u64)j.first_operand + POS_PLAN_OPERANDS > noperands) return 2;
  return 0;
}
LCP2_HD u32 pos_plan_operand_problem(const RecOperandDev &o, u32 k, bool first, u32 ncols, u64 n) {
  if (o.src > PLAN_PREV) return 3;
  if (o.src == PLAN_PREV) {
    if (first) return 4;
    if (k == 0) return 5;
    if (o.col >= 12) return 6;
  }
  if (o.src == PLAN_CELL && o.col >= ncols) return 7;
  if (o.src == PLAN_CELL && o.v >= n) return 8;
  return 0;
}
// 0: the job may read its operands and write its row; otherwise why lcp2_witness_plan_rows refuses it
LCP2_HD u32 pos_plan_problem(const PosJobDev &j, bool first, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  if (const u32 problem = pos_plan_job_problem(j, noperands, n)) return problem;
  for (u32 k = 0; k < POS_PLAN_OPERANDS; k++)
    if (const u32 problem = pos_plan_operand_problem(operands[(u64)j.first_operand + k], k, first, ncols, n)) return problem;
  return 0;
}
// the verdict on the swap operand's value, canonical
LCP2_HD u32 pos_plan_swap_problem(u64 v) { return v > 1 ? POS_PLAN_SWAP_NOT_BOOLEAN : 0; }
inline const char *pos_plan_problem_str(u32 problem) {
  switch (problem) {
    case 1: return "row out of range";
    case 2: return "operands run past the end of the operand list";
    case 3: return "operand src above 2";
    case 4: return "PREV operand in the first job of a chain";
    case 5: return "PREV as the swap operand";
    case 6: return "PREV operand column of 12 or more";
    case 7: return "cell operand column out of range";
    case 8: return "cell operand row out of range";
    case 9: return "swap value not 0 or 1";
    default: return "ok";
  }
}

// A HOST plan checked completely, as lcp2_witness_plan_rows does before it writes anything: the rec jobs first, then the PoseidonGate
// jobs chain by chain - structure, and the values that are IMM.  family 0: a rec job (rec_problem_str), 1: a PoseidonGate job;
// problem 0: nothing to refuse.  chain_ends: ascending and ending at npos (the entry point checks that first).
struct PlanProblem {
  u32 family, problem;
  u64 job;
};
inline PlanProblem plan_lists_problem(const RecJobDev *rec, u64 nrec, const PosJobDev *pos, const u32 *chain_ends, u64 nchains,
                                      const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  if (const RecListProblem bad = rec_lists_problem(rec, nrec, operands, noperands, ncols, n); bad.problem) return {0, bad.problem, bad.job};
  for (u64 g = 0; g < nchains; g++) {
    const u64 begin = g ? chain_ends[g - 1] : 0;
    for (u64 i = begin; i < chain_ends[g]; i++) {
      u32 problem = pos_plan_problem(pos[i], i == begin, operands, noperands, ncols, n);
      if (!problem && operands[pos[i].first_operand].src == PLAN_IMM) problem = pos_plan_swap_problem(gl_canon(operands[pos[i].first_operand].v));
      if (problem) return {1, problem, i};
    }
  }
  return {0, 0, 0};
}

// The jobs of chain c: [begin, end).  A device chain_ends is not validated as a list: an entry past npos is clipped and a
// descending one gives an empty chain, so no index leaves the job list whatever the table holds.
LCP2_HD void pos_plan_chain_range(const u32 *chain_ends, u64 c, u64 npos, u64 &begin, u64 &end) {
  begin = c ? chain_ends[c - 1] : 0;
  end = chain_ends[c];
  if (end > npos) end = npos;
  if (begin > end) begin = end;
}

// One job whose structure is valid.  mine: its 13 operands; prev: the 12 outputs of the job before it in the chain; cell(row, col):
// a load from the matrix; put(column, canonical value): all 135 cells as pos_row_cells writes them.  Returns 0, or
// POS_PLAN_SWAP_NOT_BOOLEAN and writes nothing.
template <class Cell, class Mds, class Put>
LCP2_HD u32 pos_plan_job_cells(const RecOperandDev *mine, const u64 prev[12], Cell cell, const u64 *rc, Mds mds, Put put) {
  auto get = [&](u32 k) -> u64 {
    const RecOperandDev o = mine[k];
    return o.src == PLAN_CELL ? cell(o.v, o.col) : o.src == PLAN_PREV ? prev[o.col] : o.v;
  };
  const u64 swap = gl_canon(get(0));
  if (const u32 problem = pos_plan_swap_problem(swap)) return problem;
  u64 in[12];
  for (u32 k = 0; k < 12; k++) in[k] = get(1 + k);
  pos_row_cells(in, swap != 0, rc, mds, put);
  return 0;
}

// Lane c of one level's chain launch in the one-lane-per-chain form: chain c of [chain_begin, chain_end).  Returns 0 when the chain
// ran (or the lane had nothing to do), else row_refusal(job, problem) of the job that stopped it: the rows before that job are
// written, that row and the rest of the chain are not.  flags, gate: row_flag.hpp - a level that begins after a refusal writes nothing.
LCP2_HD u64 pos_plan_chain_lane(const PosJobDev *jobs, u64 npos, const u32 *chain_ends, u64 chain_begin, u64 chain_end, u64 c,
                                const RecOperandDev *operands, u64 noperands, u64 *wires, u32 ncols, u64 n, const u64 *rc, const u64 *flags,
                                u64 gate) {
  if (c < chain_begin || c >= chain_end) return 0;
  if ((flags[0] >> 8) < gate) return 0;
  u64 begin, end;
  pos_plan_chain_range(chain_ends, c, npos, begin, end);
  u64 prev[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (u64 i = begin; i < end; i++) {
    const PosJobDev job = jobs[i];
    if (const u32 problem = pos_plan_problem(job, i == begin, operands, noperands, ncols, n)) return row_refusal(i, problem);
    u64 *W = wires + job.row;
    u64 out[12];
    const u32 problem = pos_plan_job_cells(
        operands + job.first_operand, prev, [&](u64 row, u32 col) { return wires[(u64)col * n + row]; }, rc, [](u64 *s) { pos_mds(s); },
        [&](u32 col, u64 v) {
          W[(u64)col * n] = v;
          if (col >= POS_WIRE_OUTPUT && col < POS_WIRE_OUTPUT + 12) out[col - POS_WIRE_OUTPUT] = v;
        });
    if (problem) return row_refusal(i, problem);
    for (u32 k = 0; k < 12; k++) prev[k] = out[k];
  }
  return 0;
}

}  // namespace lcp2
