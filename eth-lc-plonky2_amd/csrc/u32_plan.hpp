// plonky2_u32 / comparison jobs inside a recorded witness plan (lcp2_witness_plan_rows_u32): the jobs of lcp2_u32_gate_rows with
// their inputs taken from the plan's one operand list instead of four immediates.
//
// A job is (row, kind, op, first_operand) and takes u32_plan_operands(kind) operands (rec_rows.hpp RecOperandDev) in the order of
// in[] of a U32JobDev; src is PLAN_IMM or PLAN_CELL, PLAN_PREV is refused as in a rec job.  Every operand is canonicalised when it
// is read and must then be a u32.  This header is the portable text: the validation (u32_plan_problem and the two value checks),
// one job of a level from its operands to its cells (u32_plan_lane, which resolves the operands into a U32JobDev and ends in
// u32_rows.hpp u32_job_cells: the cells of lcp2_u32_gate_rows, from the same text), and the check of a host plan of all three
// families (plan_u32_lists_problem) - what k_u32_plan_rows (kernels_witness.hip) runs per lane, what the level runner of
// witness_rows.hip validates a host list with, and what tests/emu/emu_plan_u32.cpp runs on the CPU.
#pragma once
#include "pos_plan.hpp"
#include "u32_rows.hpp"

namespace lcp2 {

constexpr u32 U32_PLAN_MAX_OPERANDS = 4;
// the reasons after the four of u32_job_problem
constexpr u32 U32_PLAN_OPERANDS_PAST_END = 5, U32_PLAN_SRC = 6, U32_PLAN_CELL_COLUMN = 7, U32_PLAN_CELL_ROW = 8, U32_PLAN_NOT_U32 = 9;

struct U32PlanJobDev {  // = lcp2_u32_plan_job
  uint32_t row;
  uint16_t kind, op;
  uint32_t first_operand, reserved;
};

LCP2_HD u32 u32_plan_operands(u32 kind) {
  return kind == U32_KIND_ARITHMETIC ? 3 : kind == U32_KIND_ADD_MANY ? 4 : kind == U32_KIND_SUBTRACTION ? 3 : kind == U32_KIND_RANGE_CHECK ? 1
       : kind == U32_KIND_COMPARISON ? 2 : 0;
}
LCP2_HD U32JobDev u32_plan_shape(const U32PlanJobDev &j) { return {j.row, j.kind, j.op, {0, 0, 0, 0}}; }

// Structure, in the order u32_plan_problem_str lists it.  The job's own fields (u32_job_problem on the job without inputs: row,
// kind, op), then one operand of it
LCP2_HD u32 u32_plan_job_problem(const U32PlanJobDev &j, u64 noperands, u64 n) {
  if (const u32 problem = u32_job_problem(u32_plan_shape(j), n)) return problem;
  if ((u64)j.first_operand + u32_plan_operands(j.kind) > noperands) return U32_PLAN_OPERANDS_PAST_END;
  return 0;
}
LCP2_HD u32 u32_plan_operand_problem(const RecOperandDev &o, u32 ncols, u64 n) {
  if (o.src > PLAN_CELL) return U32_PLAN_SRC;
  if (o.src == PLAN_CELL && o.col >= ncols) return U32_PLAN_CELL_COLUMN;
  if (o.src == PLAN_CELL && o.v >= n) return U32_PLAN_CELL_ROW;
  return 0;
}
// 0: the job may read its operands and write its cells; otherwise why lcp2_witness_plan_rows_u32 refuses it
LCP2_HD u32 u32_plan_problem(const U32PlanJobDev &j, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  if (const u32 problem = u32_plan_job_problem(j, noperands, n)) return problem;
  for (u32 k = 0; k < u32_plan_operands(j.kind); k++)
    if (const u32 problem = u32_plan_operand_problem(operands[(u64)j.first_operand + k], ncols, n)) return problem;
  return 0;
}
// Values.  The verdict on one operand's value, canonical; the borrow of a subtraction is u32_job_problem's on the resolved job
LCP2_HD u32 u32_plan_value_problem(u64 v) { return v >> 32 ? U32_PLAN_NOT_U32 : 0; }
inline const char *u32_plan_problem_str(u32 problem) {
  switch (problem) {
    case U32_PLAN_OPERANDS_PAST_END: return "operands run past the end of the operand list";
    case U32_PLAN_SRC: return "operand src above 1";
    case U32_PLAN_CELL_COLUMN: return "cell operand column out of range";
    case U32_PLAN_CELL_ROW: return "cell operand row out of range";
    case U32_PLAN_NOT_U32: return "operand value of 2^32 or more";
    default: return u32_problem_str(problem);
  }
}

// A HOST list checked completely: the structure of every job, and the value conditions of the operands that are IMM.  problem 0:
// nothing to refuse; otherwise the first refused job
inline RecListProblem u32_plan_list_problem(const U32PlanJobDev *jobs, u64 njobs, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  for (u64 i = 0; i < njobs; i++) {
    if (const u32 problem = u32_plan_problem(jobs[i], operands, noperands, ncols, n)) return {problem, i};
    U32JobDev resolved = u32_plan_shape(jobs[i]);
    for (u32 k = 0; k < u32_plan_operands(jobs[i].kind); k++) {
      const RecOperandDev &o = operands[(u64)jobs[i].first_operand + k];
      if (o.src != PLAN_IMM) continue;
      if (const u32 problem = u32_plan_value_problem(gl_canon(o.v))) return {problem, i};
      resolved.in[k] = (u32)gl_canon(o.v);
    }
    if (const u32 problem = u32_job_problem(resolved, n)) return {problem, i};  // an IMM borrow above 1 (a CELL counts as 0 here)
  }
  return {0, 0};
}
// A HOST plan of three families, as lcp2_witness_plan_rows_u32 checks it before it writes anything: the rec jobs, then the u32
// jobs, then the PoseidonGate jobs.  family as in PlanRefusal: 0 rec, 1 PoseidonGate, 2 u32
inline PlanProblem plan_u32_lists_problem(const RecJobDev *rec, u64 nrec, const U32PlanJobDev *u32_jobs, u64 nu32, const PosJobDev *pos,
                                          const u32 *chain_ends, u64 nchains, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  if (const RecListProblem bad = rec_lists_problem(rec, nrec, operands, noperands, ncols, n); bad.problem) return {0, bad.problem, bad.job};
  if (const RecListProblem bad = u32_plan_list_problem(u32_jobs, nu32, operands, noperands, ncols, n); bad.problem) return {2, bad.problem, bad.job};
  return plan_lists_problem(nullptr, 0, pos, chain_ends, nchains, operands, noperands, ncols, n);
}

// Lane i of k_u32_plan_rows over the jobs [begin, end) of one level, its indices shifted as k_rec_gate_rows' are (row_flag.hpp):
// jobs[0] is job `base` of the list.  Returns 0 when the job ran (or the lane had nothing to do), else the problem of job i, which
// then wrote nothing.  No index is used before it is checked.  The operand records are all read before the first cell, and the
// cells before the first value is looked at: two rounds of independent loads, not one dependent chain per operand.
// flags, gate: row_flag.hpp - a level that begins after a refusal writes nothing.
LCP2_HD u32 u32_plan_lane(const U32PlanJobDev *jobs, u64 base, u64 begin, u64 end, u64 i, const RecOperandDev *operands, u64 noperands,
                          u64 *wires, u32 ncols, u64 n, const u64 *flags, u64 gate) {
  if (i < begin || i >= end) return 0;
  if ((flags[0] >> 8) < gate) return 0;
  const U32PlanJobDev job = jobs[i - base];
  if (const u32 problem = u32_plan_job_problem(job, noperands, n)) return problem;
  const u32 count = u32_plan_operands(job.kind);
  RecOperandDev o[U32_PLAN_MAX_OPERANDS];
  for (u32 k = 0; k < U32_PLAN_MAX_OPERANDS; k++) o[k] = k < count ? operands[(u64)job.first_operand + k] : RecOperandDev{0, 0, PLAN_IMM};
  for (u32 k = 0; k < U32_PLAN_MAX_OPERANDS; k++)
    if (const u32 problem = u32_plan_operand_problem(o[k], ncols, n)) return problem;
  u64 v[U32_PLAN_MAX_OPERANDS];
  for (u32 k = 0; k < U32_PLAN_MAX_OPERANDS; k++) v[k] = o[k].src == PLAN_CELL ? wires[(u64)o[k].col * n + o[k].v] : o[k].v;
  U32JobDev resolved = u32_plan_shape(job);
  for (u32 k = 0; k < U32_PLAN_MAX_OPERANDS; k++) {
    v[k] = gl_canon(v[k]);
    if (const u32 problem = u32_plan_value_problem(v[k])) return problem;
    resolved.in[k] = (u32)v[k];
  }
  if (const u32 problem = u32_job_problem(resolved, n)) return problem;  // a subtraction borrow above 1
  u64 *W = wires + job.row;
  u32_job_cells(resolved, [&](u32 col, u64 x) { W[(u64)col * n] = x; });
  return 0;
}

}  // namespace lcp2
