// SHA-256 jobs inside a recorded witness plan (lcp2_witness_plan_rows_sha): the 310 rows of one two_to_one_sha256 (sha_layout.hpp)
// with its 16 message words taken from the plan's one operand list instead of words_in.
//
// A job is (first_row, first_operand) and takes 16 operands (rec_rows.hpp RecOperandDev): W0..W15.  src is PLAN_IMM or PLAN_CELL,
// PLAN_PREV is refused as in a rec job.  Every operand is canonicalised when it is read and must then be a u32.  The digest lands in
// the matrix - digest word i at row first_row + 307 + i / 3, column 3 (i % 3) + 2 - so a CELL operand is all the chaining there is.
// This header is the portable text: the validation (sha_plan_problem and the value check), one job from its operands to its cells
// by ONE lane (sha_plan_job_lane: all 16 loads, then sha_rows.hpp sha_words_record into a record on the stack, then the 310 rows
// through sha_row_cells - the cells of lcp2_sha256_witness, from the same text), and the check of a host plan of all four families
// (plan_sha_lists_problem) - the reference of k_sha_plan_jobs (kernels_witness.hip), which runs a job with one 64-lane wave and
// writes the same cells, what the level runner of witness_rows.hip validates a host list with, and what tests/emu/emu_plan_sha.cpp
// runs on the CPU.
#pragma once
#include "sha_rows.hpp"
#include "u32_plan.hpp"

namespace lcp2 {

constexpr u32 SHA_PLAN_OPERANDS = 16;  // W0..W15
constexpr u32 SHA_PLAN_ROWS = 1, SHA_PLAN_OPERANDS_PAST_END = 2, SHA_PLAN_SRC = 3, SHA_PLAN_CELL_COLUMN = 4, SHA_PLAN_CELL_ROW = 5,
              SHA_PLAN_NOT_U32 = 6;

struct ShaPlanJobDev {  // = lcp2_sha_plan_job
  uint32_t first_row, first_operand;
};

// Structure, in the order sha_plan_problem_str lists it.  The job's own fields, then one operand of it
LCP2_HD u32 sha_plan_job_problem(const ShaPlanJobDev &j, u64 noperands, u64 n) {
  if ((u64)j.first_row + SHA_ROWS > n) return SHA_PLAN_ROWS;
  if ((u64)j.first_operand + SHA_PLAN_OPERANDS > noperands) return SHA_PLAN_OPERANDS_PAST_END;
  return 0;
}
LCP2_HD u32 sha_plan_operand_problem(const RecOperandDev &o, u32 ncols, u64 n) {
  if (o.src > PLAN_CELL) return SHA_PLAN_SRC;
  if (o.src == PLAN_CELL && o.col >= ncols) return SHA_PLAN_CELL_COLUMN;
  if (o.src == PLAN_CELL && o.v >= n) return SHA_PLAN_CELL_ROW;
  return 0;
}
// 0: the job may read its operands and write its rows; otherwise why lcp2_witness_plan_rows_sha refuses it
LCP2_HD u32 sha_plan_problem(const ShaPlanJobDev &j, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  if (const u32 problem = sha_plan_job_problem(j, noperands, n)) return problem;
  for (u32 k = 0; k < SHA_PLAN_OPERANDS; k++)
    if (const u32 problem = sha_plan_operand_problem(operands[(u64)j.first_operand + k], ncols, n)) return problem;
  return 0;
}
// the verdict on one operand's value, canonical
LCP2_HD u32 sha_plan_value_problem(u64 v) { return v >> 32 ? SHA_PLAN_NOT_U32 : 0; }
inline const char *sha_plan_problem_str(u32 problem) {
  switch (problem) {
    case SHA_PLAN_ROWS: return "rows out of range";
    case SHA_PLAN_OPERANDS_PAST_END: return "operands run past the end of the operand list";
    case SHA_PLAN_SRC: return "operand src above 1";
    case SHA_PLAN_CELL_COLUMN: return "cell operand column out of range";
    case SHA_PLAN_CELL_ROW: return "cell operand row out of range";
    case SHA_PLAN_NOT_U32: return "operand value of 2^32 or more";
    default: return "ok";
  }
}

// A HOST list checked completely: the structure of every job, and the values of the operands that are IMM.  problem 0: nothing to
// refuse; otherwise the first refused job
inline RecListProblem sha_plan_list_problem(const ShaPlanJobDev *jobs, u64 njobs, const RecOperandDev *operands, u64 noperands, u32 ncols, u64 n) {
  for (u64 i = 0; i < njobs; i++) {
    if (const u32 problem = sha_plan_problem(jobs[i], operands, noperands, ncols, n)) return {problem, i};
    for (u32 k = 0; k < SHA_PLAN_OPERANDS; k++) {
      const RecOperandDev &o = operands[(u64)jobs[i].first_operand + k];
      if (o.src != PLAN_IMM) continue;
      if (const u32 problem = sha_plan_value_problem(gl_canon(o.v))) return {problem, i};
    }
  }
  return {0, 0};
}
// A HOST plan of four families, as lcp2_witness_plan_rows_sha checks it before it writes anything: the rec jobs, then the SHA jobs,
// then the u32 jobs, then the PoseidonGate jobs.  family as in PlanRefusal: 0 rec, 1 PoseidonGate, 2 u32, 3 SHA
inline PlanProblem plan_sha_lists_problem(const RecJobDev *rec, u64 nrec, const ShaPlanJobDev *sha, u64 nsha, const U32PlanJobDev *u32_jobs, u64 nu32,
                                          const PosJobDev *pos, const u32 *chain_ends, u64 nchains, const RecOperandDev *operands, u64 noperands,
                                          u32 ncols, u64 n) {
  if (const RecListProblem bad = rec_lists_problem(rec, nrec, operands, noperands, ncols, n); bad.problem) return {0, bad.problem, bad.job};
  if (const RecListProblem bad = sha_plan_list_problem(sha, nsha, operands, noperands, ncols, n); bad.problem) return {3, bad.problem, bad.job};
  return plan_u32_lists_problem(nullptr, 0, u32_jobs, nu32, pos, chain_ends, nchains, operands, noperands, ncols, n);
}

// The ONE-LANE reference of k_sha_plan_jobs: job i of the jobs [begin, end) of one level, its indices shifted as k_rec_gate_rows'
// are (row_flag.hpp): jobs[0] is job `base` of the list.  Returns 0 when the job ran (or there was nothing to do), else the problem
// of job i, which then wrote nothing: structure by operand index first, then values by operand index.  No index is used before it
// is checked, and all 16 operands are loaded before the first store: a CELL inside the job's own rows yields the word from before
// the call.  flags, gate: row_flag.hpp - a level that begins after a refusal writes nothing.
LCP2_SHA_LANE u32 sha_plan_job_lane(const ShaPlanJobDev *jobs, u64 base, u64 begin, u64 end, u64 i, const RecOperandDev *operands, u64 noperands,
                                    u64 *wires, u32 ncols, u64 n, const u64 *flags, u64 gate) {
  if (i < begin || i >= end) return 0;
  if ((flags[0] >> 8) < gate) return 0;
  const ShaPlanJobDev job = jobs[i - base];
  if (const u32 problem = sha_plan_job_problem(job, noperands, n)) return problem;
  RecOperandDev o[SHA_PLAN_OPERANDS];
  for (u32 k = 0; k < SHA_PLAN_OPERANDS; k++) o[k] = operands[(u64)job.first_operand + k];
  for (u32 k = 0; k < SHA_PLAN_OPERANDS; k++)
    if (const u32 problem = sha_plan_operand_problem(o[k], ncols, n)) return problem;
  uint32_t msg[SHA_PLAN_OPERANDS];
  for (u32 k = 0; k < SHA_PLAN_OPERANDS; k++) {
    const u64 v = gl_canon(o[k].src == PLAN_CELL ? wires[(u64)o[k].col * n + o[k].v] : o[k].v);
    if (const u32 problem = sha_plan_value_problem(v)) return problem;
    msg[k] = (uint32_t)v;
  }
  uint32_t R[SHA_REC_WORDS];
  sha_words_record(msg, R);
  for (u32 lr = 0; lr < SHA_ROWS; lr++) {
    u64 *W = wires + job.first_row + lr;
    sha_row_cells(R, lr, [&](u32 col, u64 x) { W[(u64)col * n] = x; });
  }
  return 0;
}

}  // namespace lcp2
