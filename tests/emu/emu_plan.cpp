// TEST HARNESS (not product code): csrc/pos_plan.hpp compiled for the CPU - the validation of lcp2_witness_plan_rows, the portable
// PoseidonGate job and chain texts, one level's two launches as lcp2_rec_gate_rows (no chains) and lcp2_witness_plan_rows make them
// (k_rec_gate_rows with its shifted indices, then the chains in the one-lane-per-chain reference form of k_pos_plan_chains) as
// loops over lanes, and the two flag words of row_flag.hpp with the entry points' decode of them.
// Built by tests/rows_lib.py with g++ and included by tests/emu/sanitize_plan_main.cpp; never loaded by the package.
#include "../../eth-lc-plonky2_amd/csrc/pos_plan.hpp"
#include "emu_rc.hpp"

using namespace lcp2;

extern "C" {

unsigned emu_plan_pos_job_bytes() { return (unsigned)sizeof(PosJobDev); }
unsigned emu_plan_operand_bytes() { return (unsigned)sizeof(RecOperandDev); }
unsigned emu_plan_pos_operands() { return POS_PLAN_OPERANDS; }
const char *emu_plan_problem_str(unsigned problem) { return pos_plan_problem_str(problem); }

// one PoseidonGate job as a host list sees it: its structure, then its swap value where that is IMM
unsigned emu_plan_pos_problem(const PosJobDev *job, int first, const RecOperandDev *operands, unsigned long long noperands, unsigned ncols,
                              unsigned long long n) {
  unsigned problem = pos_plan_problem(*job, first != 0, operands, noperands, ncols, n);
  if (!problem && operands[job->first_operand].src == PLAN_IMM) problem = pos_plan_swap_problem(gl_canon(operands[job->first_operand].v));
  return problem;
}

// the whole host plan as the entry point checks it: 0, or the problem with *family (0 rec, 1 poseidon) and *job
unsigned emu_plan_lists_problem(const RecJobDev *rec, unsigned long long nrec, const PosJobDev *pos, const unsigned *chain_ends,
                                unsigned long long nchains, const RecOperandDev *operands, unsigned long long noperands, unsigned ncols,
                                unsigned long long n, unsigned *family, unsigned long long *job) {
  const PlanProblem p = plan_lists_problem(rec, nrec, pos, chain_ends, nchains, operands, noperands, ncols, n);
  *family = p.family;
  *job = p.job;
  return p.problem;
}

// level `level` of lcp2_witness_plan_rows: the rec jobs [rec_begin, rec_end) lane by lane in blocks of `threads`, then the chains
// [chain_begin, chain_end); flags[0], flags[1] as the kernels keep them (both ROW_NO_PROBLEM before the first level)
void emu_plan_level(const RecJobDev *rec, unsigned long long rec_begin, unsigned long long rec_end, const PosJobDev *pos, unsigned long long npos,
                    const unsigned *chain_ends, unsigned long long chain_begin, unsigned long long chain_end, const RecOperandDev *operands,
                    unsigned long long noperands, unsigned long long *wires, unsigned ncols, unsigned long long n, unsigned long long *flags,
                    unsigned long long level, unsigned threads) {
  const u64 shift = plan_shift(level), gate = plan_gate(rec_begin, level);
  const u64 blocks = (rec_end - rec_begin + threads - 1) / threads;
  for (u64 b = 0; b < blocks; b++)
    for (unsigned t = 0; t < threads; t++) {
      const u64 i = rec_begin + shift + b * threads + t;
      const u64 problem = rec_rows_lane(rec, shift, rec_begin + shift, rec_end + shift, i, operands, noperands, wires, ncols, n, flags, true);
      if (problem && row_refusal(i, problem) < flags[0]) flags[0] = row_refusal(i, problem);
    }
  for (u64 c = chain_begin; c < chain_end; c++) {
    const u64 refusal = pos_plan_chain_lane(pos, npos, chain_ends, chain_begin, chain_end, c, operands, noperands, wires, ncols, n,
                                            emu_round_constants(), flags, gate);
    if (!refusal) continue;
    if (refusal < flags[1]) flags[1] = refusal;
    if (row_refusal(rec_end + shift, ROW_OTHER_FAMILY) < flags[0]) flags[0] = row_refusal(rec_end + shift, ROW_OTHER_FAMILY);
  }
}

// what the flag words name after the last level, as the entry points decode them: 0, or the problem with *family and *job
unsigned emu_plan_refusal(const unsigned long long *flags, const unsigned *rec_level_ends, unsigned long long nlevels, unsigned *family,
                          unsigned long long *job) {
  const PlanRefusal r = plan_refusal(flags, rec_level_ends, nlevels);
  *family = r.family;
  *job = r.job;
  return r.problem;
}

}  // extern "C"
