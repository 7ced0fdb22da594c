// TEST HARNESS (not product code): csrc/sha_plan.hpp compiled for the CPU - the validation of lcp2_witness_plan_rows_sha, the one-lane
// reference of k_sha_plan_jobs, one level's four launches as the level runner makes them (k_rec_gate_rows, k_sha_plan_jobs and
// k_u32_plan_rows with their shifted indices, then the chains in the one-lane-per-chain reference form of k_pos_plan_chains) as
// loops, and the four flag words of row_flag.hpp with the entry point's decode of them.
// Built by tests/test_sha_plan_emu.py through rows_lib.build_emu and included by tests/emu/sanitize_plan_sha_main.cpp; never loaded
// by the package.
#include "../../eth-lc-plonky2_amd/csrc/sha_plan.hpp"
#include "emu_rc.hpp"

using namespace lcp2;

extern "C" {

unsigned emu_plan_sha_job_bytes() { return (unsigned)sizeof(ShaPlanJobDev); }
unsigned emu_plan_sha_operands() { return SHA_PLAN_OPERANDS; }
const char *emu_plan_sha_problem_str(unsigned problem) { return sha_plan_problem_str(problem); }

// the whole host plan as the entry point checks it: 0, or the problem with *family (0 rec, 1 poseidon, 2 u32, 3 sha) and *job
unsigned emu_plan_sha_lists_problem(const RecJobDev *rec, unsigned long long nrec, const ShaPlanJobDev *sha, unsigned long long nsha,
                                    const U32PlanJobDev *u32_jobs, unsigned long long nu32, const PosJobDev *pos, const unsigned *chain_ends,
                                    unsigned long long nchains, const RecOperandDev *operands, unsigned long long noperands, unsigned ncols,
                                    unsigned long long n, unsigned *family, unsigned long long *job) {
  const PlanProblem p = plan_sha_lists_problem(rec, nrec, sha, nsha, u32_jobs, nu32, pos, chain_ends, nchains, operands, noperands, ncols, n);
  *family = p.family;
  *job = p.job;
  return p.problem;
}

// level `level` of lcp2_witness_plan_rows_sha: the rec jobs [rec_begin, rec_end) lane by lane in blocks of `threads`, the SHA jobs
// [sha_begin, sha_end) one after the other (a block of the kernel is one job), the u32 jobs [u32_begin, u32_end) like the rec jobs,
// then the chains [chain_begin, chain_end); flags[0..3] as the kernels keep them (all ROW_NO_PROBLEM before the first level)
void emu_plan_sha_level(const RecJobDev *rec, unsigned long long rec_begin, unsigned long long rec_end, const ShaPlanJobDev *sha,
                        unsigned long long sha_begin, unsigned long long sha_end, const U32PlanJobDev *u32_jobs, unsigned long long u32_begin,
                        unsigned long long u32_end, const PosJobDev *pos, unsigned long long npos, const unsigned *chain_ends,
                        unsigned long long chain_begin, unsigned long long chain_end, const RecOperandDev *operands, unsigned long long noperands,
                        unsigned long long *wires, unsigned ncols, unsigned long long n, unsigned long long *flags, unsigned long long level,
                        unsigned threads) {
  const u64 shift = plan_shift(level), gate = plan_gate(rec_begin, level), marker = rec_end + shift;
  auto fold = [](unsigned long long &word, u64 refusal) {
    if (refusal < word) word = refusal;
  };
  for (u64 b = 0; b < (rec_end - rec_begin + threads - 1) / threads; b++)
    for (unsigned t = 0; t < threads; t++) {
      const u64 i = rec_begin + shift + b * threads + t;
      if (const u64 problem = rec_rows_lane(rec, shift, rec_begin + shift, rec_end + shift, i, operands, noperands, wires, ncols, n, flags, true))
        fold(flags[0], row_refusal(i, problem));
    }
  for (u64 i = sha_begin + shift; i < sha_end + shift; i++)
    if (const u32 problem = sha_plan_job_lane(sha, shift, sha_begin + shift, sha_end + shift, i, operands, noperands, wires, ncols, n, flags, gate)) {
      fold(flags[3], row_refusal(i, problem));
      fold(flags[0], row_refusal(marker, ROW_SHA_FAMILY));
    }
  for (u64 b = 0; b < (u32_end - u32_begin + threads - 1) / threads; b++)
    for (unsigned t = 0; t < threads; t++) {
      const u64 i = u32_begin + shift + b * threads + t;
      if (const u32 problem = u32_plan_lane(u32_jobs, shift, u32_begin + shift, u32_end + shift, i, operands, noperands, wires, ncols, n, flags, gate)) {
        fold(flags[2], row_refusal(i, problem));
        fold(flags[0], row_refusal(marker, ROW_U32_FAMILY));
      }
    }
  for (u64 c = chain_begin; c < chain_end; c++)
    if (const u64 refusal = pos_plan_chain_lane(pos, npos, chain_ends, chain_begin, chain_end, c, operands, noperands, wires, ncols, n,
                                                emu_round_constants(), flags, gate)) {
      fold(flags[1], refusal);
      fold(flags[0], row_refusal(marker, ROW_OTHER_FAMILY));
    }
}

// what the four flag words name after the last level, as the entry point decodes them: 0, or the problem with *family and *job
unsigned emu_plan_sha_refusal(const unsigned long long *flags, const unsigned *rec_level_ends, const unsigned *u32_level_ends,
                              const unsigned *sha_level_ends, unsigned long long nlevels, unsigned *family, unsigned long long *job) {
  const PlanRefusal r = plan_refusal_sha(flags, rec_level_ends, u32_level_ends, sha_level_ends, nlevels);
  *family = r.family;
  *job = r.job;
  return r.problem;
}

}  // extern "C"
