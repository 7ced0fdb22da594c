// The refusal flag of the row generators that validate a job list on the device (lcp2_u32_gate_rows, lcp2_rec_gate_rows,
// lcp2_witness_plan_rows, lcp2_witness_plan_rows_u32, lcp2_witness_plan_rows_sha).
//
// One 64-bit word per call, two for a plan, three for a plan with u32 jobs, four for one with SHA jobs.  The entry point sets it to ROW_NO_PROBLEM before the
// first launch; a lane whose job is
// refused writes no cell and folds row_refusal(index, problem) into the word with a minimum (the kernels: atomicMin; tests/emu: a
// compare), so after the last launch the word names the FIRST refused job of the list and why (u32_problem_str / rec_problem_str),
// whatever the order the lanes ran in.  The entry point reads it back once (witness_rows.hip RefusalFlag).
#pragma once
#include "gl64.hpp"

namespace lcp2 {

constexpr u64 ROW_NO_PROBLEM = ~0ull;  // no job of the call has been refused
LCP2_HD u64 row_refusal(u64 index, u64 problem) { return index << 8 | problem; }  // problem in [1, 255]


// A plan (lcp2_rec_gate_rows is one without chains) runs TWO families level by level - rec jobs (k_rec_gate_rows) and PoseidonGate
// chains (k_pos_plan_chains) - and a refusal in either must stop every later level of both.  The choice: a family bit folded into ONE
// word, and a second word that only names the PoseidonGate job.
//   flags[0]  the word k_rec_gate_rows folds its refusals into and tests before it runs.  Level l of EVERY call is launched with its
//             job indices shifted by plan_shift(l) = l + 1, so the key of level l, plan_gate(begin_l, l) = begin_l + l + 1, grows
//             strictly from level to level even where a level holds no rec job.  A refused rec job i of level l folds
//             row_refusal(i + l + 1, problem); a refused chain of level l folds row_refusal(end_l + l + 1, ROW_OTHER_FAMILY): above
//             every rec refusal of its own level - the minimum keeps the rec job, which is the one the error names when both
//             families refuse in a level - not below the key of level l, so the other chains of the level still run, and below the
//             key of level l + 1.  Both kernels return at once when (flags[0] >> 8) < the key of their level.
//   flags[1]  the minimum of row_refusal(PoseidonGate job, problem) over the refused chains, read when flags[0] carries the bit.
constexpr u64 ROW_OTHER_FAMILY = 0xFF;  // the problem byte of flags[0] when the refusal is the other family's: above every reason
LCP2_HD u64 plan_shift(u64 level) { return level + 1; }
LCP2_HD u64 plan_gate(u64 rec_begin, u64 level) { return rec_begin + plan_shift(level); }

// What the two words say after the last level.  problem 0: nothing refused; else the family (0 rec, 1 PoseidonGate), the index of
// the job in its list and why.  A rec job's level is the one whose shifted range holds the index
struct PlanRefusal {
  u32 family, problem;
  u64 job;
};
inline PlanRefusal plan_refusal(const u64 *words, const uint32_t *rec_level_ends, size_t nlevels) {
  if (words[0] == ROW_NO_PROBLEM) return {0, 0, 0};
  const u32 problem = (u32)(words[0] & 0xFF);
  if (problem == ROW_OTHER_FAMILY) return {1, (u32)(words[1] & 0xFF), words[1] >> 8};
  const u64 shifted = words[0] >> 8;
  for (size_t l = 0; l < nlevels; l++)
    if (shifted >= plan_gate(l ? rec_level_ends[l - 1] : 0, l) && shifted < rec_level_ends[l] + plan_shift(l)) return {0, problem, shifted - plan_shift(l)};
  return {0, problem, 0};
}

// A plan with u32 jobs (lcp2_witness_plan_rows_u32) runs a THIRD family between the two: per level the rec jobs, the u32 jobs
// (k_u32_plan_rows), the chains.  flags[0] keeps its meaning and its gate.  A refused u32 job of level l folds
// row_refusal(end_l + l + 1, ROW_U32_FAMILY) into it - the key of a refused chain, one below it in the problem byte: above every rec
// refusal of the level, below the chain's, so the minimum orders the three families rec / u32 / PoseidonGate - and its own
//   flags[2]  the minimum of row_refusal(u32 job + plan_shift(l), problem) over the refused u32 jobs, shifted per level like the rec
//             jobs of flags[0], so that the word orders by list index across levels; read when flags[0] carries ROW_U32_FAMILY.
// family 2: a u32 job (u32_plan_problem_str).  A call without u32 jobs keeps two words and plan_refusal.
constexpr u64 ROW_U32_FAMILY = 0xFE;
inline PlanRefusal plan_refusal_u32(const u64 *words, const uint32_t *rec_level_ends, const uint32_t *u32_level_ends, size_t nlevels) {
  if (words[0] == ROW_NO_PROBLEM || (words[0] & 0xFF) != ROW_U32_FAMILY) return plan_refusal(words, rec_level_ends, nlevels);
  const u32 problem = (u32)(words[2] & 0xFF);
  const u64 shifted = words[2] >> 8;
  for (size_t l = 0; l < nlevels; l++)
    if (shifted >= plan_gate(l ? u32_level_ends[l - 1] : 0, l) && shifted < u32_level_ends[l] + plan_shift(l)) return {2, problem, shifted - plan_shift(l)};
  return {2, problem, 0};
}

// A plan with SHA-256 jobs (lcp2_witness_plan_rows_sha) runs a FOURTH family after the rec jobs: per level the rec jobs, the SHA
// jobs (k_sha_plan_jobs), the u32 jobs, the chains.  A refused SHA job of level l folds row_refusal(end_l + l + 1, ROW_SHA_FAMILY)
// into flags[0] - the key of a refused u32 job or chain, one below the u32 marker in the problem byte, so the minimum orders the
// four families rec / SHA / u32 / PoseidonGate and every word above keeps its meaning - and its own
//   flags[3]  the minimum of row_refusal(SHA job + plan_shift(l), problem) over the refused SHA jobs, shifted per level like
//             flags[2]; read when flags[0] carries ROW_SHA_FAMILY.
// family 3: a SHA job (sha_plan_problem_str).  A call without SHA jobs keeps two or three words and the decodes above.
constexpr u64 ROW_SHA_FAMILY = 0xFD;
inline PlanRefusal plan_refusal_sha(const u64 *words, const uint32_t *rec_level_ends, const uint32_t *u32_level_ends, const uint32_t *sha_level_ends,
                                    size_t nlevels) {
  if (words[0] == ROW_NO_PROBLEM || (words[0] & 0xFF) != ROW_SHA_FAMILY) return plan_refusal_u32(words, rec_level_ends, u32_level_ends, nlevels);
  const u32 problem = (u32)(words[3] & 0xFF);
  const u64 shifted = words[3] >> 8;
  for (size_t l = 0; l < nlevels; l++)
    if (shifted >= plan_gate(l ? sha_level_ends[l - 1] : 0, l) && shifted < sha_level_ends[l] + plan_shift(l)) return {3, problem, shifted - plan_shift(l)};
  return {3, problem, 0};
}

}  // namespace lcp2
