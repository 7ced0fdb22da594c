// TEST HARNESS (not product code): csrc/u32_rows.hpp compiled for the CPU - the per-job function of k_u32_gate_rows
// (lcp2_u32_gate_rows), the validation it shares with the host entry point, and the kernel's grid as a loop over lanes.
// Built by tests/test_u32_rows.py with g++; never loaded by the package.
#include "../../eth-lc-plonky2_amd/csrc/u32_rows.hpp"

using namespace lcp2;

extern "C" {

unsigned emu_u32_job_bytes() { return (unsigned)sizeof(U32JobDev); }
unsigned emu_u32_row_columns() { return U32_ROW_COLUMNS; }
unsigned emu_u32_kind_ops(unsigned kind) { return u32_kind_ops(kind); }
unsigned emu_u32_job_problem(const U32JobDev *job, unsigned long long n) { return u32_job_problem(*job, n); }

// the cells of one valid job in the order the kernel stores them: returns their number (at most `cap` are recorded)
unsigned emu_u32_job_cells(const U32JobDev *job, unsigned *cols, unsigned long long *vals, unsigned cap) {
  unsigned count = 0;
  u32_job_cells(*job, [&](u32 col, u64 v) {
    if (count < cap) { cols[count] = col; vals[count] = v; }
    count++;
  });
  return count;
}

unsigned long long emu_u32_no_problem() { return ROW_NO_PROBLEM; }
const char *emu_u32_problem_str(unsigned problem) { return u32_problem_str(problem); }

// k_u32_gate_rows over a grid of `blocks` blocks of `threads` lanes, lane by lane; *flag as the kernel keeps it (ROW_NO_PROBLEM
// before the launch)
void emu_u32_gate_rows(const U32JobDev *jobs, unsigned long long njobs, unsigned long long *wires, unsigned long long n,
                       unsigned long long *flag, unsigned blocks, unsigned threads) {
  for (unsigned b = 0; b < blocks; b++)
    for (unsigned t = 0; t < threads; t++) {
      const u64 i = (u64)b * threads + t;
      const u32 problem = u32_rows_lane(jobs, njobs, i, wires, n);
      if (problem && row_refusal(i, problem) < *flag) *flag = row_refusal(i, problem);
    }
}

}  // extern "C"
