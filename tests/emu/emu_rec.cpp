// TEST HARNESS (not product code): csrc/rec_rows.hpp compiled for the CPU - the per-job function of k_rec_gate_rows
// (lcp2_rec_gate_rows) and the validation it shares with the host entry point.  A level's launch is emu_plan.cpp's.
// Built by tests/test_rec_rows.py with g++; never loaded by the package.
#include "../../eth-lc-plonky2_amd/csrc/rec_rows.hpp"

using namespace lcp2;

extern "C" {

unsigned emu_rec_job_bytes() { return (unsigned)sizeof(RecJobDev); }
unsigned emu_rec_operand_bytes() { return (unsigned)sizeof(RecOperandDev); }
unsigned emu_rec_row_columns() { return REC_ROW_COLUMNS; }
unsigned emu_rec_kind_ops(unsigned kind) { return rec_kind_ops(kind); }
unsigned emu_rec_kind_operands(unsigned kind, unsigned op) { return rec_kind_operands(kind, op); }
unsigned long long emu_rec_coset_domain(unsigned i) { return rec_coset_domain(i); }
unsigned long long emu_rec_coset_weight(unsigned i) { return rec_coset_weight(i); }
unsigned emu_rec_job_problem(const RecJobDev *job, const RecOperandDev *operands, unsigned long long noperands, unsigned ncols,
                             unsigned long long n) {
  return rec_job_problem(*job, operands, noperands, ncols, n);
}
// the verdict on the value-checked operand of a job whose operands are all IMM (0 when the kind has none)
unsigned emu_rec_value_problem(const RecJobDev *job, const RecOperandDev *operands) {
  const int k = rec_value_operand(job->kind, job->op);
  return k < 0 ? 0 : rec_value_problem(job->kind, gl_canon(operands[job->first_operand + k].v));
}

// the cells of one valid job whose operands are all IMM, in the order the kernel stores them: returns their number
unsigned emu_rec_job_cells(const RecJobDev *job, const RecOperandDev *operands, unsigned *cols, unsigned long long *vals, unsigned cap) {
  unsigned count = 0;
  rec_job_cells(*job, [&](u32 k) { return (u64)operands[job->first_operand + k].v; },
                [&](u32 col, u64 v) {
                  if (count < cap) { cols[count] = col; vals[count] = v; }
                  count++;
                });
  return count;
}

}  // extern "C"
