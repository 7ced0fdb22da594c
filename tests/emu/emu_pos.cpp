// TEST HARNESS (not product code): csrc/pos_rows.hpp compiled for the CPU - the row function of k_poseidon_gate_rows
// (lcp2_poseidon_gate_rows), the validation of the entry point, and the kernel's grid as a loop over lanes.
// Built by tests/test_pos_rows.py with g++; never loaded by the package.
#include "../../eth-lc-plonky2_amd/csrc/pos_rows.hpp"
#include "emu_rc.hpp"

using namespace lcp2;

extern "C" {

unsigned emu_pos_row_bytes() { return (unsigned)sizeof(PoseidonRowDev); }
unsigned emu_pos_gate_wires() { return POS_GATE_WIRES; }
unsigned emu_pos_row_problem(const PoseidonRowDev *job, unsigned long long n) { return pos_row_problem(*job, n); }

// the cells of one job in the order the kernel stores them: returns their number (at most `cap` are recorded)
unsigned emu_pos_row_cells(const PoseidonRowDev *job, unsigned *cols, unsigned long long *vals, unsigned cap) {
  unsigned count = 0;
  pos_row_cells(job->in, job->swap != 0, emu_round_constants(), [](u64 *s) { pos_mds(s); }, [&](u32 col, u64 v) {
    if (count < cap) { cols[count] = col; vals[count] = v; }
    count++;
  });
  return count;
}

// k_poseidon_gate_rows over a grid of `blocks` blocks of `threads` lanes, lane by lane
void emu_pos_gate_rows(const PoseidonRowDev *rows, unsigned long long nrows, unsigned long long *wires, unsigned long long n,
                       unsigned blocks, unsigned threads) {
  for (unsigned b = 0; b < blocks; b++)
    for (unsigned t = 0; t < threads; t++) pos_rows_lane(rows, nrows, (u64)b * threads + t, wires, n, emu_round_constants());
}

}  // extern "C"
