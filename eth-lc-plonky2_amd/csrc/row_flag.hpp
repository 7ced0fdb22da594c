// The refusal flag of the row generators that validate a job list on the device (lcp2_u32_gate_rows, lcp2_rec_gate_rows).
//
// One 64-bit word per call.  The entry point sets it to ROW_NO_PROBLEM before the first launch; a lane whose job is refused writes
// no cell and folds row_refusal(index, problem) into the word with a minimum (the kernels: atomicMin; tests/emu: a compare), so
// after the last launch the word names the FIRST refused job of the list and why (u32_problem_str / rec_problem_str), whatever
// the order the lanes ran in.  The entry point reads it back once (witness_rows.hip RefusalFlag).
#pragma once
#include "gl64.hpp"

namespace lcp2 {

constexpr u64 ROW_NO_PROBLEM = ~0ull;  // no job of the call has been refused
LCP2_HD u64 row_refusal(u64 index, u64 problem) { return index << 8 | problem; }  // problem in [1, 255]

}  // namespace lcp2
