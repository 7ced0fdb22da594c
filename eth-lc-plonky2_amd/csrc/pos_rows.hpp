// One PoseidonGate row, from its 12 inputs and its swap flag to every cell of the row (lcp2_poseidon_gate_rows).
//
// plonky2 gates/poseidon.rs PoseidonGenerator::run_once as ONE function: inputs in, (column, value) pairs out through a store
// callback.  k_poseidon_gate_rows (kernels_witness.hip) calls it with a store into the column-major witness matrix,
// lcp2_poseidon_gate_rows (witness_rows.hip) validates its list with pos_row_problem, poseidon_gate_row (host/poseidon_host.cpp)
// calls it with a store into a row of its own, and tests/emu/emu_pos.cpp compiles the same text for the CPU.  The wire layout is
// the one host/gates.cpp and kernels_quotient.hip q_poseidon_native read; poseidon_py.py gate_row states the row in Python.
// Every value written is canonical: the inputs are reduced when they are read and the state is reduced after every layer.
#pragma once
#include "poseidon.hpp"

namespace lcp2 {

constexpr uint32_t POS_WIRE_INPUT = 0, POS_WIRE_OUTPUT = 12, POS_WIRE_SWAP = 24, POS_WIRE_DELTA = 25, POS_WIRE_FULL_0 = 29,
                   POS_WIRE_PARTIAL = 65, POS_WIRE_FULL_1 = 87, POS_GATE_WIRES = 135;
// what enters S-box i of full round `round`: of the first half (rounds 1..3; round 0 takes the inputs), of the second half (0..3)
constexpr uint32_t pos_wire_full_sbox_0(uint32_t round, uint32_t i) { return POS_WIRE_FULL_0 + 12 * (round - 1) + i; }
constexpr uint32_t pos_wire_full_sbox_1(uint32_t round, uint32_t i) { return POS_WIRE_FULL_1 + 12 * round + i; }

struct PoseidonRowDev {  // = lcp2_poseidon_row
  uint32_t row, swap;
  unsigned long long in[12];
};

// 0: the job may run; otherwise why lcp2_poseidon_gate_rows refuses its list (1: row out of range, 2: swap flag not boolean)
LCP2_HD u32 pos_row_problem(const PoseidonRowDev &j, u64 n) {
  if (j.row >= n) return 1;
  if (j.swap > 1) return 2;
  return 0;
}

// Every cell of the row, columns 0 .. POS_GATE_WIRES - 1, each once: put(column, canonical value).  The permutation in its plain
// round form (constants, S-box, MDS), recording what enters every S-box that has a wire; the value entering lane 0's S-box in a
// partial round is the same in plonky2's fast-partial-round refactoring.  in: any u64; rc: the 360 round constants, canonical;
// mds(s): the MDS layer in place, lazy values out (pos_mds, or a host's vector form of it).
template <class Mds, class Put>
LCP2_HD void pos_row_cells(const u64 in[12], bool swap, const u64 *rc, Mds mds, Put put) {
  u64 s[12];
#pragma unroll
  for (int j = 0; j < 12; j++) { s[j] = gl_canon(in[j]); put(POS_WIRE_INPUT + j, s[j]); }
  put(POS_WIRE_SWAP, swap ? 1 : 0);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const u64 delta = swap ? gl_sub(s[j + 4], s[j]) : 0;
    put(POS_WIRE_DELTA + j, delta);
    const u64 l = gl_add(s[j], delta), r = gl_sub(s[j + 4], delta);
    s[j] = l; s[j + 4] = r;
  }
#pragma unroll 1
  for (int round = 0; round < POS_ROUNDS; round++) {
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = gl_add(s[j], rc[12 * round + j]);
    const bool full = round < POS_FULL_HALF || round >= POS_FULL_HALF + POS_PARTIAL;
    if (full) {
#pragma unroll
      for (int j = 0; j < 12; j++) {
        if (round >= 1 && round < POS_FULL_HALF) put(pos_wire_full_sbox_0(round, j), s[j]);
        if (round >= POS_FULL_HALF + POS_PARTIAL) put(pos_wire_full_sbox_1(round - POS_FULL_HALF - POS_PARTIAL, j), s[j]);
        s[j] = gl_canon(pos_sbox(s[j]));
      }
    } else {
      put(POS_WIRE_PARTIAL + (round - POS_FULL_HALF), s[0]);
      s[0] = gl_canon(pos_sbox(s[0]));
    }
    mds(s);
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = gl_canon(s[j]);
  }
#pragma unroll
  for (int j = 0; j < 12; j++) put(POS_WIRE_OUTPUT + j, s[j]);
}

// lane i of k_poseidon_gate_rows: the list is a host list that passed pos_row_problem, so the lane checks nothing but its index
LCP2_HD void pos_rows_lane(const PoseidonRowDev *rows, u64 nrows, u64 i, u64 *wires, u64 n, const u64 *rc) {
  if (i >= nrows) return;
  const PoseidonRowDev job = rows[i];
  u64 *W = wires + job.row;
  pos_row_cells(job.in, job.swap != 0, rc, [](u64 *s) { pos_mds(s); }, [&](u32 col, u64 v) { W[(u64)col * n] = v; });
}

}  // namespace lcp2
