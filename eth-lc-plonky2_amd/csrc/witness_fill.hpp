// lcp2_witness_fill_copies as portable text: what the kernels of witness_fill.hip run per routed cell and per listed cell, and what
// tests/emu/emu_fill.cpp runs on the CPU.  plonky2's PartitionWitness::get_full_witness hands the value of a partition's
// representative to every wire of the partition; here the partitions are read back from the sigma columns, once per circuit.
//
// The class table (4 bytes per routed cell: 1.34 GB at n = 2^22 with 80 routed wires; cell = wire * n + row):
//   (a) next[cell]   the cell whose id sigma_wire(w^row) is (wc_decode_cell); a cell that is its own image is seen without a decode.
//                    sigma must be a PERMUTATION of the cells: a value that is no id is refused where it is decoded, and two cells
//                    with one image are found through inv[next[cell]] = the smallest cell with that image (fill_image_shared).
//   (b) label[cell]  the smallest cell of the cycle through `cell`, by pointer jumping: after round k label is the minimum over the 2^k
//                    cells from `cell` on and ptr = next^(2^k).  A round reads only what the round before wrote (ping-pong), so
//                    the result does not depend on the order of the lanes.  A round that lowers no label ends the loop (then every
//                    label is its cycle's minimum: the windows from the points cell + j 2^k cover the whole cycle); 32 rounds
//                    cover every cycle of fewer than 2^32 cells, so the loop is bounded whatever the columns hold.
//   (c) class_of     a cycle of more than one cell is a class, numbered by the rank of its smallest cell among the smallest cells
//                    (roots) of all classes; FILL_NONE for a cell that is its own image.
// A call (fill_owner_lane, fill_broadcast_cell, fill_conflict_lane): the listed cell with the smallest list index owns its class
// (a minimum on owner[class]); every routed cell of an owned class then takes the owner's value FROM THE LIST.  A listed cell marks
// itself in the top bit of its class_of word, so that the broadcast can tell the cells it fills from the ones that were listed; the
// broadcast takes the marks off again.  Conflicts are counted on canonical values in a pass of their own over the list.
#pragma once
#include "row_flag.hpp"
#include "sha_layout.hpp"
#include "witness_check.hpp"

namespace lcp2 {

constexpr u32 FILL_NONE = 0xFFFFFFFFu;    // class_of: in no class; owner: no listed cell; next: the sigma value is no cell id
constexpr u32 FILL_LISTED = 0x80000000u;  // class_of during a call: the cell is in the list (classes hold two cells or more, so their
                                          // numbers stay below 2^31)
constexpr u32 FILL_MAX_ROUNDS = 32;
constexpr u64 FILL_MAX_CELLS = 1ull << 32;  // cell indices and list indices are 32-bit
enum : u32 { FILL_CELL_ROW = 1, FILL_CELL_COLUMN = 2 };   // why a listed cell is refused
enum : u32 { FILL_SIGMA_NO_ID = 1, FILL_SIGMA_SHARED = 2 };  // why the sigma columns are refused
inline const char *fill_cell_problem_str(u32 problem) { return problem == FILL_CELL_ROW ? "row out of range" : "column out of range"; }

// folds: the kernels' atomics, a compare on the CPU
LCP2_HD void fill_fold_min(u32 *word, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(word, v);
#else
  if (v < *word) *word = v;
#endif
}
LCP2_HD void fill_fold_or(u32 *word, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(word, v);
#else
  *word |= v;
#endif
}

// ---- (a) the cell that follows (wire, row); own_id = k_is[wire] w^row.  FILL_NONE: the value is the id of no cell
LCP2_HD u32 fill_next_cell(const WcDecode &t, const u64 *sigmas, u64 n, u32 wire, u64 row, u64 own_id) {
  const u64 s = gl_canon(sigmas[(u64)wire * n + row]);
  if (s == own_id) return (u32)((u64)wire * n + row);
  const WcCell to = wc_decode_cell(t, s);
  return to.wire == WC_NO_WIRE ? FILL_NONE : (u32)((u64)to.wire * n + to.row);
}
// one lane of the decode pass: next[cell], and cell folded into inv[next[cell]] (inv starts as FILL_NONE everywhere).  false: refused
LCP2_HD bool fill_next_lane(const WcDecode &t, const u64 *sigmas, u64 n, u32 wire, u64 row, u64 own_id, u32 *next, u32 *inv) {
  const u32 cell = (u32)((u64)wire * n + row), to = fill_next_cell(t, sigmas, n, wire, row, own_id);
  next[cell] = to;
  if (to == FILL_NONE) return false;
  fill_fold_min(&inv[to], cell);
  return true;
}
// after the whole decode pass: does a smaller cell have the same image?  (the larger of two such cells says so)
LCP2_HD bool fill_image_shared(const u32 *next, const u32 *inv, u32 cell) {
  const u32 to = next[cell];
  return to != FILL_NONE && inv[to] != cell;
}

// ---- (b) one cell of a jumping round; true: its label went down.  The first round reads next alone (label = cell, ptr = next)
LCP2_HD bool fill_jump_first(const u32 *next, u32 *label_out, u32 *ptr_out, u32 cell) {
  const u32 p = next[cell];
  label_out[cell] = p < cell ? p : cell;
  ptr_out[cell] = next[p];
  return p < cell;
}
LCP2_HD bool fill_jump_cell(const u32 *label_in, const u32 *ptr_in, u32 *label_out, u32 *ptr_out, u32 cell) {
  const u32 p = ptr_in[cell], mine = label_in[cell], ahead = label_in[p];
  label_out[cell] = ahead < mine ? ahead : mine;
  ptr_out[cell] = ptr_in[p];
  return ahead < mine;
}

// ---- (c) the smallest cell of a class; rank[cell] = the roots below `cell`; the class of a cell
LCP2_HD bool fill_is_root(const u32 *label, const u32 *next, u32 cell) { return label[cell] == cell && next[cell] != cell; }
// class_of and next may be one array: a lane reads next at its own cell only, before it writes
LCP2_HD void fill_number_cell(const u32 *label, const u32 *rank, const u32 *next, u32 *class_of, u32 cell) {
  const bool alone = next[cell] == cell;
  class_of[cell] = alone ? FILL_NONE : rank[label[cell]];
}

// ---- a call
LCP2_HD u32 fill_cell_problem(const CellDev &c, u64 n, u32 num_wires) {
  if (c.row >= n) return FILL_CELL_ROW;
  if (c.col >= num_wires) return FILL_CELL_COLUMN;
  return 0;
}
// the index of the first refused cell of a host list and why; ncells when there is none
inline size_t fill_cells_problem(const CellDev *cells, size_t ncells, u64 n, u32 num_wires, u32 *problem) {
  for (size_t i = 0; i < ncells; i++)
    if ((*problem = fill_cell_problem(cells[i], n, num_wires)) != 0) return i;
  return ncells;
}
// the class of a valid listed cell, FILL_NONE when it is in none (a non-routed wire, its own image)
LCP2_HD u32 fill_class_of_listed(const CellDev &c, const u32 *class_of, u64 n, u32 num_routed) {
  if (c.col >= num_routed) return FILL_NONE;
  const u32 cls = class_of[(u64)c.col * n + c.row];
  return cls == FILL_NONE ? FILL_NONE : cls & ~FILL_LISTED;
}
// lane i of the owner pass: the plain store of entry i, its index folded into owner[class], its mark.  Returns 0, or the problem
// of an entry that is refused and has done nothing
LCP2_HD u32 fill_owner_lane(const CellDev *cells, u64 ncells, u64 i, u32 *class_of, u32 *owner, u64 *wires, u64 n, u32 num_wires, u32 num_routed) {
  if (i >= ncells) return 0;
  const CellDev c = cells[i];
  if (const u32 problem = fill_cell_problem(c, n, num_wires)) return problem;
  const u64 at = (u64)c.col * n + c.row;
  wires[at] = c.value;
  const u32 cls = fill_class_of_listed(c, class_of, n, num_routed);
  if (cls != FILL_NONE) {
    fill_fold_min(&owner[cls], (u32)i);
    fill_fold_or(&class_of[at], FILL_LISTED);
  }
  return 0;
}
// one routed cell after the whole owner pass: the owner's value as the list holds it, and the mark taken off.  Returns 1 for a cell
// that received the value without being listed.  A cell of a class nobody owns is neither read nor written
LCP2_HD u32 fill_broadcast_cell(const CellDev *cells, u32 *class_of, const u32 *owner, u64 *wires, u32 cell) {
  const u32 raw = class_of[cell];
  if (raw == FILL_NONE) return 0;
  const u32 o = owner[raw & ~FILL_LISTED];
  if (o == FILL_NONE) return 0;  // (then no cell of the class carries a mark)
  if (raw & FILL_LISTED) class_of[cell] = raw & ~FILL_LISTED;
  wires[cell] = cells[o].value;
  return raw & FILL_LISTED ? 0 : 1;
}
// entry i against its class's owner: 0 nothing to report, FILL_IS_OWNER it is the owner, FILL_CONFLICT its canonical value differs
enum : u32 { FILL_IS_OWNER = 1, FILL_CONFLICT = 2 };
LCP2_HD u32 fill_conflict_lane(const CellDev *cells, u64 ncells, u64 i, const u32 *class_of, const u32 *owner, u64 n, u32 num_wires, u32 num_routed) {
  if (i >= ncells) return 0;
  const CellDev c = cells[i];
  if (fill_cell_problem(c, n, num_wires)) return 0;
  const u32 cls = fill_class_of_listed(c, class_of, n, num_routed);
  if (cls == FILL_NONE) return 0;
  const u32 o = owner[cls];
  if (o == (u32)i) return FILL_IS_OWNER;
  return gl_canon(cells[o].value) != gl_canon(c.value) ? FILL_CONFLICT : 0;
}

}  // namespace lcp2
