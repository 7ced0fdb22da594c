// lcp2_witness_settle_copies as portable text: what the k_settle_* kernels of witness_fill.hip run per listed source and per routed
// cell, and what tests/emu/emu_settle.cpp runs on the CPU.  The class table, the owner words and the marks are those of
// witness_fill.hpp; what differs is where a class's value comes from: the list holds cells only (row, col), and the value is the word
// the MATRIX holds at the owner's cell (plonky2: PartitionWitness::get_full_witness after the generators have run on the device).
//
// The values live in the array that is written, so the ORDER OF THE PASSES is what makes the result independent of the lane order:
//   (1) settle_owner_lane     over the list.  Reads the list and class_of, folds into owner[] and marks class_of.  The matrix is
//                             neither read nor written.
//   (2) settle_conflict_lane  over the list, after ALL of (1): owner[] is final.  Reads the matrix (the source's cell and its owner's
//                             cell), writes nothing but the counts.
//   (3) settle_broadcast_cell over the routed cells, after ALL of (2).  The only pass that stores to the matrix.  A lane reads the
//                             matrix at the OWNER'S CELL of its own class only, and stores to its own cell only when that is NOT the
//                             owner's cell.  Every class has one owner cell (owner[] is final, and a cell listed twice is one cell),
//                             every cell is in one class, so the words read in this launch (the owner cells of the owned classes) and
//                             the words written in it (the other cells of those classes) are disjoint sets: no lane reads a word
//                             that another lane of the same launch writes, and no scratch copy of the values is needed.
// (2) runs before (3) because it compares the words the matrix held when the call began; after (3) a conflicting source holds its
// owner's word.  The first-conflict lookup reads the list and owner[] only and may run at any time after (2).
#pragma once
#include "witness_fill.hpp"

namespace lcp2 {

struct CellRefDev {  // = lcp2_cell_ref
  uint32_t row, col;
};

LCP2_HD u32 fill_cell_problem(const CellRefDev &c, u64 n, u32 num_wires) {
  if (c.row >= n) return FILL_CELL_ROW;
  if (c.col >= num_wires) return FILL_CELL_COLUMN;
  return 0;
}
// the index of the first refused source of a host list and why; nsources when there is none
inline size_t fill_cells_problem(const CellRefDev *refs, size_t nsources, u64 n, u32 num_wires, u32 *problem) {
  for (size_t i = 0; i < nsources; i++)
    if ((*problem = fill_cell_problem(refs[i], n, num_wires)) != 0) return i;
  return nsources;
}
// the class of a valid source, FILL_NONE when it is in none (a non-routed wire, its own image)
LCP2_HD u32 settle_class_of_source(const CellRefDev &c, const u32 *class_of, u64 n, u32 num_routed) {
  if (c.col >= num_routed) return FILL_NONE;
  const u32 cls = class_of[(u64)c.col * n + c.row];
  return cls == FILL_NONE ? FILL_NONE : cls & ~FILL_LISTED;
}
// (1) lane i: its index folded into owner[class], its mark.  Returns 0, or the problem of an entry that is refused and has done
// nothing.  No access to the matrix
LCP2_HD u32 settle_owner_lane(const CellRefDev *refs, u64 nsources, u64 i, u32 *class_of, u32 *owner, u64 n, u32 num_wires, u32 num_routed) {
  if (i >= nsources) return 0;
  const CellRefDev c = refs[i];
  if (const u32 problem = fill_cell_problem(c, n, num_wires)) return problem;
  const u32 cls = settle_class_of_source(c, class_of, n, num_routed);
  if (cls != FILL_NONE) {
    fill_fold_min(&owner[cls], (u32)i);
    fill_fold_or(&class_of[(u64)c.col * n + c.row], FILL_LISTED);
  }
  return 0;
}
// (2) source i against its class's owner, on the canonical words of the matrix: 0, FILL_IS_OWNER or FILL_CONFLICT
LCP2_HD u32 settle_conflict_lane(const CellRefDev *refs, u64 nsources, u64 i, const u32 *class_of, const u32 *owner, const u64 *wires, u64 n, u32 num_wires,
                                 u32 num_routed) {
  if (i >= nsources) return 0;
  const CellRefDev c = refs[i];
  if (fill_cell_problem(c, n, num_wires)) return 0;
  const u32 cls = settle_class_of_source(c, class_of, n, num_routed);
  if (cls == FILL_NONE) return 0;
  const u32 o = owner[cls];
  if (o == (u32)i) return FILL_IS_OWNER;
  const CellRefDev oc = refs[o];
  return gl_canon(wires[(u64)oc.col * n + oc.row]) != gl_canon(wires[(u64)c.col * n + c.row]) ? FILL_CONFLICT : 0;
}
// (3) one routed cell: the word at the owner's cell of its class, unless it is that cell; the mark taken off.  Returns 1 for a cell
// of an owned class that was not listed.  A cell of a class nobody owns is neither read nor written
LCP2_HD u32 settle_broadcast_cell(const CellRefDev *refs, u32 *class_of, const u32 *owner, u64 *wires, u64 n, u32 cell) {
  const u32 raw = class_of[cell];
  if (raw == FILL_NONE) return 0;
  const u32 o = owner[raw & ~FILL_LISTED];
  if (o == FILL_NONE) return 0;  // (then no cell of the class carries a mark)
  if (raw & FILL_LISTED) class_of[cell] = raw & ~FILL_LISTED;
  const CellRefDev oc = refs[o];
  const u64 from = (u64)oc.col * n + oc.row;
  if (from != cell) wires[cell] = wires[from];
  return raw & FILL_LISTED ? 0 : 1;
}

}  // namespace lcp2
