// TEST HARNESS (not product code): csrc/witness_settle.hpp compiled for the CPU - the three passes of lcp2_witness_settle_copies
// (owner, conflicts, broadcast) over host arrays, each pass complete before the next as the launches are, and within a pass block by
// block under a TILING: `tile` lanes per block, the blocks from the first to the last or (`reverse`) from the last to the first and
// the lanes of a block likewise.  No tiling may change the matrix or the report.  The class table comes from emu_fill.cpp's
// emu_fill_classes or from the model.  tests/test_settle_copies_emu.py holds the results to circuit.settle_copies_model.  Built by
// tests/rows_lib.py build_emu with g++; never loaded by the package.
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/witness_settle.hpp"

using namespace lcp2;

namespace {
// lanes 0 .. count - 1 in blocks of `tile`
template <class F>
void tiled(u64 count, u64 tile, int reverse, F f) {
  const u64 blocks = (count + tile - 1) / tile;
  for (u64 b = 0; b < blocks; b++) {
    const u64 block = reverse ? blocks - 1 - b : b;
    for (u64 k = 0; k < tile; k++) f(block * tile + (reverse ? tile - 1 - k : k));  // lanes past the end run too, as on the device
  }
}
}  // namespace

extern "C" {
// a call on a host matrix wires [num_wires][n].  report: the six words of lcp2_fill_report; *flag: the refusal word (ROW_NO_PROBLEM, or
// row_refusal(first refused entry, why)).  class_of is given back without marks.  host_list: validate first, change nothing if refused
void emu_settle_copies(uint32_t *class_of, u64 num_classes, u64 n, unsigned num_wires, unsigned num_routed, const CellRefDev *refs, u64 nsources,
                       int host_list, u64 *wires, u64 *report, u64 *flag, u64 tile, int reverse) {
  *flag = ROW_NO_PROBLEM;
  report[0] = num_classes; report[1] = report[2] = report[3] = 0; report[4] = report[5] = ~0ull;
  if (host_list) {
    u32 problem = 0;
    const size_t at = fill_cells_problem(refs, nsources, n, num_wires, &problem);
    if (at != nsources) { *flag = row_refusal(at, problem); return; }
  }
  std::vector<u32> owner(num_classes, FILL_NONE);
  tiled(nsources, tile, reverse, [&](u64 i) {
    if (const u32 problem = settle_owner_lane(refs, nsources, i, class_of, owner.data(), n, num_wires, num_routed))
      if (row_refusal(i, problem) < *flag) *flag = row_refusal(i, problem);
  });
  tiled(nsources, tile, reverse, [&](u64 i) {
    const u32 what = settle_conflict_lane(refs, nsources, i, class_of, owner.data(), wires, n, num_wires, num_routed);
    if (what == FILL_IS_OWNER) report[1]++;
    if (what == FILL_CONFLICT) { report[3]++; if (i < report[4]) report[4] = i; }
  });
  if (report[4] != ~0ull) report[5] = owner[settle_class_of_source(refs[report[4]], class_of, n, num_routed)];
  const u64 routed = (u64)num_routed * n;
  tiled(routed, tile, reverse, [&](u64 cell) {
    if (cell < routed) report[2] += settle_broadcast_cell(refs, class_of, owner.data(), wires, n, (u32)cell);
  });
}
}
