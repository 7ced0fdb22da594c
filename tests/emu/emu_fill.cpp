// TEST HARNESS (not product code): csrc/witness_fill.hpp compiled for the CPU - the decode pass with its permutation check, the
// pointer-jumping rounds on ping-pong arrays, the numbering, and the three passes of a call (owner, broadcast, conflicts) - lane by
// lane in the order the entry points launch them; `reverse` runs the lanes of every pass from the last to the first, which must
// change nothing.  tests/test_fill_copies_emu.py holds the results to the numpy model of eth-lc-plonky2_amd/circuit.py.  Built by
// tests/rows_lib.py build_emu with g++; never loaded by the package.
#include <cstring>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/witness_fill.hpp"
#include "../../eth-lc-plonky2_amd/csrc/ntt_host.hpp"

using namespace lcp2;

namespace {
struct Roots {
  std::vector<u64> lo, hi, tab;
  WcDecode t;
  Roots(const u64 *k_is, u32 num_routed, u32 lg) : tab(2 * (size_t)num_routed) {
    t.roots.h = (lg + 1) / 2;
    const u64 w = gl_root_of_unity(lg);
    lo = make_pow_table(w, 1, (size_t)1 << t.roots.h);
    hi = make_pow_table(w, 1ull << t.roots.h, (size_t)1 << (lg - t.roots.h));
    t.roots.lo = lo.data(); t.roots.hi = hi.data();
    wc_decode_tables(k_is, num_routed, lg, tab.data());
    t.kn = tab.data(); t.kinv = tab.data() + num_routed; t.num_routed = num_routed; t.degree_bits = lg;
  }
};
// lanes 0 .. count - 1, or the other way round
template <class F>
void lanes(u64 count, int reverse, F f) {
  for (u64 k = 0; k < count; k++) f(reverse ? count - 1 - k : k);
}
}  // namespace

extern "C" {
// d: lcp2_circuit_desc with host constants_sigmas.  class_of [num_routed][n]; out[0] = classes, out[1] = rounds that lowered a label,
// out[2] = the refused cell, out[3] = the other cell with its image (FILL_SIGMA_SHARED).  Returns 0, or FILL_SIGMA_* when the sigma
// columns are refused (class_of is then not written)
int emu_fill_classes(const lcp2_circuit_desc *d, uint32_t *class_of, u64 *out, int reverse) {
  const lcp2_params &p = d->params;
  const u64 n = 1ull << p.degree_bits;
  const u32 NR = p.num_routed_wires;
  const u64 cells = (u64)NR * n;
  if (cells >= FILL_MAX_CELLS) return -1;
  const u64 *k_is = (const u64 *)d->k_is;
  Roots R(k_is, NR, p.degree_bits);
  const u64 *sigmas = (const u64 *)d->constants_sigmas + (u64)p.num_constants * n;
  std::vector<u32> next(cells), L[2] = {std::vector<u32>(cells), std::vector<u32>(cells, FILL_NONE)}, P[2] = {std::vector<u32>(cells), std::vector<u32>(cells)};
  u32 *inv = L[1].data();
  u64 flag = ROW_NO_PROBLEM;
  lanes(cells, reverse, [&](u64 cell) {
    const u32 wire = (u32)(cell / n);
    const u64 row = cell % n;
    if (!fill_next_lane(R.t, sigmas, n, wire, row, gl_mul(gl_canon(k_is[wire]), two_level(R.t.roots, row)), next.data(), inv))
      if (row_refusal(cell, FILL_SIGMA_NO_ID) < flag) flag = row_refusal(cell, FILL_SIGMA_NO_ID);
  });
  lanes(cells, reverse, [&](u64 cell) {
    if (fill_image_shared(next.data(), inv, (u32)cell) && row_refusal(cell, FILL_SIGMA_SHARED) < flag) flag = row_refusal(cell, FILL_SIGMA_SHARED);
  });
  out[0] = out[1] = 0; out[2] = out[3] = ~0ull;
  if (flag != ROW_NO_PROBLEM) {
    out[2] = flag >> 8;
    if ((flag & 0xFF) == FILL_SIGMA_SHARED) out[3] = inv[next[flag >> 8]];
    return (int)(flag & 0xFF);
  }
  u32 rounds = 0, last = 0;
  for (u32 r = 0; r < FILL_MAX_ROUNDS; r++) {
    last = r & 1;
    bool changed = false;
    lanes(cells, reverse, [&](u64 cell) {
      if (r == 0 ? fill_jump_first(next.data(), L[0].data(), P[0].data(), (u32)cell)
                 : fill_jump_cell(L[last ^ 1].data(), P[last ^ 1].data(), L[last].data(), P[last].data(), (u32)cell))
        changed = true;
    });
    if (!changed) break;
    rounds++;
  }
  const u32 *label = L[last].data();
  u32 *rank = P[last].data(), running = 0;
  for (u64 cell = 0; cell < cells; cell++)
    if (fill_is_root(label, next.data(), (u32)cell)) rank[cell] = running++;
  memcpy(class_of, next.data(), cells * 4);  // the numbering overwrites next in place, as on the device
  lanes(cells, reverse, [&](u64 cell) { fill_number_cell(label, rank, class_of, class_of, (u32)cell); });
  out[0] = running; out[1] = rounds;
  return 0;
}

// a call on a host matrix wires [num_wires][n].  report: the six words of lcp2_fill_report; *flag: the refusal word (ROW_NO_PROBLEM, or
// row_refusal(first refused entry, why)).  class_of is given back without marks.  host_list: validate first, write nothing if refused
void emu_fill_copies(uint32_t *class_of, u64 num_classes, u64 n, unsigned num_wires, unsigned num_routed, const CellDev *cells, u64 ncells,
                     int host_list, u64 *wires, u64 *report, u64 *flag, int reverse) {
  *flag = ROW_NO_PROBLEM;
  report[0] = num_classes; report[1] = report[2] = report[3] = 0; report[4] = report[5] = ~0ull;
  if (host_list) {
    u32 problem = 0;
    const size_t at = fill_cells_problem(cells, ncells, n, num_wires, &problem);
    if (at != ncells) { *flag = row_refusal(at, problem); return; }
  }
  std::vector<u32> owner(num_classes, FILL_NONE);
  lanes(ncells, reverse, [&](u64 i) {
    if (const u32 problem = fill_owner_lane(cells, ncells, i, class_of, owner.data(), wires, n, num_wires, num_routed))
      if (row_refusal(i, problem) < *flag) *flag = row_refusal(i, problem);
  });
  lanes((u64)num_routed * n, reverse, [&](u64 cell) { report[2] += fill_broadcast_cell(cells, class_of, owner.data(), wires, (u32)cell); });
  lanes(ncells, reverse, [&](u64 i) {
    const u32 what = fill_conflict_lane(cells, ncells, i, class_of, owner.data(), n, num_wires, num_routed);
    if (what == FILL_IS_OWNER) report[1]++;
    if (what == FILL_CONFLICT) { report[3]++; if (i < report[4]) report[4] = i; }
  });
  if (report[4] != ~0ull) report[5] = owner[fill_class_of_listed(cells[report[4]], class_of, n, num_routed)];
}
}
