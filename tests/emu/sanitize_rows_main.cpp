// TEST HARNESS (not product code): emu_rows.cpp under ASan + UBSan as a stand-alone program, linked against nothing else
// (built like its siblings: g++ -O1 -g -std=c++17 -fsanitize=address,undefined tests/emu/sanitize_rows_main.cpp).
// A 2^3-row layout with 5 routed wires, three gates in two selector columns and one gate constant, every array in a heap block of
// exactly its size: random binding lists over sparse class ids under several tilings and both lane orders must give one matrix,
// every cell's sigma chain must come back to the cell after exactly the size of its class, and refused lists must name their index
// without a read or a write outside the blocks.
#include <map>
#include <vector>
#include "emu_rows.cpp"
#include "sanitize_common.hpp"

int main() {
  lcp2_circuit_desc desc = {};
  lcp2_params &p = desc.params;
  p.degree_bits = 3; p.num_wires = 9; p.num_routed_wires = 5; p.num_constants = 3;
  const u64 n = 8;
  const u32 NR = 5, NC = 3;
  lcp2_gate gates[3] = {{0, 0, 0, 2, 0, 0, 0, 0}, {0, 1, 0, 2, 0, 0, 0, 0}, {1, 2, 2, 3, 0, 0, 0, 0}};
  std::vector<u64> k_is(NR);
  u64 acc = 1;
  for (u64 &k : k_is) { k = acc; acc = gl_mul(acc, 7); }
  desc.k_is = (const uint64_t *)k_is.data(); desc.num_selectors = 2; desc.num_gates = 3; desc.gates = gates;
  std::vector<uint32_t> gate_of_row = {2, 1, 1, 0, 2, 1};  // rows 6, 7: pad_gate
  std::vector<u64> consts(gate_of_row.size());
  for (u64 &c : consts) c = rnd();
  u32 rounds = 0;
  for (u32 trial = 0; trial < 24; trial++) {
    // a random subset of the 40 cells in random order, class ids drawn from a few sparse values
    std::vector<u32> cells(NR * n);
    for (u32 i = 0; i < cells.size(); i++) cells[i] = i;
    for (u32 i = (u32)cells.size() - 1; i > 0; i--) std::swap(cells[i], cells[rnd() % (i + 1)]);
    const u32 M = trial == 0 ? 0 : 1 + (u32)(rnd() % cells.size());
    const u32 num_classes = trial % 3 == 0 ? 1 : trial % 3 == 1 ? 37 : 0x80000001u;
    const u32 ids[4] = {0, num_classes / 2, num_classes - 1, num_classes / 3};
    std::vector<lcp2_copy_binding> list(M);
    std::map<u32, u32> size_of;
    for (u32 i = 0; i < M; i++) { list[i] = {cells[i] % (u32)n, cells[i] / (u32)n, ids[rnd() % 4]}; size_of[list[i].cls]++; }
    lcp2_circuit_rows rows = {gate_of_row.data(), gate_of_row.size(), 0, (const uint64_t *)consts.data(), list.data(), M, LCP2_MEM_HOST, num_classes};
    const char *why = nullptr;
    CHECK(emu_rows_args(&desc, &rows, &why) == 0 && !why);
    std::vector<u64> first((NC + NR) * n), again((NC + NR) * n);
    u64 info[6];
    CHECK(emu_rows_expand(&desc, &rows, 256, 8, 0, first.data(), info) == 0);
    const unsigned tilings[3][3] = {{1, 1, 1}, {3, 2, 0}, {2, 5, 1}};
    for (const auto &t : tilings) {
      CHECK(emu_rows_expand(&desc, &rows, t[0], t[1], (int)t[2], again.data(), info) == 0);
      CHECK(first == again);
    }
    // selector and constant columns
    for (u64 r = 0; r < n; r++) {
      const u32 g = r < gate_of_row.size() ? gate_of_row[r] : 0;
      CHECK(first[gates[g].selector_index * n + r] == gates[g].selector_value && first[(1 - gates[g].selector_index) * n + r] == 0xFFFFFFFFull);
      CHECK(first[2 * n + r] == (r < consts.size() ? consts[r] : 0));
    }
    // every bound cell's chain closes after exactly its class's size, every other cell is its own image
    std::map<u64, u32> cell_of_id;
    Roots R(p.degree_bits);
    for (u32 c = 0; c < NR * n; c++) cell_of_id[rows_cell_id(k_is.data(), R.t, c / (u32)n, c % n)] = c;
    std::vector<int> cls_of(NR * n, -1);
    for (u32 i = 0; i < M; i++) cls_of[list[i].col * n + list[i].row] = (int)i;
    for (u32 c = 0; c < NR * n; c++) {
      u32 at = c, steps = 0;
      do {
        CHECK(cell_of_id.count(first[NC * n + at]));
        at = cell_of_id[first[NC * n + at]];
        steps++;
      } while (at != c && steps <= M);
      CHECK(at == c && steps == (cls_of[c] < 0 ? 1 : size_of[list[cls_of[c]].cls]));
    }
    rounds++;
  }
  {  // refusals: an entry out of range in each field, a cell bound twice, a gate index out of range
    std::vector<lcp2_copy_binding> list = {{1, 1, 0}, {2, 2, 1}, {8, 0, 0}, {0, 5, 0}, {0, 0, 2}};
    lcp2_circuit_rows rows = {gate_of_row.data(), gate_of_row.size(), 0, nullptr, list.data(), list.size(), LCP2_MEM_HOST, 2};
    std::vector<u64> out((NC + NR) * n);
    u64 info[6];
    CHECK(emu_rows_expand(&desc, &rows, 2, 2, 1, out.data(), info) == LCP2_E_INVALID && info[0] == row_refusal(2, ROWS_BIND_ROW));
    list = {{1, 1, 0}, {2, 2, 1}, {2, 2, 0}, {1, 1, 1}};
    rows.bindings = list.data(); rows.num_bindings = list.size();
    CHECK(emu_rows_expand(&desc, &rows, 2, 2, 0, out.data(), info) == LCP2_E_INVALID && info[0] == ROW_NO_PROBLEM && info[2] == 0 && info[3] == 3);
    std::vector<uint32_t> bad = gate_of_row;
    bad[3] = 3;
    rows.gate_of_row = bad.data(); rows.num_bindings = 2;
    CHECK(emu_rows_expand(&desc, &rows, 2, 2, 0, out.data(), info) == LCP2_E_INVALID && info[1] == row_refusal(3, ROWS_GATE));
    const char *why = nullptr;
    rows.pad_gate = 3;
    CHECK(emu_rows_args(&desc, &rows, &why) == LCP2_E_INVALID && why);
  }
  printf("sanitize_rows: %u random lists over 40 cells under 4 tilings, chains closed, 4 refusals: ok\n", rounds);
  return 0;
}
