// TEST HARNESS (not product code): emu_settle.cpp under ASan + UBSan as a stand-alone program, linked against nothing else:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_settle tests/emu/sanitize_settle_main.cpp && /tmp/emu_sanitize_settle
// Hand-made cycles on a 5-wire matrix of 7 rows with 3 routed wires, every array sized exactly (a read past a list, the table, the
// owner words or the matrix is a heap overflow): one source per class into a scrambled matrix, a partial list, a conflict in both
// list orders, v against v + p, a source on a non-routed wire and one in no class, a cell listed twice, a refused entry in a host and
// in a device list, an empty list - each under four tilings, which must agree word for word.
#include <vector>
#include "emu_settle.cpp"
#include "sanitize_common.hpp"

namespace {
constexpr u64 N = 7, NONE = ROW_NO_PROBLEM;
constexpr unsigned W = 5, NR = 3;
struct Cell { u32 col, row; };
// three classes, numbered by their smallest cell (col * N + row): 0 = {(0,0), (2,6), (1,3)}, 1 = {(0,2), (0,5)},
// 2 = {(1,0), (1,1), (1,2), (2,0), (2,1)}; every other routed cell is its own image
const std::vector<std::vector<Cell>> CLASSES = {{{0, 0}, {2, 6}, {1, 3}}, {{0, 2}, {0, 5}}, {{1, 0}, {1, 1}, {1, 2}, {2, 0}, {2, 1}}};
std::vector<uint32_t> table() {
  std::vector<uint32_t> t(NR * N, FILL_NONE);
  for (size_t k = 0; k < CLASSES.size(); k++)
    for (const Cell &c : CLASSES[k]) t[c.col * N + c.row] = (uint32_t)k;
  return t;
}
struct Result {
  std::vector<u64> wires, report;
  u64 flag;
  bool operator==(const Result &o) const { return wires == o.wires && report == o.report && flag == o.flag; }
};
// the call under four tilings; false if they differ or a mark is left in the table
bool settle(const std::vector<CellRefDev> &refs, int host_list, const std::vector<u64> &start, Result *out) {
  const std::vector<uint32_t> clean = table();
  const struct { u64 tile; int reverse; } tilings[4] = {{256, 0}, {1, 0}, {2, 1}, {3, 0}};
  for (int k = 0; k < 4; k++) {
    Result r{start, std::vector<u64>(6), 0};
    std::vector<uint32_t> t = clean;
    std::vector<CellRefDev> list = refs;  // a copy sized exactly
    list.shrink_to_fit();
    emu_settle_copies(t.data(), CLASSES.size(), N, W, NR, list.data(), list.size(), host_list, r.wires.data(), r.report.data(), &r.flag, tilings[k].tile,
                      tilings[k].reverse);
    if (t != clean) return false;
    if (k == 0) *out = r;
    else if (!(r == *out)) return false;
  }
  return true;
}
}  // namespace

int main() {
  std::vector<u64> witness(W * N);
  for (auto &x : witness) x = rnd();
  for (const auto &cls : CLASSES)
    for (const Cell &c : cls) witness[c.col * N + c.row] = witness[cls[0].col * N + cls[0].row];
  auto at = [](Cell c) { return c.col * N + c.row; };
  Result r;
  // ---- one source per class (not the smallest cell), every other cell of every class scrambled: the witness comes back
  {
    std::vector<u64> m = witness;
    const Cell src[3] = {CLASSES[0][2], CLASSES[1][1], CLASSES[2][3]};
    for (size_t k = 0; k < 3; k++)
      for (const Cell &c : CLASSES[k])
        if (at(c) != at(src[k])) m[at(c)] = rnd();
    CHECK(settle({{src[2].row, src[2].col}, {src[0].row, src[0].col}, {src[1].row, src[1].col}}, 1, m, &r));
    CHECK(r.wires == witness && r.flag == NONE);
    CHECK(r.report == (std::vector<u64>{3, 3, 10 - 3, 0, ~0ull, ~0ull}));
    // ---- a partial list: classes 0 and 2 keep their scrambled words
    CHECK(settle({{src[1].row, src[1].col}}, 0, m, &r));
    std::vector<u64> want = m;
    want[at(CLASSES[1][0])] = m[at(src[1])];
    CHECK(r.wires == want && r.report == (std::vector<u64>{3, 1, 1, 0, ~0ull, ~0ull}));
  }
  // ---- a conflict, both list orders: the owner is the smaller index, the class holds its word, the other classes are untouched
  for (int order = 0; order < 2; order++) {
    std::vector<u64> m = witness;
    const Cell a = CLASSES[2][1], b = CLASSES[2][4];
    m[at(a)] = 77; m[at(b)] = 78;
    const Cell first = order ? b : a, second = order ? a : b;
    CHECK(settle({{0, 4}, {first.row, first.col}, {second.row, second.col}}, 1, m, &r));
    std::vector<u64> want = m;
    for (const Cell &c : CLASSES[2]) want[at(c)] = m[at(first)];
    CHECK(r.wires == want && r.flag == NONE);
    CHECK(r.report == (std::vector<u64>{3, 1, 3, 1, 2, 1}));
  }
  // ---- v against v + p: no conflict, the owner's raw word
  {
    std::vector<u64> m = witness;
    m[at(CLASSES[1][0])] = 5; m[at(CLASSES[1][1])] = 5 + GL_P;
    CHECK(settle({{CLASSES[1][1].row, CLASSES[1][1].col}, {CLASSES[1][0].row, CLASSES[1][0].col}}, 1, m, &r));
    CHECK(r.wires[at(CLASSES[1][0])] == 5 + GL_P && r.wires[at(CLASSES[1][1])] == 5 + GL_P);
    CHECK(r.report == (std::vector<u64>{3, 1, 0, 0, ~0ull, ~0ull}));
  }
  // ---- a non-routed wire, a routed cell in no class, the last cell of the matrix: nothing changes
  CHECK(settle({{3, 4}, {6, 0}, {(u32)N - 1, W - 1}}, 1, witness, &r));
  CHECK(r.wires == witness && r.report == (std::vector<u64>{3, 0, 0, 0, ~0ull, ~0ull}) && r.flag == NONE);
  // ---- one cell listed twice, with another source of its class between
  {
    std::vector<u64> m = witness;
    m[at(CLASSES[0][0])] = 1; m[at(CLASSES[0][1])] = 2; m[at(CLASSES[0][2])] = 3;
    const Cell a = CLASSES[0][1], b = CLASSES[0][0];
    CHECK(settle({{a.row, a.col}, {b.row, b.col}, {a.row, a.col}}, 0, m, &r));
    CHECK(r.wires[at(CLASSES[0][0])] == 2 && r.wires[at(CLASSES[0][1])] == 2 && r.wires[at(CLASSES[0][2])] == 2);
    CHECK(r.report == (std::vector<u64>{3, 1, 1, 1, 1, 0}));
  }
  // ---- refused entries: a host list changes nothing; in a device list the entry does nothing and the rest is done
  {
    std::vector<u64> m = witness;
    m[at(CLASSES[1][0])] = 9;
    const std::vector<CellRefDev> refs = {{CLASSES[1][0].row, CLASSES[1][0].col}, {(u32)N, 0}, {0, W}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
    CHECK(settle(refs, 1, m, &r));
    CHECK(r.wires == m && r.flag == row_refusal(1, FILL_CELL_ROW) && r.report == (std::vector<u64>{3, 0, 0, 0, ~0ull, ~0ull}));
    CHECK(settle(refs, 0, m, &r));
    std::vector<u64> want = m;
    want[at(CLASSES[1][1])] = 9;
    CHECK(r.wires == want && r.flag == row_refusal(1, FILL_CELL_ROW) && r.report == (std::vector<u64>{3, 1, 1, 0, ~0ull, ~0ull}));
    CHECK(settle({{0, W}}, 0, m, &r));
    CHECK(r.wires == m && r.flag == row_refusal(0, FILL_CELL_COLUMN));
  }
  // ---- an empty list (a null pointer)
  {
    Result e{witness, std::vector<u64>(6), 0};
    std::vector<uint32_t> t = table();
    emu_settle_copies(t.data(), CLASSES.size(), N, W, NR, nullptr, 0, 1, e.wires.data(), e.report.data(), &e.flag, 4, 0);
    CHECK(e.wires == witness && t == table() && e.flag == NONE && e.report == (std::vector<u64>{3, 0, 0, 0, ~0ull, ~0ull}));
  }
  printf("sanitize_settle: 3 hand-made classes, 4 tilings each: round trip, partial list, conflicts, v + p, no-class sources, a double, refusals, empty: ok\n");
  return 0;
}
