// TEST HARNESS (not product code): emu_pos.cpp and emu_u32.cpp under ASan + UBSan as a stand-alone program
// (tests/checks/emu_sanitize.sh): the Poseidon edge rows one by one and as a grid on a tagged matrix, and a u32 job list with two
// refused jobs.
#include <vector>
#include "sanitize_common.hpp"
#include "emu_rc.hpp"
#include "../../eth-lc-plonky2_amd/csrc/pos_rows.hpp"
#include "../../eth-lc-plonky2_amd/csrc/u32_rows.hpp"

using namespace lcp2;

extern "C" {
unsigned emu_pos_row_cells(const PoseidonRowDev *job, unsigned *cols, unsigned long long *vals, unsigned cap);
void emu_pos_gate_rows(const PoseidonRowDev *rows, unsigned long long nrows, unsigned long long *wires, unsigned long long n, unsigned blocks,
                       unsigned threads);
void emu_u32_gate_rows(const U32JobDev *jobs, unsigned long long njobs, unsigned long long *wires, unsigned long long n, unsigned long long *flag,
                       unsigned blocks, unsigned threads);
}

int main() {
  const u64 *rc = emu_round_constants();
  const u64 TAG = ~0ull - 1, edge[4] = {0, GL_P - 1, GL_P, ~0ull};
  std::vector<PoseidonRowDev> rows;
  for (u32 swap = 0; swap < 2; swap++)
    for (u64 v : edge) {
      PoseidonRowDev j{(u32)rows.size(), swap, {}};
      for (auto &x : j.in) x = v;
      rows.push_back(j);
    }
  PoseidonRowDev same{(u32)rows.size(), 1, {5, GL_P, ~0ull, 7, 5, 0, GL_EPS - 1, 7, 1, 2, 3, 4}};  // first four = next four mod p: deltas 0
  rows.push_back(same);
  for (const PoseidonRowDev &j : rows) {
    unsigned cols[POS_GATE_WIRES];
    unsigned long long vals[POS_GATE_WIRES];
    u64 got[POS_GATE_WIRES], seen[POS_GATE_WIRES] = {}, s[12];
    CHECK(emu_pos_row_cells(&j, cols, vals, POS_GATE_WIRES) == POS_GATE_WIRES);
    for (u32 k = 0; k < POS_GATE_WIRES; k++) { CHECK(cols[k] < POS_GATE_WIRES && !seen[cols[k]]++ && vals[k] < GL_P); got[cols[k]] = vals[k]; }
    for (int i = 0; i < 12; i++) s[i] = gl_canon(j.in[j.swap && i < 8 ? (i + 4) % 8 : i]);
    pos_permute_portable(s, rc);
    for (int i = 0; i < 12; i++) CHECK(got[POS_WIRE_OUTPUT + i] == s[i]);
    if (&j == &rows.back()) for (int i = 0; i < 4; i++) CHECK(got[POS_WIRE_DELTA + i] == 0);
  }
  const u64 n = 16;
  std::vector<unsigned long long> wires(POS_GATE_WIRES * n, TAG);
  emu_pos_gate_rows(rows.data(), rows.size(), wires.data(), n, 2, 64);
  for (u32 c = 0; c < POS_GATE_WIRES; c++)
    for (u64 r = 0; r < n; r++) CHECK((wires[c * n + r] == TAG) == (r >= rows.size()));

  // 100 range-check jobs, jobs 7 (row out of range) and 70 (unknown kind) refused: the flag names job 7, neither writes
  std::vector<U32JobDev> jobs;
  for (u32 i = 0; i < 100; i++) jobs.push_back(U32JobDev{i % 16, U32_KIND_RANGE_CHECK, (uint16_t)(i / 16), {0xFFFFFFFFu - i, 0, 0, 0}});
  jobs[7].row = (u32)n;
  jobs[70].kind = 9;
  std::vector<unsigned long long> w32(U32_ROW_COLUMNS * n, TAG);
  unsigned long long flag = ROW_NO_PROBLEM;
  emu_u32_gate_rows(jobs.data(), jobs.size(), w32.data(), n, &flag, 2, 64);
  CHECK(flag == row_refusal(7, 1));
  CHECK(w32[0 * n + 7] == TAG && w32[(70 / 16) * n + 70 % 16] == TAG && w32[0 * n + 8] == 0xFFFFFFFFu - 8);
  printf("emu_pos and emu_u32 under the sanitizers: ok\n");
  return 0;
}
