// TEST HARNESS (not product code): emu_pos.cpp, emu_u32.cpp and emu_gates.cpp under ASan + UBSan as a stand-alone program
// (tests/checks/emu_sanitize.sh): the Poseidon edge rows one by one and as a grid on a tagged matrix, a u32 job list with two
// refused jobs, and the walk of the light native gates (csrc/light_gates.hpp) on wire matrices of exactly num_wires columns.
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
void emu_light_walk(unsigned num_ops, unsigned num_limbs, const unsigned long long *wires, unsigned num_wires, const unsigned long long *consts,
                    unsigned num_selectors, unsigned long long count, const unsigned long long *alphas, unsigned long long *a_alone,
                    unsigned long long *b_alone, unsigned long long *a_pair, unsigned long long *b_pair);
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

  // the light-gate walk: the wire matrix ends with wire num_wires - 1 (heap: a read past it is ASan's), num_wires = the top wire the
  // shape reads and one above it, the shapes on both sides of a batch of 16; the pair must give what each gate gives alone
  const unsigned shapes[][2] = {{20, 63}, {1, 127}, {33, 1}, {4, 15}, {4, 16}, {5, 14}, {3, 0}, {0, 17}};
  for (const auto &sh : shapes) {
    const unsigned ops = sh[0], limbs = sh[1], top = 4 * ops > (limbs ? limbs + 1 : 0) ? 4 * ops : limbs + 1;
    for (unsigned nw = top; nw <= top + 1; nw++) {
      const u64 cnt = 3;
      std::vector<unsigned long long> lw((size_t)nw * cnt), lc(3 * cnt), out[4];
      u64 seed = 1 + nw;
      for (auto &v : lw) v = gl_canon(seed = seed * 6364136223846793005ull + 1442695040888963407ull);
      for (auto &v : lc) v = gl_canon(seed = seed * 6364136223846793005ull + 1442695040888963407ull);
      for (auto &o : out) o.assign(2 * cnt, TAG);
      const unsigned long long alphas[2] = {lw[0] | 1, 0};
      emu_light_walk(ops, limbs, lw.data(), nw, lc.data(), 1, cnt, alphas, out[0].data(), out[1].data(), out[2].data(), out[3].data());
      for (u64 k = 0; k < 2 * cnt; k++) {
        CHECK(ops && limbs ? out[0][k] == out[2][k] && out[1][k] == out[3][k] : out[2][k] == TAG && out[3][k] == TAG);
        CHECK((out[0][k] == TAG) == !ops && (out[1][k] == TAG) == !limbs);
      }
    }
  }
  printf("emu_pos, emu_u32 and the light-gate walk under the sanitizers: ok\n");
  return 0;
}
