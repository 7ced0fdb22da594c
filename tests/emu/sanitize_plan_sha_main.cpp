// TEST HARNESS (not product code): emu_plan_sha.cpp under ASan + UBSan as a stand-alone program, linked against nothing else:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_plan_sha tests/emu/sanitize_plan_sha_main.cpp && /tmp/emu_sanitize_plan_sha
// The plan of all four families (two SHA jobs; a u32 job and a rec job that read digest cells; a SHA job that reads their outputs
// beside a PoseidonGate chain that reads digest cells) against sha_words_record / sha_row_cells on the resolved words, with the
// matrix and the lists sized exactly (a read or a store past them is a heap overflow), and the refusals: every reason with the
// operand list ending at the refused job, the value reason through a CELL, a later level, and four families refusing in one level.
#include <vector>
#include "emu_plan_sha.cpp"
#include "sanitize_common.hpp"

struct Plan {
  std::vector<RecJobDev> rec;
  std::vector<ShaPlanJobDev> sha;
  std::vector<U32PlanJobDev> u32_jobs;
  std::vector<PosJobDev> pos;
  std::vector<unsigned> chain_ends;
  std::vector<RecOperandDev> ops;
  void hash(u32 first_row, const std::vector<RecOperandDev> &o) {
    sha.push_back({first_row, (u32)ops.size()});
    ops.insert(ops.end(), o.begin(), o.end());
  }
};

static void level(const Plan &p, u64 rb, u64 re, u64 sb, u64 se, u64 ub, u64 ue, u64 cb, u64 ce, std::vector<u64> &w, u64 n, u64 *flags, u64 lv) {
  emu_plan_sha_level(p.rec.data(), rb, re, p.sha.data(), sb, se, p.u32_jobs.data(), ub, ue, p.pos.data(), p.pos.size(), p.chain_ends.data(), cb, ce,
                     p.ops.data(), p.ops.size(), (unsigned long long *)w.data(), POS_GATE_WIRES, n, (unsigned long long *)flags, lv, 64);
}
static RecOperandDev digest(u32 first_row, u32 i) { return {first_row + 307 + i / 3, 3 * (i % 3) + 2, PLAN_CELL}; }
static std::vector<RecOperandDev> random_words() {
  std::vector<RecOperandDev> o;
  for (u32 k = 0; k < 16; k++) {
    const u64 v = rnd() >> 32;
    o.push_back({k % 5 == 0 && v < 0xFFFFFFFFull ? v + GL_P : v, 0, PLAN_IMM});  // some spelled v + p
  }
  return o;
}
// the rows of one hash from its 16 words, into `want`
static void expect(std::vector<u64> &want, u64 n, u32 first_row, const uint32_t *msg) {
  uint32_t R[SHA_REC_WORDS];
  sha_words_record(msg, R);
  for (u32 lr = 0; lr < SHA_ROWS; lr++) sha_row_cells(R, lr, [&](u32 col, u64 x) { want[col * n + first_row + lr] = x; });
}

int main() {
  const u64 NONE = ROW_NO_PROBLEM;
  const u32 NC = POS_GATE_WIRES;
  // ---- case (c): four families in three levels, the last hash flush against the end of the matrix
  {
    const u64 n = 3 * SHA_ROWS + 3;
    const u32 h0 = 3, h1 = 3 + SHA_ROWS, h2 = 3 + 2 * SHA_ROWS, urow = 0, rrow = 1, crow = 2;
    Plan p;
    std::vector<u64> w(NC * n);
    for (auto &x : w) x = rnd();
    std::vector<u64> want = w;
    p.hash(h1, random_words());
    p.hash(h0, random_words());
    p.u32_jobs.push_back({urow, (uint16_t)U32_KIND_ADD_MANY, 2, (u32)p.ops.size(), 0});
    for (const RecOperandDev &o : {digest(h1, 0), digest(h0, 7), RecOperandDev{4000000000ull, 0, PLAN_IMM}, RecOperandDev{3, 0, PLAN_IMM}}) p.ops.push_back(o);
    p.rec.push_back({rrow, (uint16_t)REC_ARITHMETIC, 5, (u32)p.ops.size(), 0});
    for (const RecOperandDev &o : {RecOperandDev{0, 0, REC_IMM}, RecOperandDev{1, 0, REC_IMM}, RecOperandDev{9, 0, REC_IMM}, RecOperandDev{9, 0, REC_IMM}, digest(h0, 4)})
      p.ops.push_back(o);
    std::vector<RecOperandDev> msg = {{urow, 6 * 2 + 4, PLAN_CELL}, {rrow, 4 * 5 + 3, PLAN_CELL}};
    for (u32 k = 0; k < 6; k++) msg.push_back({rnd() >> 32, 0, PLAN_IMM});
    for (u32 i = 0; i < 8; i++) msg.push_back(digest(i < 4 ? h0 : h1, i));
    p.hash(h2, msg);
    p.pos.push_back({crow, (u32)p.ops.size()});
    p.ops.push_back({1, 0, PLAN_IMM});
    for (u32 i = 0; i < 12; i++) p.ops.push_back(digest(i < 8 ? h0 : h1, i % 8));
    p.chain_ends.push_back(1);
    p.ops.shrink_to_fit();
    unsigned family = 9;
    unsigned long long job = 9;
    CHECK(emu_plan_sha_lists_problem(p.rec.data(), 1, p.sha.data(), 3, p.u32_jobs.data(), 1, p.pos.data(), p.chain_ends.data(), 1, p.ops.data(),
                                     p.ops.size(), NC, n, &family, &job) == 0);
    u64 flags[4] = {NONE, NONE, NONE, NONE};
    level(p, 0, 0, 0, 2, 0, 0, 0, 0, w, n, flags, 0);
    level(p, 0, 1, 2, 2, 0, 1, 0, 0, w, n, flags, 1);
    level(p, 1, 1, 2, 3, 1, 1, 0, 1, w, n, flags, 2);
    for (u64 f : flags) CHECK(f == NONE);
    uint32_t m[3][16];
    for (u32 j = 0; j < 2; j++) {
      for (u32 k = 0; k < 16; k++) m[j][k] = (uint32_t)gl_canon(p.ops[p.sha[j].first_operand + k].v);
      expect(want, n, p.sha[j].first_row, m[j]);
    }
    auto cell = [&](const RecOperandDev &o) { return want[o.col * n + o.v]; };
    const u64 total = cell(digest(h1, 0)) + cell(digest(h0, 7)) + 4000000000ull + 3;
    CHECK(w[(6 * 2 + 4) * n + urow] == (total & 0xFFFFFFFFull) && w[(6 * 2 + 5) * n + urow] == total >> 32);
    CHECK(w[(4 * 5 + 3) * n + rrow] == cell(digest(h0, 4)));
    for (u32 k = 0; k < 16; k++) m[2][k] = (uint32_t)(msg[k].src == PLAN_CELL ? w[msg[k].col * n + msg[k].v] : msg[k].v);
    expect(want, n, h2, m[2]);
    for (u32 c = 0; c < SHA_ROW_COLUMNS; c++)
      for (u64 r = 3; r < n; r++) CHECK(w[c * n + r] == want[c * n + r]);
    for (u32 c = SHA_ROW_COLUMNS; c < NC; c++)
      for (u64 r = 3; r < n; r++) CHECK(w[c * n + r] == want[c * n + r]);  // untouched
    for (u32 i = 0; i < 12; i++) CHECK(w[i * n + crow] == cell(digest(i < 8 ? h0 : h1, i % 8)));
    CHECK(w[24 * n + crow] == 1);
  }
  // ---- every reason in the LAST job of level 0, its operands ending a list sized exactly; level 1 then writes nothing
  u32 reasons = 0;
  const u64 n = 3 * SHA_ROWS + 2;
  for (u32 code = 1; code <= 6; code++)
    for (int by_cell = 0; by_cell < (code == SHA_PLAN_NOT_U32 ? 2 : 1); by_cell++) {
      Plan q;
      std::vector<u64> m(NC * n, 0);
      m[0 * n + 1] = 1ull << 32;
      m[2 * n + 1] = 41 + GL_P;
      std::vector<RecOperandDev> ok = random_words(), later = random_words(), bad = random_words();
      ok[3] = {1, 2, PLAN_CELL};  // accepted: a cell holding 41 + p
      q.ops.insert(q.ops.end(), later.begin(), later.end());  // the operands of level 1's job come first, so that the refused job's end the list
      q.hash(2, ok);
      u32 first_row = 2 + SHA_ROWS;
      if (code == SHA_PLAN_ROWS) first_row = (u32)(n - SHA_ROWS + 1);
      if (code == SHA_PLAN_SRC) bad[15] = {0, 0, PLAN_PREV};
      if (code == SHA_PLAN_CELL_COLUMN) bad[0] = {0, NC, PLAN_CELL};
      if (code == SHA_PLAN_CELL_ROW) bad[8] = {n, 0, PLAN_CELL};
      if (code == SHA_PLAN_NOT_U32) bad[15] = by_cell ? RecOperandDev{1, 0, PLAN_CELL} : RecOperandDev{1ull << 32, 0, PLAN_IMM};
      q.hash(first_row, bad);
      if (code == SHA_PLAN_OPERANDS_PAST_END) q.ops.pop_back();
      q.sha.push_back({2 + 2 * SHA_ROWS, 0});  // level 1
      q.ops.shrink_to_fit();
      unsigned family = 0;
      unsigned long long job = 0;
      const unsigned host = emu_plan_sha_lists_problem(nullptr, 0, q.sha.data(), 2, nullptr, 0, nullptr, nullptr, 0, q.ops.data(), q.ops.size(), NC, n, &family, &job);
      CHECK(by_cell ? host == 0 : host == code && family == 3 && job == 1);
      u64 f[4] = {NONE, NONE, NONE, NONE};
      level(q, 0, 0, 0, 2, 0, 0, 0, 0, m, n, f, 0);
      CHECK(f[3] == row_refusal(1 + plan_shift(0), code) && f[0] == row_refusal(plan_shift(0), ROW_SHA_FAMILY) && f[1] == NONE && f[2] == NONE);
      CHECK(m[5 * n + 2 + 48 + 6] == 41);  // the valid job of the level is written: W_3 on its round E row
      for (u32 c = 0; c < NC; c++)
        for (u64 r = 2 + SHA_ROWS; r < n; r++) CHECK(m[c * n + r] == 0);
      level(q, 0, 0, 2, 3, 0, 0, 0, 0, m, n, f, 1);  // a later level writes nothing
      for (u32 c = 0; c < NC; c++)
        for (u64 r = 2 + SHA_ROWS; r < n; r++) CHECK(m[c * n + r] == 0);
      const unsigned ends[2] = {2, 3}, none[2] = {0, 0};
      CHECK(emu_plan_sha_refusal((unsigned long long *)f, none, none, ends, 2, &family, &job) == code && family == 3 && job == 1);
      reasons++;
    }
  // ---- four families refuse in level 1 of two: RANDOM_ACCESS index 16, a word of 2^32, a borrow of 2, a swap of 2 (all CELLs)
  {
    Plan q;
    std::vector<u64> m(NC * n, 0);
    m[0 * n + 1] = 1ull << 32;
    m[1 * n + 1] = 2;
    m[4 * n + 1] = 16;
    const RecOperandDev Z = {0, 0, PLAN_IMM};
    q.hash(2, random_words());  // level 0
    std::vector<RecOperandDev> bad = random_words();
    bad[6] = {1, 0, PLAN_CELL};
    q.hash(2 + SHA_ROWS, bad);                    // level 1: refused
    q.hash(2 + 2 * SHA_ROWS, random_words());     // level 1: valid
    q.u32_jobs.push_back({0, (uint16_t)U32_KIND_SUBTRACTION, 0, (u32)q.ops.size(), 0});
    for (const RecOperandDev &o : {Z, Z, RecOperandDev{1, 1, PLAN_CELL}}) q.ops.push_back(o);
    q.rec.push_back({0, (uint16_t)REC_RANDOM_ACCESS, 0, (u32)q.ops.size(), 0});
    q.ops.push_back({1, 4, REC_CELL});
    for (u32 i = 0; i < 16; i++) q.ops.push_back({i, 0, REC_IMM});
    q.pos.push_back({0, (u32)q.ops.size()});
    q.ops.push_back({1, 1, PLAN_CELL});
    for (u32 i = 0; i < 12; i++) q.ops.push_back(Z);
    q.chain_ends.push_back(1);
    q.ops.shrink_to_fit();
    u64 f[4] = {NONE, NONE, NONE, NONE};
    level(q, 0, 0, 0, 1, 0, 0, 0, 0, m, n, f, 0);
    level(q, 0, 1, 1, 3, 0, 1, 0, 1, m, n, f, 1);
    CHECK(f[0] == row_refusal(0 + plan_shift(1), 9) && f[1] == row_refusal(0, 9) && f[2] == row_refusal(0 + plan_shift(1), 4) &&
          f[3] == row_refusal(1 + plan_shift(1), SHA_PLAN_NOT_U32));
    for (u32 c = 0; c < NC; c++) {
      CHECK(m[c * n + 0] == 0);
      for (u64 r = 2 + SHA_ROWS; r < 2 + 2 * SHA_ROWS; r++) CHECK(m[c * n + r] == 0);
    }
    CHECK(m[0 * n + 2 + 2 * SHA_ROWS + 48] != 0 || m[1 * n + 2 + 2 * SHA_ROWS + 48] != 0);  // the valid hash of the level is written
    unsigned family = 9;
    unsigned long long job = 9;
    const unsigned rec_ends[2] = {0, 1}, u32_ends[2] = {0, 1}, sha_ends[2] = {1, 3}, no_rec[2] = {0, 0};
    CHECK(emu_plan_sha_refusal((unsigned long long *)f, rec_ends, u32_ends, sha_ends, 2, &family, &job) == 9 && family == 0 && job == 0);
    f[0] = row_refusal(plan_shift(1), ROW_SHA_FAMILY);  // as the words stand without the rec job: the SHA job before the u32 job and the chain
    CHECK(emu_plan_sha_refusal((unsigned long long *)f, no_rec, u32_ends, sha_ends, 2, &family, &job) == SHA_PLAN_NOT_U32 && family == 3 && job == 1);
    f[0] = row_refusal(plan_shift(1), ROW_U32_FAMILY);
    CHECK(emu_plan_sha_refusal((unsigned long long *)f, no_rec, u32_ends, sha_ends, 2, &family, &job) == 4 && family == 2 && job == 0);
  }
  printf("sanitize_plan_sha: four families in three levels, %u refusals, four families in one level: ok\n", reasons);
  return 0;
}
