// TEST HARNESS (not product code): emu_plan_u32.cpp under ASan + UBSan as a stand-alone program, linked against nothing else:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -o /tmp/emu_sanitize_plan_u32 tests/emu/sanitize_plan_u32_main.cpp && /tmp/emu_sanitize_plan_u32
// Two levels of random u32 plan jobs of every kind and operation slot - the second level's operands CELLs of the first level's
// outputs - against u32_job_cells on the resolved inputs, and the refusals: every reason with the lists sized exactly (a read past a
// refused index is a heap overflow), the two value reasons through CELLs, later levels, and three families refusing in one level.
#include <vector>
#include "emu_plan_u32.cpp"
#include "sanitize_common.hpp"

struct Plan {
  std::vector<RecJobDev> rec;
  std::vector<U32PlanJobDev> u32_jobs;
  std::vector<PosJobDev> pos;
  std::vector<unsigned> chain_ends;
  std::vector<RecOperandDev> ops;
  void job(u32 row, u32 kind, u32 op, std::initializer_list<RecOperandDev> o) {
    u32_jobs.push_back({row, (uint16_t)kind, (uint16_t)op, (u32)ops.size(), 0});
    ops.insert(ops.end(), o.begin(), o.end());
  }
};

static void level(const Plan &p, u64 rb, u64 re, u64 ub, u64 ue, u64 cb, u64 ce, std::vector<u64> &w, u64 n, u64 *flags, u64 lv, unsigned threads = 256) {
  emu_plan_u32_level(p.rec.data(), rb, re, p.u32_jobs.data(), ub, ue, p.pos.data(), p.pos.size(), p.chain_ends.data(), cb, ce, p.ops.data(),
                     p.ops.size(), (unsigned long long *)w.data(), POS_GATE_WIRES, n, (unsigned long long *)flags, lv, threads);
}

int main() {
  const u64 n = 70, NONE = ROW_NO_PROBLEM;
  const u32 NC = POS_GATE_WIRES;
  // ---- level 0: every (kind, op) on its own row from IMMs (some spelled v + p); level 1: the same slots on other rows from CELLs
  Plan p;
  std::vector<u64> w(NC * n);
  for (auto &x : w) x = rnd();
  const std::vector<u64> start = w;
  auto imm = [&](u64 hi) -> RecOperandDev {
    const u64 v = rnd() % hi;
    return {rnd() % 4 == 0 && v < U32_MAX ? v + GL_P : v, 0, PLAN_IMM};
  };
  u32 row = 0;
  struct Out { u32 row, col; };
  std::vector<Out> words, bits;
  for (u32 kind = 0; kind < U32_KINDS; kind++)
    for (u32 op = 0; op < u32_kind_ops(kind); op++, row++) {
      const u64 full = 1ull << 32;
      if (kind == U32_KIND_ARITHMETIC) { p.job(row, kind, op, {imm(full), imm(full), imm(full)}); words.push_back({row, 6 * op + 3}); words.push_back({row, 6 * op + 4}); }
      if (kind == U32_KIND_ADD_MANY) { p.job(row, kind, op, {imm(full), imm(full), imm(full), imm(4)}); words.push_back({row, 6 * op + 4}); }
      if (kind == U32_KIND_SUBTRACTION) { p.job(row, kind, op, {imm(full), imm(full), imm(2)}); words.push_back({row, 5 * op + 3}); bits.push_back({row, 5 * op + 4}); }
      if (kind == U32_KIND_RANGE_CHECK) p.job(row, kind, op, {imm(full)});
      if (kind == U32_KIND_COMPARISON) { p.job(row, kind, op, {imm(full), imm(full)}); bits.push_back({row, 2}); }
    }
  const u64 level0 = p.u32_jobs.size();
  CHECK(level0 == 22);
  auto word = [&]() -> RecOperandDev { const Out o = words[rnd() % words.size()]; return {o.row, o.col, PLAN_CELL}; };
  auto bit = [&]() -> RecOperandDev { const Out o = bits[rnd() % bits.size()]; return {o.row, o.col, PLAN_CELL}; };  // a borrow or result_bool
  for (u32 kind = 0; kind < U32_KINDS; kind++)
    for (u32 op = 0; op < u32_kind_ops(kind); op++, row++) {
      if (kind == U32_KIND_ARITHMETIC) p.job(row, kind, op, {word(), word(), word()});
      if (kind == U32_KIND_ADD_MANY) p.job(row, kind, op, {word(), word(), word(), bit()});
      if (kind == U32_KIND_SUBTRACTION) p.job(row, kind, op, {word(), word(), bit()});
      if (kind == U32_KIND_RANGE_CHECK) p.job(row, kind, op, {word()});
      if (kind == U32_KIND_COMPARISON) p.job(row, kind, op, {word(), bit()});
    }
  CHECK(row == 44 && row <= n);
  u64 flags[3] = {NONE, NONE, NONE};
  level(p, 0, 0, 0, level0, 0, 0, w, n, flags, 0, 16);
  const std::vector<u64> middle = w;
  level(p, 0, 0, level0, p.u32_jobs.size(), 0, 0, w, n, flags, 1, 16);
  CHECK(flags[0] == NONE && flags[1] == NONE && flags[2] == NONE);
  std::vector<u64> want = start;
  for (size_t i = 0; i < p.u32_jobs.size(); i++) {
    const U32PlanJobDev j = p.u32_jobs[i];
    const std::vector<u64> &from = i < level0 ? start : middle;
    U32JobDev r = {j.row, j.kind, j.op, {0, 0, 0, 0}};
    for (u32 k = 0; k < u32_plan_operands(j.kind); k++) {
      const RecOperandDev o = p.ops[j.first_operand + k];
      const u64 v = gl_canon(o.src == PLAN_CELL ? from[o.col * n + o.v] : o.v);
      CHECK(v <= U32_MAX);
      r.in[k] = (u32)v;
    }
    CHECK(u32_job_problem(r, n) == 0);
    u32_job_cells(r, [&](u32 col, u64 x) { want[col * n + j.row] = x; });
  }
  CHECK(w == want);
  // ---- every reason in the LAST job of a list sized exactly; level 1 then writes nothing
  u32 reasons = 0;
  for (u32 code = 1; code <= 9; code++)
    for (int by_cell = 0; by_cell < (code == 4 || code == 9 ? 2 : 1); by_cell++) {
      Plan q;
      std::vector<u64> m(NC * n, 0);
      m[0 * n + 60] = 1ull << 32;
      m[1 * n + 60] = 2;
      m[2 * n + 60] = 41 + GL_P;
      const RecOperandDev one = {1, 0, PLAN_IMM}, big = by_cell ? RecOperandDev{60, 0, PLAN_CELL} : RecOperandDev{1ull << 32, 0, PLAN_IMM},
                          two = by_cell ? RecOperandDev{60, 1, PLAN_CELL} : RecOperandDev{2, 0, PLAN_IMM};
      q.ops.push_back(one);  // the operand of level 1's job, so that the refused job's operands end the list
      q.job(3, U32_KIND_ADD_MANY, 1, {one, {60, 2, PLAN_CELL}, {41 + GL_P, 0, PLAN_IMM}, one});  // accepted: 1 + 41 + 41 + 1
      if (code == 1) q.job((u32)n, U32_KIND_ARITHMETIC, 0, {one, one, one});
      if (code == 2) q.job(4, U32_KINDS, 0, {one, one, one, one});
      if (code == 3) q.job(4, U32_KIND_RANGE_CHECK, U32_RANGE_OPS, {one});
      if (code == 4) q.job(4, U32_KIND_SUBTRACTION, 5, {one, one, two});
      if (code == 5) { q.job(4, U32_KIND_ADD_MANY, 0, {one, one, one, one}); q.ops.pop_back(); }
      if (code == 6) q.job(4, U32_KIND_COMPARISON, 0, {one, {0, 0, PLAN_PREV}});
      if (code == 7) q.job(4, U32_KIND_RANGE_CHECK, 0, {{0, NC, PLAN_CELL}});
      if (code == 8) q.job(4, U32_KIND_ARITHMETIC, 2, {one, one, {n, 0, PLAN_CELL}});
      if (code == 9) q.job(4, U32_KIND_ARITHMETIC, 2, {one, big, one});
      q.u32_jobs.push_back({5, (uint16_t)U32_KIND_RANGE_CHECK, 0, 0, 0});  // level 1
      q.ops.shrink_to_fit();
      unsigned family = 0;
      unsigned long long job = 0;
      const unsigned host = emu_plan_u32_lists_problem(nullptr, 0, q.u32_jobs.data(), 2, nullptr, nullptr, 0, q.ops.data(), q.ops.size(), NC, n, &family, &job);
      CHECK(by_cell ? host == 0 : host == code && family == 2 && job == 1);
      u64 f[3] = {NONE, NONE, NONE};
      level(q, 0, 0, 0, 2, 0, 0, m, n, f, 0);
      CHECK(f[2] == row_refusal(1 + plan_shift(0), code) && f[0] == row_refusal(plan_shift(0), ROW_U32_FAMILY) && f[1] == NONE);
      CHECK(m[(6 + 4) * n + 3] == 84 && m[(6 + 5) * n + 3] == 0);  // the valid job of the level is written
      for (u32 c = 0; c < NC; c++) CHECK(m[c * n + 4] == 0 && m[c * n + n - 1] == 0);
      level(q, 0, 0, 2, 3, 0, 0, m, n, f, 1);  // a later level writes nothing
      for (u32 c = 0; c < NC; c++) CHECK(m[c * n + 5] == 0);
      const unsigned ends[2] = {2, 3};
      CHECK(emu_plan_u32_refusal((unsigned long long *)f, nullptr, ends, 2, &family, &job) == code && family == 2 && job == 1);
      reasons++;
    }
  // ---- three families refuse in level 1 of two: RANDOM_ACCESS index 16, a borrow of 2, a swap of 2 (all CELLs): the rec job is named
  {
    Plan q;
    std::vector<u64> m(NC * n, 0);
    m[1 * n + 60] = 2;
    m[4 * n + 60] = 16;
    const RecOperandDev Z = {0, 0, PLAN_IMM};
    q.job(3, U32_KIND_RANGE_CHECK, 0, {{7, 0, PLAN_IMM}});                                  // level 0
    q.job(4, U32_KIND_SUBTRACTION, 0, {Z, Z, {60, 1, PLAN_CELL}});                          // level 1: refused
    q.job(5, U32_KIND_COMPARISON, 0, {{3, 0, PLAN_CELL}, {9, 0, PLAN_IMM}});                             // level 1: valid
    q.rec.push_back({30, (uint16_t)REC_RANDOM_ACCESS, 0, (u32)q.ops.size(), 0});
    q.ops.push_back({60, 4, REC_CELL});
    for (u32 i = 0; i < 16; i++) q.ops.push_back({i, 0, REC_IMM});
    q.pos.push_back({40, (u32)q.ops.size()});
    q.ops.push_back({60, 1, PLAN_CELL});
    for (u32 i = 0; i < 12; i++) q.ops.push_back(Z);
    q.chain_ends.push_back(1);
    u64 f[3] = {NONE, NONE, NONE};
    level(q, 0, 0, 0, 1, 0, 0, m, n, f, 0);
    level(q, 0, 1, 1, 3, 0, 1, m, n, f, 1);
    CHECK(f[0] == row_refusal(0 + plan_shift(1), 9) && f[1] == row_refusal(0, 9) && f[2] == row_refusal(1 + plan_shift(1), 4));
    CHECK(m[0 * n + 3] == 7 && m[0 * n + 5] == 7 && m[2 * n + 5] == 1 && m[0 * n + 30] == 0 && m[12 * n + 40] == 0);
    for (u32 c = 0; c < NC; c++) CHECK(m[c * n + 4] == 0);
    unsigned family = 9;
    unsigned long long job = 9;
    const unsigned rec_ends[2] = {0, 1}, u32_ends[2] = {1, 3};
    CHECK(emu_plan_u32_refusal((unsigned long long *)f, rec_ends, u32_ends, 2, &family, &job) == 9 && family == 0 && job == 0);
    const unsigned no_rec[2] = {0, 0};
    f[0] = row_refusal(plan_shift(1), ROW_U32_FAMILY);  // as the words stand without the rec job: the u32 job before the chain
    CHECK(emu_plan_u32_refusal((unsigned long long *)f, no_rec, u32_ends, 2, &family, &job) == 4 && family == 2 && job == 1);
  }
  printf("sanitize_plan_u32: %zu jobs in two levels, %u refusals, three families in one level: ok\n", p.u32_jobs.size(), reasons);
  return 0;
}
