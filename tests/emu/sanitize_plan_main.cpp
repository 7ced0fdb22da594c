// TEST HARNESS (not product code): emu_plan.cpp under ASan + UBSan as a stand-alone program, linked against nothing else
// (tests/checks/emu_sanitize.sh).
// Random PoseidonGate chains with operands of all three sources against pos_row_cells row by row, and the refusals: every
// structural reason (the lists sized exactly, so a read past a refused index is a heap overflow), a CELL swap of 2 in the middle of
// a chain, and both families in one level.
#include <vector>
#include "emu_plan.cpp"
#include "sanitize_common.hpp"

struct Plan {
  std::vector<RecJobDev> rec;
  std::vector<PosJobDev> pos;
  std::vector<unsigned> chain_ends;
  std::vector<RecOperandDev> ops;
  void job(u32 row, const RecOperandDev (&o)[13]) {
    pos.push_back({row, (u32)ops.size()});
    ops.insert(ops.end(), o, o + 13);
  }
  void end_chain() { chain_ends.push_back((unsigned)pos.size()); }
};

static void level(const Plan &p, u64 rb, u64 re, u64 cb, u64 ce, std::vector<u64> &w, u64 n, u64 *flags, u64 lv) {
  emu_plan_level(p.rec.data(), rb, re, p.pos.data(), p.pos.size(), p.chain_ends.data(), cb, ce, p.ops.data(), p.ops.size(),
                 (unsigned long long *)w.data(), POS_GATE_WIRES, n, (unsigned long long *)flags, lv, 64);
}

int main() {
  const u64 n = 64, NONE = ROW_NO_PROBLEM, edge[5] = {0, GL_P - 1, ~0ull, GL_P, 1};
  const u64 *rc = emu_round_constants();
  // ---- random chains on rows 8.., CELL sources in rows 0..7
  std::vector<u64> w(POS_GATE_WIRES * n);
  for (u64 c = 0; c < POS_GATE_WIRES; c++)
    for (u64 r = 0; r < 8; r++) w[c * n + r] = rnd();
  w[0 * n + 0] = 0;
  w[0 * n + 1] = GL_P + 1;
  Plan p;
  u32 row = 8, seen_src[3] = {0, 0, 0};
  const u32 lengths[6] = {1, 2, 17, 0, 5, 3};
  for (u32 len : lengths) {
    for (u32 k = 0; k < len; k++) {
      RecOperandDev o[13];
      const u64 pick = rnd() % 4;
      o[0] = pick == 0 ? RecOperandDev{0, 0, PLAN_CELL} : pick == 1 ? RecOperandDev{1, 0, PLAN_CELL} : RecOperandDev{pick == 2 ? GL_P + 1 : GL_P, 0, PLAN_IMM};
      for (u32 i = 1; i < 13; i++) {
        const u64 s = rnd() % 4;
        o[i] = s == 0 && k ? RecOperandDev{0, (u32)(rnd() % 12), PLAN_PREV}
             : s == 1     ? RecOperandDev{rnd() % 8, (u32)(rnd() % POS_GATE_WIRES), PLAN_CELL}
                          : RecOperandDev{s == 2 ? edge[rnd() % 5] : rnd(), 0, PLAN_IMM};
        seen_src[o[i].src]++;
      }
      p.job(row++, o);
    }
    p.end_chain();
  }
  CHECK(seen_src[0] && seen_src[1] && seen_src[2] && row <= n);
  const std::vector<u64> start = w;
  u64 flags[2] = {NONE, NONE};
  level(p, 0, 0, 0, p.chain_ends.size(), w, n, flags, 0);
  CHECK(flags[0] == NONE && flags[1] == NONE);
  for (size_t g = 0; g < p.chain_ends.size(); g++) {
    u64 prev[12] = {};
    for (u64 i = g ? p.chain_ends[g - 1] : 0; i < p.chain_ends[g]; i++) {
      const RecOperandDev *o = &p.ops[p.pos[i].first_operand];
      u64 v[13], cells[POS_GATE_WIRES];
      for (u32 k = 0; k < 13; k++) v[k] = o[k].src == PLAN_CELL ? start[o[k].col * n + o[k].v] : o[k].src == PLAN_PREV ? prev[o[k].col] : o[k].v;
      pos_row_cells(v + 1, gl_canon(v[0]) != 0, rc, [](u64 *s) { pos_mds(s); }, [&](u32 col, u64 x) { cells[col] = x; });
      for (u32 c = 0; c < POS_GATE_WIRES; c++) CHECK(w[c * n + p.pos[i].row] == cells[c] && cells[c] < GL_P);
      for (u32 k = 0; k < 12; k++) prev[k] = cells[POS_WIRE_OUTPUT + k];
    }
  }
  for (u64 c = 0; c < POS_GATE_WIRES; c++)
    for (u64 r = row; r < n; r++) CHECK(w[c * n + r] == start[c * n + r]);
  // ---- every structural reason in the second job of a chain (the first for 1, 2, 4), lists sized exactly
  const RecOperandDev Z = {0, 0, PLAN_IMM};
  for (u32 code = 1; code <= 9; code++) {
    Plan q;
    RecOperandDev ok[13], bad[13];
    for (u32 i = 0; i < 13; i++) ok[i] = bad[i] = Z;
    const bool single = code == 1 || code == 2 || code == 4;
    if (!single) q.job(3, ok);
    if (code == 3) bad[6] = {1, 0, 3};
    if (code == 4) bad[1] = {0, 0, PLAN_PREV};
    if (code == 5) bad[0] = {0, 0, PLAN_PREV};
    if (code == 6) bad[12] = {0, 12, PLAN_PREV};
    if (code == 7) bad[1] = {0, POS_GATE_WIRES, PLAN_CELL};
    if (code == 8) bad[0] = {n, 0, PLAN_CELL};
    if (code == 9) bad[0] = {2, 0, PLAN_IMM};
    q.job(code == 1 ? (u32)n : 4, bad);
    if (code == 2) q.ops.pop_back();
    q.end_chain();
    const u32 at = single ? 0 : 1;
    unsigned family = 0;
    unsigned long long job = 0;
    CHECK(emu_plan_lists_problem(nullptr, 0, q.pos.data(), q.chain_ends.data(), 1, q.ops.data(), q.ops.size(), POS_GATE_WIRES, n, &family, &job) == code);
    CHECK(family == 1 && job == at);
    std::vector<u64> m(POS_GATE_WIRES * n, 0);
    u64 f[2] = {NONE, NONE};
    level(q, 0, 0, 0, 1, m, n, f, 0);
    CHECK(f[1] == row_refusal(at, code) && f[0] == row_refusal(plan_shift(0), ROW_OTHER_FAMILY));
    for (u64 c = 0; c < POS_GATE_WIRES; c++) CHECK(m[c * n + 4] == 0 && m[c * n + n - 1] == 0);
    CHECK(single || m[POS_WIRE_OUTPUT * n + 3] != 0);  // the row before the refused one is written
    level(q, 0, 0, 0, 1, m, n, f, 1);                  // a later level writes nothing
    CHECK(m[POS_WIRE_OUTPUT * n + 4] == 0);
  }
  // ---- a CELL swap of 2 in row 2 of a three-row chain, next to a RANDOM_ACCESS job whose CELL index is 16: the rec job is named
  {
    Plan q;
    std::vector<u64> m(POS_GATE_WIRES * n, 0);
    m[3 * n + 0] = 2;
    m[7 * n + 0] = 16;
    RecOperandDev o[13];
    for (u32 i = 0; i < 13; i++) o[i] = Z;
    q.job(10, o);
    q.job(11, o);
    o[0] = {0, 3, PLAN_CELL};
    q.job(12, o);
    q.end_chain();
    o[0] = Z;
    q.job(13, o);
    q.end_chain();
    q.rec.push_back({30, (uint16_t)REC_RANDOM_ACCESS, 0, (u32)q.ops.size(), 0});
    q.ops.push_back({0, 7, REC_CELL});
    for (u32 i = 0; i < 16; i++) q.ops.push_back({i, 0, REC_IMM});
    u64 f[2] = {NONE, NONE};
    level(q, 0, 0, 0, 2, m, n, f, 0);  // the chains alone
    CHECK(f[1] == row_refusal(2, 9) && f[0] == row_refusal(plan_shift(0), ROW_OTHER_FAMILY));
    CHECK(m[POS_WIRE_OUTPUT * n + 10] && m[POS_WIRE_OUTPUT * n + 11] && !m[POS_WIRE_OUTPUT * n + 12] && m[POS_WIRE_OUTPUT * n + 13]);
    std::vector<u64> m2(POS_GATE_WIRES * n, 0);
    m2[3 * n + 0] = 2;
    m2[7 * n + 0] = 16;
    u64 f2[2] = {NONE, NONE};
    level(q, 0, 1, 0, 2, m2, n, f2, 0);  // both families
    CHECK(f2[0] == row_refusal(0 + plan_shift(0), 9) && f2[1] == row_refusal(2, 9) && m2[POS_WIRE_OUTPUT * n + 13] && !m2[0 * n + 30]);
  }
  printf("sanitize_plan: %zu random jobs in %zu chains, 9 refusal reasons, CELL swap and two-family refusals: ok\n", p.pos.size(), p.chain_ends.size());
  return 0;
}
