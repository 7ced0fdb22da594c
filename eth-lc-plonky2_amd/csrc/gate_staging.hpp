// The staged (device-side) encoding of the gate programs, and the host pass that makes it.  Plain C++17 without HIP, so that the
// library (kernels_quotient.hip stage_gate_programs), and the CPU harness of the witness check (tests/emu/emu_check.cpp) stage a
// program with the same text.  Readers of the staged form: q_interpret (quotient_common.hpp) and wc_walk (witness_check.hpp).
#pragma once
#include <cstdint>
#include <vector>
#include "gate_program.hpp"

namespace lcp2 {

// Operand staging of the gate-program interpreter (device-side form of the programs, made by stage_gate_programs at build()):
// every WIRE / CONST operand is fetched by an LDG instruction that issues up to QUOTIENT_STAGE column loads back to back and
// parks the values in LDS slots; the instructions after it read kind STAGE.  One exposed HBM round trip per 16 operands
// instead of one per operand (the interpreter executes one instruction at a time, so an operand load cannot overlap anything).
constexpr uint32_t QUOTIENT_STAGE = 12;
constexpr uint32_t QOP_LDG = 10;      // w0 = 10 | count << 8, w1 = offset into stage_list
constexpr uint32_t QKIND_STAGE = 5;   // operand = staging slot idx

// Instructions are scanned in order; when one needs a WIRE / CONST operand that is not in the current window, a new window opens:
// the distinct column operands of the instructions ahead are collected (in order of first use) until QUOTIENT_STAGE of them are
// found, one LDG fetches them, and operands are rewritten to their slots.  Gate: anything with code_offset / code_len (in
// instructions), rewritten to the staged program.  A list entry < num_wires is a wire column, else constants column (entry - num_wires).
template <class Gate>
void stage_programs(const std::vector<uint32_t> &code, std::vector<Gate> &gates, uint32_t num_wires, uint32_t num_selectors,
                    std::vector<uint32_t> &out, std::vector<uint32_t> &lists) {
  typedef uint32_t u32;
  out.clear(); lists.clear();
  using gate_program::Insn;
  auto column_of = [&](const Insn &in, int k) { return in.kind[k] == gate_program::KIND_WIRE ? in.idx[k] : num_wires + num_selectors + in.idx[k]; };
  for (Gate &G : gates) {
    const u32 first = G.code_offset, last = G.code_offset + G.code_len, new_first = (u32)out.size() / 2;
    std::vector<u32> window;  // columns staged by the last LDG
    for (u32 pc = first; pc < last; pc++) {
      Insn in(code[2 * pc], code[2 * pc + 1]);
      auto slot_of = [&](u32 col) { for (u32 s = 0; s < window.size(); s++) if (window[s] == col) return (int)s; return -1; };
      bool missing = false;
      for (int k = 0; k < in.nsrc(); k++)
        if (gate_program::is_column(in.kind[k]) && slot_of(column_of(in, k)) < 0) missing = true;
      if (missing) {  // open a new window from here
        window.clear();
        for (u32 q = pc; q < last && window.size() < QUOTIENT_STAGE; q++) {
          const Insn ahead(code[2 * q], code[2 * q + 1]);
          std::vector<u32> need;
          for (int k = 0; k < ahead.nsrc(); k++)
            if (gate_program::is_column(ahead.kind[k])) {
              const u32 col = column_of(ahead, k);
              bool have = false;
              for (u32 c : window) have = have || c == col;
              for (u32 c : need) have = have || c == col;
              if (!have) need.push_back(col);
            }
          if (window.size() + need.size() > QUOTIENT_STAGE) break;  // an instruction's operands never straddle two windows
          window.insert(window.end(), need.begin(), need.end());
        }
        out.push_back(QOP_LDG | (u32)window.size() << 8);
        out.push_back((u32)lists.size());
        lists.insert(lists.end(), window.begin(), window.end());
      }
      for (int k = 0; k < in.nsrc(); k++)
        if (gate_program::is_column(in.kind[k])) { in.idx[k] = (u32)slot_of(column_of(in, k)); in.kind[k] = QKIND_STAGE; }
      u32 w[2];
      in.encode(w);
      out.push_back(w[0]); out.push_back(w[1]);
    }
    G.code_offset = new_first;
    G.code_len = (u32)out.size() / 2 - new_first;
  }
  lists.resize(lists.size() + QUOTIENT_STAGE, 0);  // an LDG always reads entry 0 of its list: keep the tail readable
}

}  // namespace lcp2
