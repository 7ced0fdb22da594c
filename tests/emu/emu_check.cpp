// TEST HARNESS (not product code): csrc/witness_check.hpp compiled for the CPU - the walk of the STAGED gate programs with the
// counting sink, lane by lane the way k_witness_gates runs it (blocks of T lanes, the tail lanes of the last block repeating the
// last row without being counted), the cell-id decode, and the copy check of every routed cell.  The programs are staged by the
// library's own pass (csrc/gate_staging.hpp).  tests/test_witness_check_emu.py holds the results to orc_check_witness and to a
// numpy reference.  Built by tests/rows_lib.py build_emu with g++; never loaded by the package.
#include <cstring>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/witness_check.hpp"
#include "../../eth-lc-plonky2_amd/csrc/ntt_host.hpp"

using namespace lcp2;

namespace {
struct CpuMem {
  const uint32_t *code, *lists;
  const u64 *wires, *consts, *imm, *pis;
  u64 n, i;
  u32 num_wires, num_selectors;
  u64 regs[256], slots[QUOTIENT_STAGE];
  u64 insn(u32 pc) const { return code[2 * pc] | (u64)code[2 * pc + 1] << 32; }
  void stage(u32 cnt, u32 off) {
    for (u32 j = 0; j < cnt; j++) {
      const u32 e = lists[off + j];
      slots[j] = gl_canon(e < num_wires ? wires[(u64)e * n + i] : consts[(u64)(e - num_wires) * n + i]);
    }
  }
  u64 operand(u32 kind, u32 idx) const {
    switch (kind) {
      case 0: return regs[idx];
      case 1: return gl_canon(wires[(u64)idx * n + i]);
      case 2: return gl_canon(consts[(u64)(num_selectors + idx) * n + i]);
      case 3: return imm[idx];
      case 4: return pis[idx];
      default: return slots[idx];
    }
  }
  u64 reg(u32 r) const { return regs[r]; }
  void set_reg(u32 r, u64 v) { regs[r] = v; }
  void pmds(u32 dst, u32 src, u32 imm_offset) {
    using namespace gate_program;
    u64 x[MDS_WIDTH];
    for (u32 k = 0; k < MDS_WIDTH; k++) x[k] = regs[src + k];
    for (u32 r = 0; r < MDS_WIDTH; r++) {
      u64 t = gl_add(imm[imm_offset + r], gl_mul(x[r], MDS_DIAG[r]));
      for (u32 k = 0; k < MDS_WIDTH; k++) t = gl_add(t, gl_mul(x[(k + r) % MDS_WIDTH], MDS_CIRC[k]));
      regs[dst + r] = t;
    }
  }
  u64 sbox(u64 x) const { const u64 x2 = gl_sqr(x), x4 = gl_sqr(x2); return gl_mul(gl_mul(x2, x), x4); }
};

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
}  // namespace

extern "C" {
// d: lcp2_circuit_desc with host constants_sigmas; wires [num_wires][n]; pi_hash[4]; T: lanes per block.
// out[0] = violations, out[1] = the first as wc_gate_key (WC_NONE: none); per_gate [num_gates] (nullable)
int emu_check_gates(const lcp2_circuit_desc *d, const u64 *wires, const u64 *pi_hash, unsigned T, u64 *out, u64 *per_gate) {
  const lcp2_params &p = d->params;
  const u64 n = 1ull << p.degree_bits;
  std::vector<uint32_t> code(d->code, d->code + d->code_words), staged, lists;
  std::vector<lcp2_gate> gates(d->gates, d->gates + d->num_gates);
  if (gates.size() >= WC_MAX_GATES) return LCP2_E_UNSUPPORTED;
  for (const lcp2_gate &G : gates) if (G.num_constraints >= WC_MAX_CONSTRAINTS) return LCP2_E_UNSUPPORTED;
  stage_programs(code, gates, p.num_wires, d->num_selectors, staged, lists);
  staged.resize(staged.size() + 4, 0);
  std::vector<u64> imm(d->num_imm ? d->num_imm : 1, 0);
  for (size_t k = 0; k < d->num_imm; k++) imm[k] = gl_canon(d->imm[k]);
  CpuMem m{};
  m.code = staged.data(); m.lists = lists.data(); m.wires = wires; m.consts = (const u64 *)d->constants_sigmas; m.imm = imm.data(); m.pis = pi_hash;
  m.n = n; m.num_wires = p.num_wires; m.num_selectors = d->num_selectors;
  u64 total = 0, first = WC_NONE;
  if (per_gate) memset(per_gate, 0, gates.size() * 8);
  for (u64 block = 0; block * T < n; block++)
    for (u32 lane = 0; lane < T; lane++) {
      const u64 i0 = block * T + lane;
      const bool live = i0 < n;
      m.i = live ? i0 : n - 1;
      for (u32 g = 0; g < gates.size(); g++) {
        const lcp2_gate &G = gates[g];
        if (G.num_constraints == 0) continue;
        if (gl_canon(m.consts[(u64)G.selector_index * n + m.i]) != G.selector_value) continue;
        WcCount sink;
        sink.begin(G.num_constraints, G.flags);
        wc_walk(m, G.code_offset, G.code_len, sink);
        if (sink.emitted != G.num_constraints) return LCP2_E_INVALID;
        if (live && sink.count) {
          total += sink.count;
          if (per_gate) per_gate[g] += sink.count;
          const u64 k = wc_gate_key(m.i, g, sink.first);
          if (k < first) first = k;
        }
      }
    }
  out[0] = total; out[1] = first;
  return 0;
}

// count values s[] -> wire[] (WC_NO_WIRE: no cell id), row[]
void emu_decode_cells(const u64 *k_is, unsigned num_routed, unsigned degree_bits, const u64 *s, u64 count, uint32_t *wire, u64 *row) {
  Roots R(k_is, num_routed, degree_bits);
  for (u64 k = 0; k < count; k++) {
    const WcCell c = wc_decode_cell(R.t, s[k]);
    wire[k] = c.wire; row[k] = c.row;
  }
}

// every routed cell: out[0] = violations, out[1] = the first as wc_copy_key, out[2], out[3] = wire and row of its partner
void emu_check_copies(const lcp2_circuit_desc *d, const u64 *wires, u64 *out) {
  const lcp2_params &p = d->params;
  const u64 n = 1ull << p.degree_bits;
  const u32 NR = p.num_routed_wires;
  const u64 *k_is = (const u64 *)d->k_is;
  Roots R(k_is, NR, p.degree_bits);
  const u64 *sigmas = (const u64 *)d->constants_sigmas + (u64)p.num_constants * n;
  u64 total = 0, first = WC_NONE;
  for (u32 j = 0; j < NR; j++)
    for (u64 r = 0; r < n; r++)
      if (wc_copy_violated(R.t, wires, sigmas, n, j, r, gl_mul(gl_canon(k_is[j]), two_level(R.t.roots, r)), nullptr)) {
        total++;
        if (wc_copy_key(r, j) < first) first = wc_copy_key(r, j);
      }
  out[0] = total; out[1] = first; out[2] = WC_NO_WIRE; out[3] = ~0ull;
  if (first != WC_NONE) {
    WcCell to;
    const u32 j = (u32)first;
    const u64 r = first >> 32;
    wc_copy_violated(R.t, wires, sigmas, n, j, r, gl_mul(gl_canon(k_is[j]), two_level(R.t.roots, r)), &to);
    out[2] = to.wire; out[3] = to.wire == WC_NO_WIRE ? ~0ull : to.row;
  }
}
}
