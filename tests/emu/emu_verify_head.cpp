// TEST HARNESS (not product code): csrc/verify_head.hpp compiled for the CPU and run in the decomposition of the device head
// (csrc/kernels_verify_head.hip): per proof the canonical scan, the transcript on a GROUP-SHAPED sponge (16 lanes, state word j and
// staged word j in lane j, the permutation itself the one-lane one), the identity per (proof, slot) with the register file laid out
// as the kernel's LDS (register r of lane t at lds[r * 64 + t]) and sums that start poisoned, then the finish - next to verify_head(),
// the host's head over the same text.  Built by tests/test_verify_head_emu.py with g++ and included by
// tests/emu/sanitize_verify_head_main.cpp; never loaded by the package.
#include <cstring>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/verify_head.hpp"
#include "emu_rc.hpp"

using namespace lcp2;

namespace {
constexpr u32 EMU_LANES = 64;
constexpr u64 EMU_POISON = 0xFFFFFFFF0BADF00Dull;  // not canonical: no sum a slot writes holds it

struct EmuGroupSponge {
  const u64 *rc;
  u64 v[16], in[16];
  void reset() { for (u64 &w : v) w = 0; }
  void stage(const u64 *x, u32 at, u32 k) {
    for (u32 j = 0; j < 16; j++)
      if (j >= at && j < at + k) in[j] = gl_canon(x[j - at]);
  }
  void stage_value(u32 at, u64 value) {
    for (u32 j = 0; j < 16; j++)
      if (j == at) in[j] = value;
  }
  void duplex(u32 m) {
    for (u32 j = 0; j < 16; j++)
      if (j < m) v[j] = in[j];
    u64 s[12];
    for (u32 j = 0; j < 12; j++) s[j] = v[j];
    pos_permute(s, rc);
    for (u32 j = 0; j < 12; j++) v[j] = s[j];
  }
  u64 word(u32 i) const { return v[i]; }
  bool writer() const { return true; }
};
struct EmuLdsRegs {
  gl2 *mine;
  gl2 &operator[](u32 r) const { return mine[r * EMU_LANES]; }
};

struct EmuCircuit {
  std::vector<u64> imm, k_is;
  VerifierView v;
  EmuCircuit(const lcp2_circuit_desc *desc, const u64 *digest, const u64 *cap) : imm(desc->num_imm + 1, 0), k_is(desc->params.num_routed_wires) {
    for (size_t i = 0; i < desc->num_imm; i++) imm[i] = gl_canon(desc->imm[i]);
    for (u32 i = 0; i < desc->params.num_routed_wires; i++) k_is[i] = gl_canon(desc->k_is[i]);
    v.p = &desc->params; v.npi = desc->num_public_inputs; v.num_selectors = desc->num_selectors; v.num_gates = desc->num_gates;
    v.gates = desc->gates; v.code = desc->code; v.imm = imm.data(); v.k_is = k_is.data(); v.digest = digest; v.cs_cap = cap;
    v.code_words = desc->code_words; v.num_imm = desc->num_imm; v.num_regs = desc->num_regs ? desc->num_regs : 1;
  }
};

// the three kernels for proof `index` of a chunk (its lane is index % 64): 0, 2 or 3, and on 0 the challenge block
int emu_device_head(const EmuCircuit &C, const HeadLayout &H, const u64 *proof, const u64 *pis, u64 index, VqChallenge &out, HeadChallenges &hc,
                    std::vector<gl2> &parts) {
  EmuGroupSponge sp;
  sp.rc = emu_round_constants();
  memset(sp.in, 0, sizeof sp.in);
  if (const int rc = head_transcript(sp, H, proof, proof + H.final_poly, pis, C.v.digest, hc, out)) return rc;
  std::vector<gl2> lds((size_t)H.num_regs * EMU_LANES, gl2_make(EMU_POISON, EMU_POISON));
  parts.assign((size_t)(H.num_gates + 1) * HEAD_MAX_CHALLENGES, gl2_make(EMU_POISON, EMU_POISON));
  for (u32 slot = 0; slot <= H.num_gates; slot++) {
    gl2 *o = parts.data() + head_part_index(H, 0, slot);
    if (slot < H.num_gates) head_gate_slot(H, C.v.gates[slot], C.v.code, C.v.imm, proof, hc, EmuLdsRegs{lds.data() + index % EMU_LANES}, o);
    else head_terms(H, proof, C.v.k_is, hc, out.zeta, o);
  }
  return head_finish(H, proof, hc, parts.data(), out);
}
}  // namespace

extern "C" {

unsigned emu_head_block_bytes() { return sizeof(VqChallenge); }

// The head of every proof of a batch, twice: device_codes / device_blocks from the kernels' decomposition, host_codes / host_blocks
// from verify_head().  Codes are 0 (the head passes), 1 (a word >= p), 2 or 3; a block is written (count x emu_head_block_bytes())
// only where the code is 0 and stays zero elsewhere.  Returns 0, or -1 for a length that is not the circuit's (nothing is read).
int emu_head_batch(const lcp2_circuit_desc *desc, const unsigned long long *digest, const unsigned long long *proofs, unsigned long long proof_words,
                   unsigned long long count, const unsigned long long *public_inputs, unsigned long long num_public_inputs, int *device_codes,
                   int *host_codes, void *device_blocks, void *host_blocks) {
  const ProofLayout L(desc->params);
  if (proof_words != L.total || num_public_inputs != desc->num_public_inputs) return -1;
  const EmuCircuit C(desc, (const u64 *)digest, nullptr);
  const HeadLayout H = head_make_layout(C.v, L, C.v.num_regs);
  std::vector<gl2> parts;
  for (u64 i = 0; i < count; i++) {
    const u64 *proof = (const u64 *)proofs + i * proof_words, *pis = (const u64 *)public_inputs + i * num_public_inputs;
    VqChallenge dev, host;
    memset(&dev, 0, sizeof dev);
    memset(&host, 0, sizeof host);
    int dc = 0, hcode = 0;
    for (u64 w = 0; w < proof_words && !dc; w++)
      if (proof[w] >= GL_P) dc = hcode = 1;  // k_verify_canon
    if (!dc) {
      HeadChallenges hc = {};
      dc = emu_device_head(C, H, proof, pis, i, dev, hc, parts);
      if (dc) memset(&dev, 0, sizeof dev);
      // the host sees the words outside the query section only: a copy of exactly those
      std::vector<u64> outside(proof, proof + L.queries);
      outside.insert(outside.end(), proof + L.final_poly, proof + L.total);
      hcode = verify_head(C.v, L, outside.data(), outside.data() + L.queries, pis, host);
      if (hcode) memset(&host, 0, sizeof host);
    }
    device_codes[i] = dc; host_codes[i] = hcode;
    memcpy((char *)device_blocks + i * sizeof(VqChallenge), &dev, sizeof dev);
    memcpy((char *)host_blocks + i * sizeof(VqChallenge), &host, sizeof host);
  }
  return 0;
}

// The gate sums of one proof under its own challenges: combined[2 k ..] = the sum over the slots of head_gate_slot (registers in the
// LDS layout), reference[2 k ..] = gate_program::eval_gates_filtered over a plain register file, k < num_challenges.  Returns the
// transcript's code (0 or 2; nothing is written on 2).
int emu_head_gate_sums(const lcp2_circuit_desc *desc, const unsigned long long *digest, const unsigned long long *proof, const unsigned long long *public_inputs,
                       unsigned long long *combined, unsigned long long *reference) {
  const ProofLayout L(desc->params);
  const EmuCircuit C(desc, (const u64 *)digest, nullptr);
  const HeadLayout H = head_make_layout(C.v, L, C.v.num_regs);
  const u64 *w = (const u64 *)proof;
  OneLaneSponge sp;
  sp.rc = emu_round_constants();
  HeadChallenges hc = {};
  VqChallenge out;
  memset(&out, 0, sizeof out);
  if (const int rc = head_transcript(sp, H, w, w + H.final_poly, (const u64 *)public_inputs, C.v.digest, hc, out)) return rc;
  std::vector<gl2> lds((size_t)H.num_regs * EMU_LANES, gl2_make(EMU_POISON, EMU_POISON));
  gl2 sum[HEAD_MAX_CHALLENGES], ref[HEAD_MAX_CHALLENGES];
  for (gl2 &s : sum) s = base2(0);
  for (u32 g = 0; g < H.num_gates; g++) {
    gl2 part[HEAD_MAX_CHALLENGES];
    head_gate_slot(H, C.v.gates[g], C.v.code, C.v.imm, w, hc, EmuLdsRegs{lds.data() + g % EMU_LANES}, part);
    for (u32 k = 0; k < H.CH; k++) sum[k] = gl2_add(sum[k], part[k]);
  }
  ZetaAlg at_zeta{w + H.op_wires, w + H.op_constants, hc.pi_hash, H.num_selectors};
  gate_program::eval_gates_filtered(at_zeta, C.v.gates, C.v.num_gates, C.v.code, C.v.imm, H.num_selectors, hc.alphas, H.CH, ref);
  for (u32 k = 0; k < H.CH; k++) {
    combined[2 * k] = sum[k].c0; combined[2 * k + 1] = sum[k].c1;
    reference[2 * k] = ref[k].c0; reference[2 * k + 1] = ref[k].c1;
  }
  return 0;
}

}  // extern "C"
