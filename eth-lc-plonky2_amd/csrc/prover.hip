// Host orchestration of the prover: lcp2_prove (= data.prove(pw)) and the C ABI of its seams.  build() is prover_build.hip, the
// stages are prover_stages.hip and prover_open.hip (whose FRI back end is fri_commit.hip), the handle they share is circuit_state.hpp.
//
// Follows plonky2 0.1.4 plonk/prover.rs::prove step by step; every heavy step is a
// kernel from kernels_*.hip on the context's stream.  The Fiat-Shamir challenger (row a14: a few hundred
// permutations) runs on the host between the commitments; it needs only the 512-byte caps, the opening
// values and the final polynomial, which are the only device-to-host copies before the query phase.
#include "circuit_state.hpp"

using namespace lcp2;

namespace {
// the three phases of the opening back to back (a circuit that holds every leaf block); what they drew stays in c->fo
int stage_fri_open(lcp2_circuit *c, gl2 zeta, HostChallenger &ch, u64 *proof) {
  if (c->sharded()) return c->ctx->fail(LCP2_E_INVALID, "sharded circuit: lcp2_fri_open_begin / _commit / _finish with their exchange steps");
  c->fo.zeta = zeta; c->fo.ch = ch;
  LCP2_TRY(fri_open_openings(c, proof));
  LCP2_TRY(fri_open_commit(c, proof));
  LCP2_TRY(fri_open_finish(c, proof));
  ch = c->fo.ch;
  return LCP2_OK;
}

// an lcp2_challenger of the caller <-> the host challenger.  A state with 8 buffered inputs (they duplex at once: never stored) or
// more than 8 outputs is none that lcp2_challenger_* produces
int load_challenger(const lcp2_challenger *chs, HostChallenger &ch) {
  if (chs->input_len >= 8 || chs->output_len > 8) return LCP2_E_INVALID;
  ch.load((const u64 *)chs->sponge, (const u64 *)chs->input, chs->input_len, (const u64 *)chs->output, chs->output_len);
  return LCP2_OK;
}
void save_challenger(const HostChallenger &ch, lcp2_challenger *chs) {
  ch.save((u64 *)chs->sponge, (u64 *)chs->input, chs->input_len, (u64 *)chs->output, chs->output_len);
}
}  // namespace

extern "C" int lcp2_prove(lcp2_circuit *c, const uint64_t *wires_in_, lcp2_mem wires_mem, const uint64_t *public_inputs_, size_t num_public_inputs,
                          uint64_t *proof_, size_t proof_words) {
  if (c && c->npi && !public_inputs_) return LCP2_E_INVALID;
  LCP2_TRY(entry_guard(c, {wires_in_, proof_}));
  if (num_public_inputs != c->npi) return c->ctx->fail(LCP2_E_INVALID, "lcp2_prove: public input count does not match the circuit");
  if (proof_words != ProofLayout(c->p).total) return c->ctx->fail(LCP2_E_INVALID, "lcp2_prove: proof buffer is not lcp2_proof_words() long");
  if (c->sharded()) return c->ctx->fail(LCP2_E_INVALID, "sharded circuit: drive the stages and their exchange steps (parallel.py ShardedProver)");
  const u64 *public_inputs = (const u64 *)public_inputs_;
  u64 *proof = (u64 *)proof_;
  const lcp2_params &p = c->p;
  const u32 CH = p.num_challenges;
  const ProofLayout L(p);
  memset(proof, 0, L.total * 8);
  HostPoseidon &H = HostPoseidon::get();
  std::vector<u64> pis(std::max<u32>(c->npi, 1), 0);
  for (u32 i = 0; i < c->npi; i++) pis[i] = gl_canon(public_inputs[i]);
  u64 pi_hash[4];
  H.hash_no_pad(pis.data(), c->npi, pi_hash);

  LCP2_TRY(stage_wires(c, (const u64 *)wires_in_, wires_mem, nullptr, proof + L.wires_cap));
  HostChallenger ch;
  ch.observe_n(c->digest, 4);
  ch.observe_n(pi_hash, 4);
  ch.observe_n(proof + L.wires_cap, L.capw);
  u64 betas[4] = {0}, gammas[4] = {0}, alphas[4] = {0};
  for (u32 k = 0; k < CH; k++) betas[k] = ch.get();
  for (u32 k = 0; k < CH; k++) gammas[k] = ch.get();
  LCP2_TRY(stage_perm_zs(c, betas, gammas, proof + L.zs_cap));
  ch.observe_n(proof + L.zs_cap, L.capw);
  for (u32 k = 0; k < CH; k++) alphas[k] = ch.get();
  LCP2_TRY(stage_quotient(c, alphas, pi_hash, proof + L.quot_cap));
  ch.observe_n(proof + L.quot_cap, L.capw);
  const gl2 zeta = ch.get_ext();
  LCP2_TRY(stage_fri_open(c, zeta, ch, proof));
  // record the transcript for stage-wise parity tests
  const FriOpenState &fo = c->fo;
  u64 *lc = c->last_challenges;
  memset(lc, 0, sizeof c->last_challenges);
  memcpy(lc, betas, 32); memcpy(lc + 4, gammas, 32); memcpy(lc + 8, alphas, 32);
  lc[12] = zeta.c0; lc[13] = zeta.c1; lc[14] = fo.alpha.c0; lc[15] = fo.alpha.c1;
  for (u32 l = 0; l < p.num_fri_layers; l++) { lc[16 + 2 * l] = fo.fri_betas[l].c0; lc[17 + 2 * l] = fo.fri_betas[l].c1; }
  lc[32] = fo.pow_witness;
  for (u32 q = 0; q < p.num_query_rounds; q++) lc[33 + q] = fo.idx[q];
  return LCP2_OK;
}

// ---- staged host witnesses: the upload of the next witness overlaps the proof in flight (include/lcp2.h)
extern "C" int lcp2_witness_stage(lcp2_circuit *c, const uint64_t *wires, uint32_t slot) {
  if (slot > 1) return LCP2_E_INVALID;
  LCP2_TRY(entry_guard(c, {wires}));
  lcp2_ctx *ctx = c->ctx;
  if (c->sharded()) return ctx->fail(LCP2_E_INVALID, "lcp2_witness_stage: a sharded circuit takes its witness shard by shard");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)c->p.num_wires * 8 << c->p.degree_bits;
  if (!ctx->copy_stream) LCP2_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  if (!c->wit_ready[slot]) LCP2_HIP(ctx, hipEventCreateWithFlags(&c->wit_ready[slot], hipEventDisableTiming));
  LCP2_HIP(ctx, c->wit_slot[slot].ensure(bytes));
  LCP2_HIP(ctx, hipMemcpyAsync(c->wit_slot[slot].p, wires, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
  LCP2_HIP(ctx, hipEventRecord(c->wit_ready[slot], ctx->copy_stream));
  c->wit_staged[slot] = true;
  return LCP2_OK;
}
extern "C" int lcp2_prove_staged(lcp2_circuit *c, uint32_t slot, const uint64_t *public_inputs, size_t num_public_inputs, uint64_t *proof, size_t proof_words) {
  if (slot > 1) return LCP2_E_INVALID;
  LCP2_TRY(entry_guard(c));  // the buffers are lcp2_prove's to check
  if (!c->wit_staged[slot]) return c->ctx->fail(LCP2_E_INVALID, "lcp2_prove_staged: nothing has been staged into this slot");
  LCP2_HIP(c->ctx, hipStreamWaitEvent(c->ctx->stream, c->wit_ready[slot], 0));  // the stream waits for the upload, the host does not
  c->wit_staged[slot] = false;
  return lcp2_prove(c, (const uint64_t *)c->wit_slot[slot].p, LCP2_MEM_DEVICE, public_inputs, num_public_inputs, proof, proof_words);
}

// ---- C ABI of the seams (include/lcp2.h)
extern "C" int lcp2_commit_wires(lcp2_circuit *c, const uint64_t *wires, lcp2_mem mem, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {wires, cap}));
  return stage_wires(c, (const u64 *)wires, mem, nullptr, (u64 *)cap);
}
extern "C" int lcp2_commit_wires_coeffs(lcp2_circuit *c, const uint64_t *wires, const uint64_t *coeffs, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {wires, coeffs, cap}));
  return stage_wires(c, (const u64 *)wires, LCP2_MEM_DEVICE, (const u64 *)coeffs, (u64 *)cap);
}
extern "C" int lcp2_commit_wires_rows(lcp2_circuit *c, const uint64_t *wire_rows, const uint64_t *coeffs, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {wire_rows, coeffs, cap}));
  return stage_wires(c, (const u64 *)wire_rows, LCP2_MEM_DEVICE, (const u64 *)coeffs, (u64 *)cap, true);
}
extern "C" int lcp2_perm_zs_rows_begin(lcp2_circuit *c, const uint64_t *betas, const uint64_t *gammas, uint64_t *block_products) {
  LCP2_TRY(entry_guard(c, {betas, gammas, block_products}));
  if (!c->rows_mode) return c->ctx->fail(LCP2_E_INVALID, "lcp2_perm_zs_rows_begin: the wires were not committed with lcp2_commit_wires_rows");
  c->perm_phase = 0;
  LCP2_TRY(perm_begin(c, (const u64 *)betas, (const u64 *)gammas));
  {
    Download d(c->ctx);
    LCP2_TRY(queue_perm_wrap(d, c));
    LCP2_TRY(d.wait());
  }
  const u32 CH = c->p.num_challenges;
  memset(block_products, 0, (size_t)c->world() * CH * 8);
  for (u32 k = 0; k < CH; k++) block_products[(size_t)c->rank() * CH + k] = gl_mul(c->perm_wrap[2 * k], c->perm_wrap[2 * k + 1]);
  c->perm_phase = 1;
  return LCP2_OK;
}
extern "C" int lcp2_perm_zs_rows_finish(lcp2_circuit *c, const uint64_t *block_products, uint64_t **device_ptr, size_t *words) {
  LCP2_TRY(entry_guard(c, {block_products, device_ptr, words}));
  if (!c->rows_mode || c->stage < lcp2_circuit::ST_WIRES || c->perm_phase != 1)
    return c->ctx->fail(LCP2_E_INVALID, "lcp2_perm_zs_rows_finish: lcp2_perm_zs_rows_begin has not run for this proof");
  const u32 CH = c->p.num_challenges;
  u64 prefix[QUOTIENT_MAX_CH];
  for (u32 k = 0; k < CH; k++) {
    u64 all = 1;
    prefix[k] = 1;
    for (u32 r = 0; r < c->world(); r++) {
      if (r == c->rank()) prefix[k] = all;
      all = gl_mul(all, gl_canon(block_products[(size_t)r * CH + k]));
    }
    // every rank sees the same products: all of them report the broken copy constraint (stage_perm_zs has the argument)
    if (all != 1) return c->ctx->fail(LCP2_E_UNSAT, "the witness violates a copy constraint (the permutation product does not return to 1)");
  }
  LCP2_TRY(perm_finish(c, prefix));
  c->perm_phase = 2;
  *device_ptr = (uint64_t *)c->zs_rows.p;
  *words = (size_t)CH * (1 + npp_of(c->p)) << c->p.degree_bits;
  return LCP2_OK;
}
extern "C" int lcp2_perm_zs_commit(lcp2_circuit *c, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {cap}));
  if (!c->rows_mode || c->stage < lcp2_circuit::ST_WIRES || c->perm_phase != 2)
    return c->ctx->fail(LCP2_E_INVALID, "lcp2_perm_zs_commit: lcp2_perm_zs_rows_finish has not run for this proof");
  c->perm_phase = 0;
  return perm_commit(c, (u64 *)cap);
}
extern "C" int lcp2_perm_zs(lcp2_circuit *c, const uint64_t *betas, const uint64_t *gammas, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {betas, gammas, cap}));
  return stage_perm_zs(c, (const u64 *)betas, (const u64 *)gammas, (u64 *)cap);
}
extern "C" int lcp2_quotient(lcp2_circuit *c, const uint64_t *alphas, const uint64_t public_inputs_hash[4], uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {alphas, cap, public_inputs_hash}));
  return stage_quotient(c, (const u64 *)alphas, (const u64 *)public_inputs_hash, (u64 *)cap);
}
extern "C" int lcp2_quotient_values(lcp2_circuit *c, const uint64_t *alphas, const uint64_t public_inputs_hash[4]) {
  LCP2_TRY(entry_guard(c, {alphas, public_inputs_hash}));
  return stage_quotient_values(c, (const u64 *)alphas, (const u64 *)public_inputs_hash);
}
extern "C" int lcp2_quotient_buffer(lcp2_circuit *c, uint64_t **device_ptr, size_t *words) {
  LCP2_TRY(entry_guard(c, {device_ptr, words}));
  *device_ptr = (uint64_t *)c->qvals.p;
  *words = ((size_t)c->p.num_challenges << (c->p.degree_bits + c->qbits()));
  return LCP2_OK;
}
extern "C" int lcp2_quotient_commit(lcp2_circuit *c, uint64_t *cap) {
  LCP2_TRY(entry_guard(c, {cap}));
  return stage_quotient_commit(c, (u64 *)cap);
}
// host-side transcript helpers (plonky2 Challenger / PoseidonHash::hash_no_pad) for callers without their own
extern "C" void lcp2_challenger_init(lcp2_challenger *ch) { if (ch) memset(ch, 0, sizeof *ch); }
extern "C" int lcp2_challenger_observe(lcp2_challenger *chs, const uint64_t *values, size_t count) {
  if (!chs || (count && !values)) return LCP2_E_INVALID;
  HostChallenger ch;
  LCP2_TRY(load_challenger(chs, ch));
  ch.observe_n((const u64 *)values, count);
  save_challenger(ch, chs);
  return LCP2_OK;
}
extern "C" int lcp2_challenger_get(lcp2_challenger *chs, uint64_t *out, size_t count) {
  if (!chs || (count && !out)) return LCP2_E_INVALID;
  HostChallenger ch;
  LCP2_TRY(load_challenger(chs, ch));
  for (size_t i = 0; i < count; i++) out[i] = ch.get();
  save_challenger(ch, chs);
  return LCP2_OK;
}
extern "C" int lcp2_hash_no_pad(const uint64_t *values, size_t count, uint64_t out[4]) {
  if ((count && !values) || !out) return LCP2_E_INVALID;
  std::vector<u64> v(std::max<size_t>(count, 1), 0);
  for (size_t i = 0; i < count; i++) v[i] = gl_canon(values[i]);
  u64 h[4];
  HostPoseidon::get().hash_no_pad(v.data(), count, h);
  memcpy(out, h, 32);
  return LCP2_OK;
}

extern "C" int lcp2_fri_open(lcp2_circuit *c, const uint64_t zeta[2], lcp2_challenger *chs, uint64_t *proof) {
  LCP2_TRY(entry_guard(c, {zeta, chs, proof}));
  HostChallenger ch;
  LCP2_TRY(load_challenger(chs, ch));
  LCP2_TRY(stage_fri_open(c, gl2_make(gl_canon(zeta[0]), gl_canon(zeta[1])), ch, (u64 *)proof));
  save_challenger(ch, chs);
  return LCP2_OK;
}

// the same stage in its three phases, for a coset-sharded proof (and for callers that want the exchange points)
extern "C" int lcp2_fri_open_begin(lcp2_circuit *c, const uint64_t zeta[2], const lcp2_challenger *chs, uint64_t *proof) {
  LCP2_TRY(entry_guard(c, {zeta, chs, proof}));
  LCP2_TRY(load_challenger(chs, c->fo.ch));
  c->fo.phase = 0;
  c->fo.zeta = gl2_make(gl_canon(zeta[0]), gl_canon(zeta[1]));
  return fri_open_openings(c, (u64 *)proof);
}
extern "C" int lcp2_fri_open_commit(lcp2_circuit *c, uint64_t *proof) {
  LCP2_TRY(entry_guard(c, {proof}));
  return fri_open_commit(c, (u64 *)proof);
}
extern "C" int lcp2_fri_open_finish(lcp2_circuit *c, lcp2_challenger *chs, uint64_t *proof) {
  LCP2_TRY(entry_guard(c, {proof}));
  LCP2_TRY(fri_open_finish(c, (u64 *)proof));
  if (chs) save_challenger(c->fo.ch, chs);
  return LCP2_OK;
}
extern "C" int lcp2_proof_section(const lcp2_circuit *c, int section, size_t *first_word, size_t *num_words) {
  if (!c || !first_word || !num_words) return LCP2_E_INVALID;
  const ProofLayout L(c->p);
  switch (section) {
    case LCP2_SECTION_OPENINGS: *first_word = L.op_constants; *num_words = L.fri_caps - L.op_constants; return LCP2_OK;
    case LCP2_SECTION_FRI_CAP0: *first_word = L.fri_caps; *num_words = c->p.num_fri_layers ? L.capw : 0; return LCP2_OK;
    case LCP2_SECTION_AFTER_CAPS: *first_word = L.op_constants; *num_words = L.total - L.op_constants; return LCP2_OK;
  }
  return LCP2_E_INVALID;
}
