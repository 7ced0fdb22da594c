// lcp2_verify_batch / lcp2_verify_batch_ex: data.verify(proof) for a batch of proofs of one circuit, the query phase on the device
// and, with LCP2_VERIFY_HEAD_DEVICE, the head too.
//
// Per chunk of the batch (as many proofs as the pinned staging buffer serves), with the HOST head:
//   1. check 1 on the device: k_verify_canon over every word, one flag per proof.  Host proofs go up into scratch first; of device
//      proofs the words outside the query section come down as two strided copies (head, tail) for the whole chunk.
//   2. the host, per proof that passed: verify_head (verify_head.hpp) - public-input hash, transcript, checks 2 and 3, reduced
//      openings, query indices - the code lcp2_verify runs, into one challenge block (verify_query.hpp VqChallenge).
//   3. the blocks go up, k_verify_paths and k_verify_fri (kernels_verify.hip) run every Merkle path and every FRI query, and the
//      status words (count x num_query_rounds) come down: one synchronisation for checks 4 to 7.
//   4. the verdict of a proof is the status of its first query that has one: the check lcp2_verify would have stopped at.
// With the DEVICE head nothing of a proof comes down: the chunk's public inputs go up, k_verify_canon, the three head kernels
// (kernels_verify_head.hip: they write the challenge blocks where the query kernels read them) and the two query kernels are queued,
// ONE copy brings the canon flags, the head codes and the status words, and ONE synchronisation ends the chunk.  The verdict of a
// proof is 1 if its flag is set, else its head code (2, 3) if it has one, else that of its statuses: the smallest check wins.
//
// Scratch slots of the context: 0 host proofs; 1 challenge blocks + flags + head codes + status words (+ transcript challenges and
// identity sums, device head); 2 heads and tails of device proofs (host head) or the chunk's public inputs and the circuit's gates,
// code, immediates, coset shifts and digest (device head, uploaded once per call); 3 the circuit's constants cap (once per call).
#include <algorithm>
#include <cstring>
#include <vector>
#include "internal.hpp"
#include "verify_head.hpp"

namespace lcp2 {
VerifierView verifier_view(const lcp2_circuit *c);
void launch_verify_canon(hipStream_t s, const u64 *proofs, u64 proof_words, u64 count, u32 *flags);
void launch_verify_paths(hipStream_t s, const VqLayout &V, const u64 *proofs, u64 count, const VqChallenge *challenges, const u64 *cs_cap, u32 *status,
                         const u64 *rc);
void launch_verify_fri(hipStream_t s, const VqLayout &V, const u64 *proofs, u64 count, const VqChallenge *challenges, u32 *status);
void launch_verify_head(hipStream_t s, const HeadLayout &H, const u64 *proofs, u64 proof_words, u64 count, const u64 *pis, const u64 *digest,
                        const lcp2_gate *gates, const uint32_t *code, const u64 *imm, const u64 *k_is, const u32 *flags, u32 *codes, HeadChallenges *hcs,
                        gl2 *parts, VqChallenge *challenges, const u64 *rc);
size_t verify_identity_lds_bytes(u32 num_regs);
}  // namespace lcp2
using namespace lcp2;

namespace {
inline size_t round64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
}

extern "C" int lcp2_verify_batch_ex(lcp2_ctx *ctx, const lcp2_circuit *c, const uint64_t *proofs, size_t proof_words, size_t count, lcp2_mem proofs_mem,
                                    const uint64_t *public_inputs, size_t num_public_inputs, int32_t *failed_checks, uint32_t flags) {
  if (!ctx || !c) return LCP2_E_INVALID;
  if (flags != LCP2_VERIFY_HEAD_HOST && flags != LCP2_VERIFY_HEAD_DEVICE) return ctx->fail(LCP2_E_INVALID, "verify batch: unknown flags");
  const VerifierView v = verifier_view(c);
  const lcp2_params &p = *v.p;
  const ProofLayout L(p);
  // an untrusted proof is only ever read through the layout of THIS circuit: refuse any other length before anything is read
  if (proof_words != L.total || num_public_inputs != v.npi) return ctx->fail(LCP2_E_INVALID, "verify batch: not this circuit's proof or public-input length");
  if (count == 0) return LCP2_OK;
  if (!proofs || ((size_t)proofs & 7) || !failed_checks || (v.npi && !public_inputs) || (proofs_mem != LCP2_MEM_HOST && proofs_mem != LCP2_MEM_DEVICE))
    return ctx->fail(LCP2_E_INVALID, "verify batch: null or misaligned argument");
  if (count > ((size_t)1 << 40) / proof_words) return ctx->fail(LCP2_E_INVALID, "verify batch: count too large");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  const VqLayout V = vq_make_layout(L, p);
  const u32 Q = p.num_query_rounds;
  const size_t head_words = L.queries, tail_words = L.total - L.final_poly, outside = head_words + tail_words;
  const bool on_device = proofs_mem == LCP2_MEM_DEVICE, dev_head = flags == LCP2_VERIFY_HEAD_DEVICE;
  const size_t pis_bytes = (size_t)v.npi * 8;
  const HeadLayout H = head_make_layout(v, L, std::max(v.num_regs, 1u));
  if (dev_head && verify_identity_lds_bytes(H.num_regs) > 65536) return ctx->fail(LCP2_E_INVALID, "verify batch: more registers than the device head holds");

  // staging, per proof.  Host head: [head and tail words (device proofs)] [flag] [challenge block] [status words].
  // Device head: [public inputs] [flag] [head code] [status words] - no word of a proof, no challenge block.
  const size_t per_proof = dev_head ? pis_bytes + 4 + 4 + (size_t)Q * 4 : (on_device ? outside * 8 : 0) + 4 + sizeof(VqChallenge) + (size_t)Q * 4, slack = 4 * 64;
  size_t chunk = std::min<size_t>(count, 4096);
  char *stage = (char *)ctx->pin;
  std::vector<char> pageable;
  if (stage && per_proof + slack <= lcp2_ctx::PIN_BYTES) {
    chunk = std::min(chunk, (lcp2_ctx::PIN_BYTES - slack) / per_proof);
  } else {  // no pinned buffer, or one proof's share does not fit it
    chunk = std::min<size_t>(chunk, 64);
    pageable.resize(chunk * per_proof + slack);
    stage = pageable.data();
  }
  // device, slot 1: [challenge blocks] then what comes down, in one piece for the device head: [flags][head codes][status]
  const size_t d_off_flags = round64(chunk * sizeof(VqChallenge)), d_off_codes = d_off_flags + round64(chunk * 4), d_off_status = d_off_codes + round64(chunk * 4),
               d_off_hcs = d_off_status + round64(chunk * (size_t)Q * 4), d_off_parts = d_off_hcs + round64(dev_head ? chunk * sizeof(HeadChallenges) : 0),
               d_work_bytes = d_off_parts + (dev_head ? chunk * (size_t)(v.num_gates + 1) * HEAD_MAX_CHALLENGES * sizeof(gl2) : 0);
  const size_t down_bytes = d_off_hcs - d_off_flags;  // <= chunk * (8 + 4 Q) + 3 * 64: inside the staging share and its slack
  // host staging: [outside words | public inputs] then the mirror of the device's [flags][head codes][status] (host head: the
  // challenge blocks in between)
  const size_t off_flags = round64(dev_head ? chunk * pis_bytes : on_device ? chunk * outside * 8 : 0),
               off_chal = off_flags + (dev_head ? 0 : round64(chunk * 4)),
               off_status = dev_head ? off_flags + (d_off_status - d_off_flags) : off_chal + round64(chunk * sizeof(VqChallenge));
  u64 *h_outside = (u64 *)stage;  // host head, device proofs
  u64 *h_pis = (u64 *)stage;      // device head
  u32 *h_flags = (u32 *)(stage + off_flags), *h_codes = (u32 *)(stage + off_flags + (d_off_codes - d_off_flags)), *h_status = (u32 *)(stage + off_status);
  VqChallenge *h_chal = (VqChallenge *)(stage + off_chal);

  char *d_work = nullptr, *d_circ = nullptr;
  u64 *d_cap = nullptr, *d_up = nullptr, *d_outside = nullptr;
  LCP2_TRY(scratch_ensure(ctx, 1, d_work_bytes, (void **)&d_work));
  LCP2_TRY(scratch_ensure(ctx, 3, L.capw * 8, (void **)&d_cap));
  // device head, slot 2: [public inputs of the chunk][gates][code][immediates][coset shifts][digest]
  const size_t c_off_gates = round64(chunk * pis_bytes), c_off_code = c_off_gates + round64(v.num_gates * sizeof(lcp2_gate)),
               c_off_imm = c_off_code + round64(v.code_words * 4), c_off_kis = c_off_imm + round64(v.num_imm * 8),
               c_off_digest = c_off_kis + round64((size_t)p.num_routed_wires * 8), c_bytes = c_off_digest + 64;
  if (dev_head) LCP2_TRY(scratch_ensure(ctx, 2, c_bytes, (void **)&d_circ));
  else if (on_device) LCP2_TRY(scratch_ensure(ctx, 2, chunk * outside * 8, (void **)&d_outside));
  if (!on_device) LCP2_TRY(scratch_ensure(ctx, 0, chunk * proof_words * 8, (void **)&d_up));
  VqChallenge *d_chal = (VqChallenge *)d_work;
  u32 *d_flags = (u32 *)(d_work + d_off_flags), *d_codes = (u32 *)(d_work + d_off_codes), *d_status = (u32 *)(d_work + d_off_status);
  LCP2_HIP(ctx, hipMemcpyAsync(d_cap, v.cs_cap, L.capw * 8, hipMemcpyHostToDevice, ctx->stream));
  if (dev_head) {
    LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_gates, v.gates, v.num_gates * sizeof(lcp2_gate), hipMemcpyHostToDevice, ctx->stream));
    if (v.code_words) LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_code, v.code, v.code_words * 4, hipMemcpyHostToDevice, ctx->stream));
    if (v.num_imm) LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_imm, v.imm, v.num_imm * 8, hipMemcpyHostToDevice, ctx->stream));
    LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_kis, v.k_is, (size_t)p.num_routed_wires * 8, hipMemcpyHostToDevice, ctx->stream));
    LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_digest, v.digest, 32, hipMemcpyHostToDevice, ctx->stream));
  }

  bool all_accepted = true;
  for (size_t at = 0; at < count; at += chunk) {
    const size_t B = std::min(chunk, count - at);
    const u64 *src = (const u64 *)proofs + at * proof_words, *d_proofs = src;
    if (!on_device) {
      LCP2_HIP(ctx, hipMemcpyAsync(d_up, src, B * proof_words * 8, hipMemcpyHostToDevice, ctx->stream));
      d_proofs = d_up;
    }
    LCP2_HIP(ctx, hipMemsetAsync(d_flags, 0, B * 4, ctx->stream));
    if (dev_head) {
      // ---- everything of the chunk is queued, then one copy and one synchronisation
      if (pis_bytes) {  // (the synchronisation that ended the chunk before has released the staging buffer)
        memcpy(h_pis, (const u64 *)public_inputs + at * v.npi, B * pis_bytes);
        LCP2_HIP(ctx, hipMemcpyAsync(d_circ, h_pis, B * pis_bytes, hipMemcpyHostToDevice, ctx->stream));
      }
      LCP2_HIP(ctx, hipMemsetAsync(d_status, 0xFF, B * (size_t)Q * 4, ctx->stream));  // VQ_STATUS_NONE
      {
        ProfScope ps(ctx, LCP2_K_OTHER, (double)B * proof_words * 8);
        launch_verify_canon(ctx->stream, d_proofs, proof_words, B, d_flags);
        launch_verify_head(ctx->stream, H, d_proofs, proof_words, B, (const u64 *)d_circ, (const u64 *)(d_circ + c_off_digest),
                           (const lcp2_gate *)(d_circ + c_off_gates), (const uint32_t *)(d_circ + c_off_code), (const u64 *)(d_circ + c_off_imm),
                           (const u64 *)(d_circ + c_off_kis), d_flags, d_codes, (HeadChallenges *)(d_work + d_off_hcs), (gl2 *)(d_work + d_off_parts), d_chal,
                           ctx->d_rc);
        launch_verify_paths(ctx->stream, V, d_proofs, B, d_chal, d_cap, d_status, ctx->d_rc);
        launch_verify_fri(ctx->stream, V, d_proofs, B, d_chal, d_status);
      }
      LCP2_HIP(ctx, hipGetLastError());
      LCP2_HIP(ctx, hipMemcpyAsync(h_flags, d_flags, down_bytes, hipMemcpyDeviceToHost, ctx->stream));
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
      for (size_t i = 0; i < B; i++) {
        const u32 check = h_flags[i] ? 1 : h_codes[i] ? h_codes[i] : vq_reduce_statuses(h_status + i * Q, Q);
        failed_checks[at + i] = (int32_t)check;
        if (check) all_accepted = false;
      }
      continue;
    }
    // ---- check 1, and the words outside the query sections of device proofs
    {
      ProfScope ps(ctx, LCP2_K_OTHER, (double)B * proof_words * 8);
      launch_verify_canon(ctx->stream, d_proofs, proof_words, B, d_flags);
      if (on_device) {
        launch_copy_2d(ctx->stream, d_outside, outside, d_proofs, proof_words, head_words, (u32)B);
        launch_copy_2d(ctx->stream, d_outside + head_words, outside, d_proofs + L.final_poly, proof_words, tail_words, (u32)B);
      }
    }
    LCP2_HIP(ctx, hipGetLastError());
    if (on_device) LCP2_HIP(ctx, hipMemcpyAsync(h_outside, d_outside, B * outside * 8, hipMemcpyDeviceToHost, ctx->stream));
    LCP2_HIP(ctx, hipMemcpyAsync(h_flags, d_flags, B * 4, hipMemcpyDeviceToHost, ctx->stream));
    LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // ---- host: transcript, checks 2 and 3, one challenge block per proof
    size_t live = 0;
    for (size_t i = 0; i < B; i++) {
      VqChallenge &ch = h_chal[i];
      int rc = 1;
      if (!h_flags[i]) {
        const u64 *head = on_device ? h_outside + i * outside : src + i * proof_words;
        const u64 *tail = on_device ? head + head_words : head + L.final_poly;
        rc = verify_head(v, L, head, tail, (const u64 *)public_inputs + (at + i) * v.npi, ch);
      }
      if (rc) { memset(&ch, 0, sizeof ch); all_accepted = false; } else live++;
      failed_checks[at + i] = rc;
    }
    if (!live) continue;
    // ---- checks 4 to 7
    LCP2_HIP(ctx, hipMemcpyAsync(d_chal, h_chal, B * sizeof(VqChallenge), hipMemcpyHostToDevice, ctx->stream));
    LCP2_HIP(ctx, hipMemsetAsync(d_status, 0xFF, B * (size_t)Q * 4, ctx->stream));  // VQ_STATUS_NONE
    {
      ProfScope ps(ctx, LCP2_K_OTHER, (double)live * Q * L.query_words * 8);
      launch_verify_paths(ctx->stream, V, d_proofs, B, d_chal, d_cap, d_status, ctx->d_rc);
      launch_verify_fri(ctx->stream, V, d_proofs, B, d_chal, d_status);
    }
    LCP2_HIP(ctx, hipGetLastError());
    LCP2_HIP(ctx, hipMemcpyAsync(h_status, d_status, B * (size_t)Q * 4, hipMemcpyDeviceToHost, ctx->stream));
    LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < B; i++) {
      if (failed_checks[at + i]) continue;
      const u32 check = vq_reduce_statuses(h_status + i * Q, Q);
      failed_checks[at + i] = (int32_t)check;
      if (check) all_accepted = false;
    }
  }
  return all_accepted ? LCP2_OK : LCP2_E_VERIFY;
}

extern "C" int lcp2_verify_batch(lcp2_ctx *ctx, const lcp2_circuit *c, const uint64_t *proofs, size_t proof_words, size_t count, lcp2_mem proofs_mem,
                                 const uint64_t *public_inputs, size_t num_public_inputs, int32_t *failed_checks) {
  return lcp2_verify_batch_ex(ctx, c, proofs, proof_words, count, proofs_mem, public_inputs, num_public_inputs, failed_checks, LCP2_VERIFY_HEAD_HOST);
}
