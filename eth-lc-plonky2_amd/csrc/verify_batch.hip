// lcp2_verify_batch: data.verify(proof) for a batch of proofs of one circuit, the query phase on the device.
//
// Per chunk of the batch (as many proofs as the pinned staging buffer serves):
//   1. check 1 on the device: k_verify_canon over every word, one flag per proof.  Host proofs go up into scratch first; of device
//      proofs the words outside the query section come down as two strided copies (head, tail) for the whole chunk.
//   2. the host, per proof that passed: verify_head (verifier.hip) - public-input hash, transcript, checks 2 and 3, reduced
//      openings, query indices - the code lcp2_verify runs, into one challenge block (verify_query.hpp VqChallenge).
//   3. the blocks go up, k_verify_paths and k_verify_fri (kernels_verify.hip) run every Merkle path and every FRI query, and the
//      status words (count x num_query_rounds) come down: one synchronisation for checks 4 to 7.
//   4. the verdict of a proof is the status of its first query that has one: the check lcp2_verify would have stopped at.
// Scratch slots of the context: 0 host proofs, 1 challenge blocks + status words + flags, 2 heads and tails of device proofs,
// 3 the circuit's constants cap (uploaded once per call).
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
}  // namespace lcp2
using namespace lcp2;

namespace {
inline size_t round64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
}

extern "C" int lcp2_verify_batch(lcp2_ctx *ctx, const lcp2_circuit *c, const uint64_t *proofs, size_t proof_words, size_t count, lcp2_mem proofs_mem,
                                 const uint64_t *public_inputs, size_t num_public_inputs, int32_t *failed_checks) {
  if (!ctx || !c) return LCP2_E_INVALID;
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
  const bool on_device = proofs_mem == LCP2_MEM_DEVICE;

  // staging, per proof: [head and tail words (device proofs)] [flag] [challenge block] [status words]
  const size_t per_proof = (on_device ? outside * 8 : 0) + 4 + sizeof(VqChallenge) + (size_t)Q * 4, slack = 4 * 64;
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
  const size_t off_flags = round64(on_device ? chunk * outside * 8 : 0), off_chal = off_flags + round64(chunk * 4),
               off_status = off_chal + round64(chunk * sizeof(VqChallenge));
  u64 *h_outside = (u64 *)stage;
  u32 *h_flags = (u32 *)(stage + off_flags), *h_status = (u32 *)(stage + off_status);
  VqChallenge *h_chal = (VqChallenge *)(stage + off_chal);

  // device: slot 1 = [challenge blocks][status][flags]
  const size_t d_off_status = round64(chunk * sizeof(VqChallenge)), d_off_flags = d_off_status + round64(chunk * (size_t)Q * 4);
  char *d_work = nullptr;
  u64 *d_cap = nullptr, *d_up = nullptr, *d_outside = nullptr;
  LCP2_TRY(scratch_ensure(ctx, 1, d_off_flags + round64(chunk * 4), (void **)&d_work));
  LCP2_TRY(scratch_ensure(ctx, 3, L.capw * 8, (void **)&d_cap));
  if (on_device) LCP2_TRY(scratch_ensure(ctx, 2, chunk * outside * 8, (void **)&d_outside));
  else LCP2_TRY(scratch_ensure(ctx, 0, chunk * proof_words * 8, (void **)&d_up));
  VqChallenge *d_chal = (VqChallenge *)d_work;
  u32 *d_status = (u32 *)(d_work + d_off_status), *d_flags = (u32 *)(d_work + d_off_flags);
  LCP2_HIP(ctx, hipMemcpyAsync(d_cap, v.cs_cap, L.capw * 8, hipMemcpyHostToDevice, ctx->stream));

  bool all_accepted = true;
  for (size_t at = 0; at < count; at += chunk) {
    const size_t B = std::min(chunk, count - at);
    const u64 *src = (const u64 *)proofs + at * proof_words, *d_proofs = src;
    if (!on_device) {
      LCP2_HIP(ctx, hipMemcpyAsync(d_up, src, B * proof_words * 8, hipMemcpyHostToDevice, ctx->stream));
      d_proofs = d_up;
    }
    // ---- check 1, and the words outside the query sections of device proofs
    LCP2_HIP(ctx, hipMemsetAsync(d_flags, 0, B * 4, ctx->stream));
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
