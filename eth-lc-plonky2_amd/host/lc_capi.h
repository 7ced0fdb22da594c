/*
 * lc_capi.h -- the C++ host layer's light-client workloads behind plain C entry points, so that a process that is not C++
 * (bench.py, the Python tests) drives the SAME path examples/lc_prover drives: the reference's main() (eth-lc-plonky2/src/main.rs:
 * 56-233: parse two updates, add_virtual_proof_target + register_public_input, builder.build(), set_proof_target, data.prove(pw),
 * data.verify(proof)) in-process, on a context and stream the caller owns.  lch_prove is data.prove(pw): witness generation (the
 * reference times generate_partial_witness inside prove(), src/main.rs:229-232) and lcp2_prove.
 * This is NOT part of the drop-in boundary (include/lcp2.h is): a plonky2 fork has its own CircuitBuilder.  No oracle, no CPU fallback.
 * Every function returns 0 or a negative lcp2_status; lch_last_error() says why (thread-local).
 */
#ifndef LC_CAPI_H
#define LC_CAPI_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/lcp2.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lch_session lch_session;

#define LCH_BLS_PROOF_STAND_IN 1u    /* the circuit also verifies, recursively, a proof with the BLS proof's 25 216 public inputs (stand-in statement circuit) */
#define LCH_SYNC_COMMITTEE_ONLY 2u   /* BASELINE configs[1]: the SyncCommitteeSSZ gadget of cur_json's next_sync_committee alone */
#define LCH_FILL_COPIES 4u           /* CircuitData::set_fill_copies(true): one host-written cell per variable class through lcp2_witness_fill_copies (off by default) */

#define LCH_COMPACT_BUILD 8u         /* CircuitBuilder::set_compact_build(true): no expanded matrix on the host, lcp2_circuit_create_from_rows builds the columns (off by default) */

typedef struct {
  uint32_t degree_bits;
  uint32_t num_public_inputs;
  uint64_t num_gates;          /* builder.num_gates() before padding */
  uint64_t proof_words;
  double build_ms;             /* CircuitBuilder -> build() on the host */
  double attach_ms;            /* lcp2_circuit_create: the preprocessed polynomials committed on the GPU */
  double inner_prove_ms;       /* LCH_BLS_PROOF_STAND_IN: the inner proof (not part of lch_prove) */
  uint32_t inner_degree_bits, inner_public_inputs;
  /* the phases of build_ms (lc::BuildTimes; step sessions): gadget code, selector and constant columns, identity sigmas, variable
   * classes, cycles - the last four are what LCH_COMPACT_BUILD leaves to the device - and what attach_ms uploaded for the columns */
  double build_gadgets_ms, build_matrix_ms, build_identity_ms, build_classes_ms, build_cycles_ms;
  uint64_t attach_upload_bytes;
} lch_info;

/* prev_json / cur_json: two consecutive light-client updates (beacon-API V1_5 layout or the layout of the reference's fixture files).
 * extra_committees: that many more SyncCommitteeSSZ gadgets in the same circuit (6 -> 7 207 two_to_one_sha256, 2.24 M gates, 2^22 rows:
 * the reference's scale made of real gadgets).  ctx: the caller's context (its device and stream); it must outlive the session. */
int lch_light_client_step_create(lcp2_ctx *ctx, const char *prev_json, const char *cur_json, uint32_t flags, uint32_t extra_committees, lch_session **out);
void lch_destroy(lch_session *s);
int lch_get_info(const lch_session *s, lch_info *out);
/* data.prove(pw): proof (info.proof_words) and public inputs (info.num_public_inputs), host buffers.  LCP2_E_UNSAT for a witness
 * the circuit does not accept. */
int lch_prove(lch_session *s, uint64_t *proof, size_t proof_words, uint64_t *public_inputs, size_t num_public_inputs);
/* data.verify(proof): LCP2_OK or LCP2_E_VERIFY */
int lch_verify(const lch_session *s, const uint64_t *proof, size_t proof_words, const uint64_t *public_inputs, size_t num_public_inputs);
/* data.verify for `count` proofs at once, Merkle paths and FRI queries on the session's context (lcp2_verify_batch); step and wrap
 * sessions alike.  proofs: count * info.proof_words, public_inputs: count * info.num_public_inputs, failed_checks: count (0 =
 * accepted, 1..7 the check lcp2_verify names).  LCP2_OK if every proof is accepted, LCP2_E_VERIFY if one is not. */
int lch_verify_batch(const lch_session *s, const uint64_t *proofs, size_t count, const uint64_t *public_inputs, int32_t *failed_checks);
/* Shrinking a proof by recursion (plonky2's test_size_optimized_recursion): lch_wrap_create builds a circuit under the standard wire
 * shape with the given FRI config (quotient_degree_factor 8, ConstantArityBits(4, 5)) that verifies one proof of `inner` - its verifier
 * data built in as constants - and registers the inner public inputs as its own; `inner` may itself be a wrap session and must outlive
 * the call only.  lch_wrap_prove proves it for one inner proof (inner_proof_words / num_inner_public_inputs: the inner session's
 * lch_get_info); LCP2_E_UNSAT if the inner proof does not verify.  lch_get_info, lch_verify, lch_expected_public_inputs (those of the
 * innermost session) and lch_destroy work on wrap sessions; lch_prove does not.  E.g. rate_bits 7 / cap_height 4 / 16 PoW bits /
 * 12 queries, then rate_bits 8 / cap_height 0 / 20 / 10. */
int lch_wrap_create(lcp2_ctx *ctx, const lch_session *inner, uint32_t rate_bits, uint32_t cap_height, uint32_t proof_of_work_bits,
                    uint32_t num_query_rounds, lch_session **out);
int lch_wrap_prove(lch_session *s, const uint64_t *inner_proof, size_t inner_proof_words, const uint64_t *inner_public_inputs,
                   size_t num_inner_public_inputs, uint64_t *proof, size_t proof_words, uint64_t *public_inputs, size_t num_public_inputs);
/* LCH_SYNC_COMMITTEE_ONLY: the native SSZ root the proved public inputs must equal (8 big-endian u32 words); else cur_state then new_state (16 words) */
int lch_expected_public_inputs(const lch_session *s, uint64_t *out, size_t count);
const char *lch_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
