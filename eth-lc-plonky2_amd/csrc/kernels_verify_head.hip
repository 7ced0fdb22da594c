// Kernels of lcp2_verify_batch_ex with LCP2_VERIFY_HEAD_DEVICE (verify_batch.hip): checks 2 and 3 of data.verify(proof) and the
// challenge blocks of the query kernels (kernels_verify.hip), made on the device.  verify_head.hpp holds the text they run.
//
//  k_verify_transcript   one 16-lane group per proof (four proofs per wave), state word j of the sponge in lane j, round constants
//                        in LDS (poseidon.hpp pos_permute_coop): public-input hash, the observe / get sequence, proof of work, query
//                        indices.  Absorbed words are loaded by the lanes that hold them, straight from the proof.  A chain of some
//                        136 + ceil(npi / 8) dependent permutations: latency bound.  Writes head code 0 or 2.
//  k_verify_identity     grid = (blocks of 64 proofs) x (num_gates + 1), one lane per proof.  blockIdx.y < num_gates walks that gate's
//                        program on the openings of the lane's proof - every lane of a wave the same program, so control flow is
//                        wave-uniform - with the gl2 register file in LDS, register r of lane t at lds[r * 64 + t]; the last slot
//                        computes the L_0 and permutation terms.  Openings are read from the proof in HBM where they lie.
//  k_verify_head_finish  one lane per proof: sums and terms under alpha against Z_H(zeta) t(zeta) (head code 3), the reduced
//                        openings, and `live` of the challenge block: 0 if the proof's canon flag or head code is set.
//
// No proof content steers an address: programs, offsets and counts are the circuit's (validated when the handle was made), and the
// query indices are reduced below N.  A proof whose canon flag is set is skipped by all three (its verdict is 1 whatever they say).
#include "internal.hpp"
#include "poseidon.hpp"
#include "verify_head.hpp"

namespace lcp2 {

constexpr int HEAD_TRANSCRIPT_THREADS = 256, HEAD_LANES = 64;

// the sponge provider of a 16-lane group: lane j holds state word j and staged word j
struct GroupSponge {
  const u64 *rcs;  // LDS copy of the round constants
  u32 j;
  u64 v, in;
  __device__ __forceinline__ void reset() { v = 0; }
  __device__ __forceinline__ void stage(const u64 *x, u32 at, u32 k) { if (j >= at && j < at + k) in = gl_canon(x[j - at]); }
  __device__ __forceinline__ void stage_value(u32 at, u64 value) { if (j == at) in = value; }
  __device__ __forceinline__ void duplex(u32 m) { if (j < m) v = in; v = pos_permute_coop(v, j, rcs); }
  __device__ __forceinline__ u64 word(u32 i) const { return __shfl(v, (int)i, 16); }
  __device__ __forceinline__ bool writer() const { return j == 0; }
};

__global__ __launch_bounds__(HEAD_TRANSCRIPT_THREADS) void k_verify_transcript(const HeadLayout H, const u64 *__restrict__ proofs, u64 proof_words, u64 count,
                                                                               const u64 *__restrict__ pis, const u64 *__restrict__ digest,
                                                                               const u32 *__restrict__ flags, HeadChallenges *__restrict__ hcs,
                                                                               VqChallenge *__restrict__ challenges, u32 *__restrict__ codes,
                                                                               const u64 *__restrict__ rc) {
  __shared__ u64 rcs[POS_ROUNDS * POS_W];
  for (u32 i = threadIdx.x; i < POS_ROUNDS * POS_W; i += HEAD_TRANSCRIPT_THREADS) rcs[i] = rc[i];
  __syncthreads();
  const u64 t = (u64)blockIdx.x * HEAD_TRANSCRIPT_THREADS + threadIdx.x, proof = t >> 4;
  if (proof >= count) return;  // whole groups
  GroupSponge sp;
  sp.rcs = rcs; sp.j = (u32)t & 15; sp.v = 0; sp.in = 0;
  int code = 0;
  if (!flags[proof]) {
    const u64 *w = proofs + proof * proof_words;
    code = head_transcript(sp, H, w, w + H.final_poly, pis + proof * H.npi, digest, hcs[proof], challenges[proof]);
  }
  if (sp.writer()) codes[proof] = (u32)code;
}

// register r of this lane: one gl2 per lane and register, lanes adjacent
struct LdsRegs {
  gl2 *mine;
  __device__ __forceinline__ gl2 &operator[](u32 r) const { return mine[r * HEAD_LANES]; }
};

__global__ __launch_bounds__(HEAD_LANES) void k_verify_identity(const HeadLayout H, const u64 *__restrict__ proofs, u64 proof_words, u64 count,
                                                                 const lcp2_gate *__restrict__ gates, const uint32_t *__restrict__ code,
                                                                 const u64 *__restrict__ imm, const u64 *__restrict__ k_is,
                                                                 const u32 *__restrict__ flags, const u32 *__restrict__ codes,
                                                                 const HeadChallenges *__restrict__ hcs, const VqChallenge *__restrict__ challenges,
                                                                 gl2 *__restrict__ parts) {
  extern __shared__ __align__(16) unsigned char head_lds[];  // num_regs * HEAD_LANES registers
  const u64 proof = (u64)blockIdx.x * HEAD_LANES + threadIdx.x;
  if (proof >= count || flags[proof] || codes[proof]) return;
  const u32 slot = blockIdx.y;  // <= H.num_gates
  const u64 *w = proofs + proof * proof_words;
  gl2 *out = parts + head_part_index(H, proof, slot);
  if (slot < H.num_gates) head_gate_slot(H, gates[slot], code, imm, w, hcs[proof], LdsRegs{(gl2 *)head_lds + threadIdx.x}, out);
  else head_terms(H, w, k_is, hcs[proof], challenges[proof].zeta, out);
}

__global__ __launch_bounds__(HEAD_LANES) void k_verify_head_finish(const HeadLayout H, const u64 *__restrict__ proofs, u64 proof_words, u64 count,
                                                                    const u32 *__restrict__ flags, u32 *__restrict__ codes,
                                                                    const HeadChallenges *__restrict__ hcs, const gl2 *__restrict__ parts,
                                                                    VqChallenge *__restrict__ challenges) {
  const u64 proof = (u64)blockIdx.x * HEAD_LANES + threadIdx.x;
  if (proof >= count) return;
  VqChallenge &c = challenges[proof];
  if (flags[proof] || codes[proof]) { c.live = 0; c.pad = 0; return; }
  const int rc = head_finish(H, proofs + proof * proof_words, hcs[proof], parts + head_part_index(H, proof, 0), c);
  if (rc) { codes[proof] = (u32)rc; c.live = 0; c.pad = 0; }
}

// LDS of k_verify_identity for a circuit of num_regs registers: at the ABI's maximum of 64 registers 64 KiB, the static limit
size_t verify_identity_lds_bytes(u32 num_regs) { return (size_t)num_regs * HEAD_LANES * sizeof(gl2); }

// flags: the canon flags of the proofs (k_verify_canon, queued before).  Writes codes[count] (0, 2 or 3), hcs and parts (scratch)
// and the whole challenge block of every proof that passes.
void launch_verify_head(hipStream_t s, const HeadLayout &H, const u64 *proofs, u64 proof_words, u64 count, const u64 *pis, const u64 *digest,
                        const lcp2_gate *gates, const uint32_t *code, const u64 *imm, const u64 *k_is, const u32 *flags, u32 *codes, HeadChallenges *hcs,
                        gl2 *parts, VqChallenge *challenges, const u64 *rc) {
  if (!count) return;
  const unsigned groups = (unsigned)((count * 16 + HEAD_TRANSCRIPT_THREADS - 1) / HEAD_TRANSCRIPT_THREADS);
  const unsigned blocks = (unsigned)((count + HEAD_LANES - 1) / HEAD_LANES);
  hipLaunchKernelGGL(k_verify_transcript, dim3(groups), dim3(HEAD_TRANSCRIPT_THREADS), 0, s, H, proofs, proof_words, count, pis, digest, flags, hcs,
                     challenges, codes, rc);
  hipLaunchKernelGGL(k_verify_identity, dim3(blocks, H.num_gates + 1), dim3(HEAD_LANES), verify_identity_lds_bytes(H.num_regs), s, H, proofs, proof_words,
                     count, gates, code, imm, k_is, flags, codes, hcs, challenges, parts);
  hipLaunchKernelGGL(k_verify_head_finish, dim3(blocks), dim3(HEAD_LANES), 0, s, H, proofs, proof_words, count, flags, codes, hcs, parts, challenges);
}

}  // namespace lcp2
