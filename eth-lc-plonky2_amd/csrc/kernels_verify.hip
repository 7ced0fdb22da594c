// Kernels of lcp2_verify_batch (verify_batch.hip): the query phase of data.verify(proof) for a batch of proofs of one circuit.
// verify_query.hpp holds the layout, the status encoding and the portable text these kernels are held to.
//
//  k_verify_canon   check 1: one flag per proof, set when any of its words is >= p
//  k_verify_paths   checks 4 and 6: one 16-lane group per (tree, proof, query) walks the Merkle path of that query in that tree -
//                   hash_or_noop of the leaf, the siblings by index bits, the comparison with the cap entry - in the lane-cooperative
//                   permutation (poseidon.hpp pos_permute_coop), round constants in LDS: a path is a chain of 20 - 40 dependent
//                   permutations, so it is latency bound like a small Merkle level
//  k_verify_fri     checks 5 and 7: one lane per (proof, query) runs vq_fri_query
//
// Both query kernels fold  ordinal << 8 | check  into the status word of their (proof, query) by atomic minimum.  Jobs of a proof
// whose challenge block is not live (it failed a check before its queries) return at once.  Every read of a proof goes through
// VqLayout (offsets and counts of the circuit, none taken from the proof) and the host's query indices, which are below N.
#include "internal.hpp"
#include "poseidon.hpp"
#include "verify_query.hpp"

namespace lcp2 {

constexpr int VERIFY_THREADS = 256;

__global__ __launch_bounds__(VERIFY_THREADS) void k_verify_canon(const u64 *__restrict__ proofs, u64 proof_words, u64 count, u32 *__restrict__ flags) {
  const u64 proof = blockIdx.y;
  if (proof >= count) return;
  const u64 *w = proofs + proof * proof_words;
  bool bad = false;
  for (u64 i = (u64)blockIdx.x * VERIFY_THREADS + threadIdx.x; i < proof_words; i += (u64)gridDim.x * VERIFY_THREADS) bad = bad || w[i] >= GL_P;
  if (bad) atomicOr(flags + proof, 1u);
}

// Groups are numbered tree-major, so the four groups of a wave walk paths of one tree (the same leaf length and sibling count) except
// where two trees meet.  The shuffles of a group read only its own lanes and all 16 lanes of a group take every branch together.
__global__ __launch_bounds__(VERIFY_THREADS) void k_verify_paths(const VqLayout V, const u64 *__restrict__ proofs, u64 count,
                                                                  const VqChallenge *__restrict__ challenges, const u64 *__restrict__ cs_cap,
                                                                  u32 *__restrict__ status, const u64 *__restrict__ rc) {
  __shared__ u64 rcs[POS_ROUNDS * POS_W];
  for (u32 i = threadIdx.x; i < POS_ROUNDS * POS_W; i += VERIFY_THREADS) rcs[i] = rc[i];
  __syncthreads();
  const u64 t = (u64)blockIdx.x * VERIFY_THREADS + threadIdx.x, group = t >> 4, per_tree = count * V.num_queries;
  const u32 j = (u32)t & 15;
  if (group >= per_tree * V.num_trees) return;  // whole groups
  const u32 tree = (u32)(group / per_tree), q = (u32)(group % V.num_queries);
  const u64 proof = (group % per_tree) / V.num_queries;
  const VqChallenge &c = challenges[proof];
  if (!c.live) return;
  const VqPath p = vq_path_of(V, c, proofs + proof * V.proof_words, cs_cap, q, tree);
  // hash_or_noop: lane i < 8 holds element i of the sponge; a block of the leaf overwrites the elements it has words for
  u64 v = 0;
  if (p.leaf_len <= 4) {
    if (j < p.leaf_len) v = gl_canon(p.leaf[j]);
  } else {
    for (u32 off = 0; off < p.leaf_len; off += 8) {
      if (j < 8 && off + j < p.leaf_len) v = gl_canon(p.leaf[off + j]);
      v = pos_permute_coop(v, j, rcs);
    }
  }
  // two_to_one(left, right): the node so far is in lanes 0..3; with the index bit set it is the right child and moves to lanes 4..7
  u64 index = p.index;
  for (u32 k = 0; k < p.nsib; k++) {
    const u64 moved = __shfl(v, (int)((j + 12) & 15), 16);
    const bool right = index & 1;
    const u64 sib = j < 8 ? p.siblings[4 * k + (j & 3)] : 0;
    v = j < 4 ? (right ? sib : v) : j < 8 ? (right ? moved : sib) : 0;
    v = pos_permute_coop(v, j, rcs);
    index >>= 1;
  }
  if (j < 4 && v != p.cap[4 * index + j]) atomicMin(status + proof * V.num_queries + q, p.status);
}

__global__ __launch_bounds__(64) void k_verify_fri(const VqLayout V, const u64 *__restrict__ proofs, u64 count,
                                                    const VqChallenge *__restrict__ challenges, u32 *__restrict__ status) {
  const u64 t = (u64)blockIdx.x * 64 + threadIdx.x;
  if (t >= count * V.num_queries) return;
  const u64 proof = t / V.num_queries;
  const u32 q = (u32)(t % V.num_queries);
  const VqChallenge &c = challenges[proof];
  if (!c.live) return;
  const u64 *w = proofs + proof * V.proof_words;
  const u32 s = vq_fri_query(V, c, w, w + V.final_poly, q);
  if (s != VQ_STATUS_NONE) atomicMin(status + t, s);
}

void launch_verify_canon(hipStream_t s, const u64 *proofs, u64 proof_words, u64 count, u32 *flags) {
  if (!count) return;
  const unsigned per_proof = (unsigned)std::min<u64>((proof_words + 4 * VERIFY_THREADS - 1) / (4 * VERIFY_THREADS), 64);
  for (u64 at = 0; at < count; at += 65535) {  // grid.y
    const u64 piece = std::min<u64>(count - at, 65535);
    hipLaunchKernelGGL(k_verify_canon, dim3(per_proof, (unsigned)piece), dim3(VERIFY_THREADS), 0, s, proofs + at * proof_words, proof_words, piece, flags + at);
  }
}
void launch_verify_paths(hipStream_t s, const VqLayout &V, const u64 *proofs, u64 count, const VqChallenge *challenges, const u64 *cs_cap, u32 *status,
                         const u64 *rc) {
  const u64 threads = count * V.num_queries * V.num_trees * 16;
  if (!threads) return;
  hipLaunchKernelGGL(k_verify_paths, dim3((unsigned)((threads + VERIFY_THREADS - 1) / VERIFY_THREADS)), dim3(VERIFY_THREADS), 0, s, V, proofs, count,
                     challenges, cs_cap, status, rc);
}
void launch_verify_fri(hipStream_t s, const VqLayout &V, const u64 *proofs, u64 count, const VqChallenge *challenges, u32 *status) {
  const u64 threads = count * V.num_queries;
  if (!threads) return;
  hipLaunchKernelGGL(k_verify_fri, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, s, V, proofs, count, challenges, status);
}

}  // namespace lcp2
