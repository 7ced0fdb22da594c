// Compressed proofs (proof_compress.hpp holds the format and the portable text):
//   lcp2_proof_compressed_words_max / lcp2_proof_compress / lcp2_proof_decompress   host only, no device work
//   lcp2_verify_batch_compressed                                                    lcp2_verify_batch_ex for compressed proofs
//
// The batch call puts one stage in front of the kernels of verify_batch.hip.  Per chunk of the batch:
//   a. k_compress_scatter: the words outside the query section of every compressed proof go where the full layout has them, in a
//      scratch proof whose query section is zeroed; a proof shorter than those words is flagged (check 1).
//   b. k_verify_canon and the head (host or device) on the scratch proofs, as in verify_batch.hip: the query indices.
//   c. k_decompress_paths: one workgroup per (proof, tree) rebuilds the tree's pruned multiproof level by level - the digests of the
//      current level in LDS, LDS-only barriers between levels, every shared node hashed once by a 16-lane group - and writes the
//      leaf and the whole sibling list of every query into the scratch proof.  A word count that is not the one the indices imply
//      is flagged (check 1) and nothing of that proof's trees is read.
//   d. k_verify_canon once more (the stored words have arrived), k_verify_paths and k_verify_fri on the scratch proofs, unchanged.
// The scratch proof of a compressed proof is what lcp2_proof_decompress gives for it, so its verdict is lcp2_verify's for that.
// A proof whose proof of work fails has no query indices: its trees are not decoded, on the host (lcp2_proof_decompress leaves the
// query section zero) as on the device, and check 2 is its verdict.
//
// Scratch slots of the context: 0 the scratch proofs, the chunk's offsets and (host proofs) its compressed words; 1 challenge
// blocks, flags, head codes, late flags, status words (+ transcript challenges and identity sums, device head); 2 the words
// outside the queries of device proofs (host head) or public inputs and circuit tables (device head); 3 the constants cap.
#include <algorithm>
#include <cstring>
#include <vector>
#include "internal.hpp"
#include "proof_compress.hpp"
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

constexpr int DECOMP_THREADS = 512, DECOMP_GROUPS = DECOMP_THREADS / 16;  // 32 groups: the 28 paths of a standard tree in one pass per level

// offsets: count + 1 word offsets into comps.  grid (pieces of a proof, proof)
__global__ __launch_bounds__(DECOMP_THREADS) void k_compress_scatter(const VqLayout V, const u64 *__restrict__ comps, const u64 *__restrict__ offsets,
                                                                      u64 *__restrict__ proofs, u32 *__restrict__ flags) {
  const u64 proof = blockIdx.y, len = offsets[proof + 1] - offsets[proof], outside = pc_outside_words(V);
  const u64 *src = comps + offsets[proof];
  u64 *dst = proofs + proof * V.proof_words;
  for (u64 i = (u64)blockIdx.x * DECOMP_THREADS + threadIdx.x; i < V.proof_words; i += (u64)gridDim.x * DECOMP_THREADS) {
    const bool query = i >= V.queries && i < V.final_poly;
    const u64 from = i < V.queries ? i : V.queries + (i - V.final_poly);
    dst[i] = !query && from < len ? src[from] : 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && len < outside) flags[proof] = 1;
}

// Workgroup barrier that orders LDS accesses only: the stores into the scratch proof stay in flight across the levels
__device__ __forceinline__ void decomp_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// pc_first_through by a 16-lane group: lane j looks at the queries j, j + 16, ..., the minimum goes round the group
__device__ __forceinline__ u32 decomp_first_through(const u32 *xs, u32 R, u32 shift, u32 level, u32 node, u32 j) {
  u32 first = PC_NONE;
  for (u32 o = j; o < R; o += 16)
    if (first == PC_NONE && ((xs[o] >> shift) >> level) == node) first = o;
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) first = min(first, (u32)__shfl_xor((int)first, d, 16));
  return first;
}

// pc_decompress_tree for tree blockIdx.x of proof blockIdx.y.  A 16-lane group is one path; it hashes as a group of k_verify_paths
// does (element i of the sponge in lane i, round constants in LDS).  Proofs that failed check 1 or the proof of work have no
// indices and are left alone.  late[proof] is set when the proof's word count is not pc_compressed_words of its indices.
__global__ __launch_bounds__(DECOMP_THREADS) void k_decompress_paths(const VqLayout V, const u64 *__restrict__ comps, const u64 *__restrict__ offsets,
                                                                      u64 *__restrict__ proofs, const VqChallenge *__restrict__ challenges,
                                                                      const u32 *__restrict__ flags, const u32 *__restrict__ codes, u32 *__restrict__ late,
                                                                      const u64 *__restrict__ rc) {
  __shared__ u64 rcs[POS_ROUNDS * POS_W];
  __shared__ u64 cur[2][VQ_MAX_QUERIES][4];
  __shared__ u32 xs[VQ_MAX_QUERIES], merged[VQ_MAX_QUERIES], stored[VQ_MAX_QUERIES], at[VQ_MAX_QUERIES];
  __shared__ u32 before[VQ_MAX_QUERIES], every[VQ_MAX_QUERIES], mine[VQ_MAX_QUERIES];
  __shared__ u32 total;
  const u32 t = blockIdx.x, tid = threadIdx.x, R = V.num_queries;
  const u64 proof = blockIdx.y;
  if (flags[proof] || codes[proof] == 1 || codes[proof] == 2) return;  // the whole workgroup
  for (u32 i = tid; i < POS_ROUNDS * POS_W; i += DECOMP_THREADS) rcs[i] = rc[i];
  if (tid < VQ_MAX_QUERIES) xs[tid] = tid < R ? challenges[proof].x_index[tid] : 0;
  __syncthreads();
  // ---- the plan of every query in this tree, and the word counts of all trees: where this tree starts and what the proof takes
  if (tid < VQ_MAX_QUERIES) {
    u32 b = 0, e = 0, m = 0;
    if (tid < R)
      for (u32 tt = 0; tt < V.num_trees; tt++) {
        const PcPlan p = pc_plan(xs, R, tid, V.tree[tt].index_shift, V.tree[tt].nsib);
        const u32 w = pc_plan_words(p, V.tree[tt].leaf_len);
        e += w;
        if (tt < t) b += w;
        if (tt == t) { m = w; merged[tid] = p.merged; stored[tid] = p.stored; }
      }
    before[tid] = b; every[tid] = e; mine[tid] = m;
  }
  __syncthreads();
  if (tid < VQ_MAX_QUERIES) {
    u32 start = (u32)pc_outside_words(V), sum = start;
    for (u32 o = 0; o < VQ_MAX_QUERIES; o++) { start += before[o] + (o < tid ? mine[o] : 0); sum += every[o]; }
    at[tid] = start;
    if (tid == 0) total = sum;
  }
  __syncthreads();
  if ((u64)total != offsets[proof + 1] - offsets[proof]) {  // the whole workgroup; nothing behind the outside words is read
    if (t == 0 && tid == 0) late[proof] = 1;
    return;
  }
  const VqTree T = V.tree[t];
  const u32 g = tid >> 4, j = tid & 15;
  const u64 *comp = comps + offsets[proof];
  u64 *full = proofs + proof * V.proof_words;
  // ---- leaves: copied for every query, hashed by the first query of each leaf (hash_or_noop as in k_verify_paths)
  for (u32 q = g; q < R; q += DECOMP_GROUPS) {
    const u32 first = decomp_first_through(xs, R, T.index_shift, 0, xs[q] >> T.index_shift, j);
    const u64 *leaf = comp + at[first];
    u64 *dst = full + pc_full_leaf(V, t, q);
    for (u32 i = j; i < T.leaf_len; i += 16) dst[i] = leaf[i];
    if (first != q) continue;
    u64 v = 0;
    if (T.leaf_len <= 4) {
      if (j < T.leaf_len) v = gl_canon(leaf[j]);
    } else {
      for (u32 off = 0; off < T.leaf_len; off += 8) {
        if (j < 8 && off + j < T.leaf_len) v = gl_canon(leaf[off + j]);
        v = pos_permute_coop(v, j, rcs);
      }
    }
    if (j < 4) cur[0][q][j] = v;
  }
  decomp_lds_barrier();
  // ---- level by level: the sibling of every path (computed one level below, or stored by the first query through the node), the
  // parent by the first query through the node
  for (u32 l = 0; l < T.nsib; l++) {
    const u32 a = l & 1;
    for (u32 q = g; q < R; q += DECOMP_GROUPS) {
      const u32 y = (xs[q] >> T.index_shift) >> l;
      const u32 first = decomp_first_through(xs, R, T.index_shift, l, y, j), other = decomp_first_through(xs, R, T.index_shift, l, y ^ 1, j);
      u64 sib = 0;
      if (j < 8) {
        PcPlan p;
        p.merged = merged[first]; p.stored = stored[first];
        sib = other != PC_NONE ? cur[a][other][j & 3] : comp[pc_level_offset(p, T.leaf_len, at[first], l) + (j & 3)];
      }
      if (j < 4) full[pc_full_leaf(V, t, q) + T.leaf_len + 4 * l + j] = sib;
      if (first != q) continue;
      const bool right = y & 1;
      const u64 node = cur[a][q][j & 3], theirs = gl_canon(sib);
      u64 v = j < 4 ? (right ? theirs : node) : j < 8 ? (right ? node : theirs) : 0;
      v = pos_permute_coop(v, j, rcs);
      if (j < 4) cur[a ^ 1][q][j] = v;
    }
    decomp_lds_barrier();
  }
}

}  // namespace lcp2
using namespace lcp2;

namespace {
inline size_t round64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

// the query indices of a proof from its words outside the query section (outside: pc_outside_words of them, as a compressed proof
// begins): 0, or 2 when the proof of work fails and there are none
int query_indices(const VerifierView &v, const ProofLayout &L, const u64 *outside, const u64 *pis, VqChallenge &c) {
  const HeadLayout H = head_make_layout(v, L, 1);
  OneLaneSponge sp;
  sp.rc = HostPoseidon::get().round_constants();
  HeadChallenges hc = {};
  return head_transcript(sp, H, outside, outside + L.queries, pis, v.digest, hc, c);
}

// decompress into `proof` (L.total words): LCP2_OK or LCP2_E_INVALID
int decompress_impl(const VerifierView &v, const ProofLayout &L, const VqLayout &V, const u64 *comp, size_t comp_words, const u64 *pis, u64 *proof) {
  const size_t outside = pc_outside_words(V);
  if (comp_words < outside) return LCP2_E_INVALID;
  VqChallenge c;
  memset(&c, 0, sizeof c);
  const int head = query_indices(v, L, comp, pis, c);
  if (head == 0 && comp_words != pc_compressed_words(V, c.x_index)) return LCP2_E_INVALID;
  memcpy(proof, comp, L.queries * 8);
  memset(proof + L.queries, 0, (L.final_poly - L.queries) * 8);
  memcpy(proof + L.final_poly, comp + L.queries, (L.total - L.final_poly) * 8);
  if (head) return LCP2_OK;  // no indices: nothing behind the outside words is read, and lcp2_verify stops at check 2
  const u64 *tree = comp + outside;
  for (u32 t = 0; t < V.num_trees; t++) {
    pc_decompress_tree(V, c.x_index, t, tree, proof, HostPoseidon::get().round_constants());
    tree += pc_tree_words(V, c.x_index, t);
  }
  return LCP2_OK;
}
}  // namespace

extern "C" size_t lcp2_proof_compressed_words_max(const lcp2_params *p) {
  bool unsupported = false;
  if (!p || params_problem(*p, &unsupported)) return 0;
  const ProofLayout L(*p);
  return pc_compressed_words_max(vq_make_layout(L, *p));
}

extern "C" int lcp2_proof_compress(const lcp2_circuit *c, const uint64_t *proof, size_t proof_words, const uint64_t *public_inputs, size_t num_public_inputs,
                                   uint64_t *out, size_t out_cap, size_t *out_words) {
  if (!c || !proof || !out_words) return LCP2_E_INVALID;
  const VerifierView v = verifier_view(c);
  const ProofLayout L(*v.p);
  if (proof_words != L.total || num_public_inputs != v.npi || (v.npi && !public_inputs)) return LCP2_E_INVALID;
  const VqLayout V = vq_make_layout(L, *v.p);
  const size_t outside = pc_outside_words(V);
  std::vector<u64> comp(L.total), back(L.total);
  memcpy(comp.data(), proof, L.queries * 8);
  memcpy(comp.data() + L.queries, (const u64 *)proof + L.final_poly, (L.total - L.final_poly) * 8);
  VqChallenge ch;
  memset(&ch, 0, sizeof ch);
  if (query_indices(v, L, comp.data(), (const u64 *)public_inputs, ch)) return LCP2_E_VERIFY;  // no indices: nothing says what to drop
  size_t words = outside;
  for (u32 t = 0; t < V.num_trees; t++) words += pc_compress_tree(V, ch.x_index, t, (const u64 *)proof, comp.data() + words);
  // what was dropped must come back: a duplicate that differs from its first occurrence, or a sibling that is not the digest of the
  // other paths, would be lost
  if (decompress_impl(v, L, V, comp.data(), words, (const u64 *)public_inputs, back.data()) != LCP2_OK || memcmp(back.data(), proof, L.total * 8))
    return LCP2_E_VERIFY;
  *out_words = words;
  if (!out || out_cap < words) return LCP2_E_INVALID;
  memcpy(out, comp.data(), words * 8);
  return LCP2_OK;
}

extern "C" int lcp2_proof_decompress(const lcp2_circuit *c, const uint64_t *comp, size_t comp_words, const uint64_t *public_inputs, size_t num_public_inputs,
                                     uint64_t *proof, size_t proof_words) {
  if (!c || !comp || !proof) return LCP2_E_INVALID;
  const VerifierView v = verifier_view(c);
  const ProofLayout L(*v.p);
  if (proof_words != L.total || num_public_inputs != v.npi || (v.npi && !public_inputs)) return LCP2_E_INVALID;
  const VqLayout V = vq_make_layout(L, *v.p);
  std::vector<u64> full(L.total);  // a refused call leaves `proof` untouched
  LCP2_TRY(decompress_impl(v, L, V, (const u64 *)comp, comp_words, (const u64 *)public_inputs, full.data()));
  memcpy(proof, full.data(), L.total * 8);
  return LCP2_OK;
}

extern "C" int lcp2_verify_batch_compressed(lcp2_ctx *ctx, const lcp2_circuit *c, const uint64_t *comps, const uint64_t *offsets, size_t count, lcp2_mem comps_mem,
                                            const uint64_t *public_inputs, size_t num_public_inputs, int32_t *failed_checks, uint32_t flags) {
  if (!ctx || !c) return LCP2_E_INVALID;
  if (flags != LCP2_VERIFY_HEAD_HOST && flags != LCP2_VERIFY_HEAD_DEVICE) return ctx->fail(LCP2_E_INVALID, "verify batch: unknown flags");
  const VerifierView v = verifier_view(c);
  const lcp2_params &p = *v.p;
  const ProofLayout L(p);
  if (num_public_inputs != v.npi) return ctx->fail(LCP2_E_INVALID, "verify batch: not this circuit's public-input length");
  if (count == 0) return LCP2_OK;
  if (!comps || ((size_t)comps & 7) || !offsets || !failed_checks || (v.npi && !public_inputs) || (comps_mem != LCP2_MEM_HOST && comps_mem != LCP2_MEM_DEVICE))
    return ctx->fail(LCP2_E_INVALID, "verify batch: null or misaligned argument");
  if (count > ((size_t)1 << 40) / L.total || L.total >= ((size_t)1 << 31)) return ctx->fail(LCP2_E_INVALID, "verify batch: count too large");
  for (size_t i = 0; i < count; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] > ((u64)1 << 56)) return ctx->fail(LCP2_E_INVALID, "verify batch: offsets do not ascend");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  const VqLayout V = vq_make_layout(L, p);
  const u32 Q = p.num_query_rounds;
  const size_t head_words = L.queries, tail_words = L.total - L.final_poly, outside = head_words + tail_words, proof_words = L.total;
  const bool on_device = comps_mem == LCP2_MEM_DEVICE, dev_head = flags == LCP2_VERIFY_HEAD_DEVICE;
  const size_t pis_bytes = (size_t)v.npi * 8;
  const HeadLayout H = head_make_layout(v, L, std::max(v.num_regs, 1u));
  if (dev_head && verify_identity_lds_bytes(H.num_regs) > 65536) return ctx->fail(LCP2_E_INVALID, "verify batch: more registers than the device head holds");

  // staging, per proof.  Host head: [outside words (device proofs)] [flag] [head code] [late flag] [challenge block] [status words].
  // Device head: [public inputs] [flag] [head code] [late flag] [status words].
  const size_t per_proof = dev_head ? pis_bytes + 12 + (size_t)Q * 4 : (on_device ? outside * 8 : 0) + 12 + sizeof(VqChallenge) + (size_t)Q * 4, slack = 5 * 64;
  size_t chunk = std::min<size_t>(count, 4096);
  chunk = std::min(chunk, std::max<size_t>(1, LCP2_COMPRESSED_SCRATCH_BYTES / (proof_words * 8)));  // the scratch proofs of a chunk
  char *stage = (char *)ctx->pin;
  std::vector<char> pageable;
  if (stage && per_proof + slack <= lcp2_ctx::PIN_BYTES) {
    chunk = std::min(chunk, (lcp2_ctx::PIN_BYTES - slack) / per_proof);
  } else {
    chunk = std::min<size_t>(chunk, 64);
    pageable.resize(chunk * per_proof + slack);
    stage = pageable.data();
  }
  size_t span_max = 0;  // the most compressed words a chunk holds
  for (size_t at = 0; at < count; at += chunk) span_max = std::max<size_t>(span_max, offsets[std::min(count, at + chunk)] - offsets[at]);
  // device, slot 1: [challenge blocks] then what comes down in one piece: [flags][head codes][late flags][status]
  const size_t d_off_flags = round64(chunk * sizeof(VqChallenge)), d_off_codes = d_off_flags + round64(chunk * 4), d_off_late = d_off_codes + round64(chunk * 4),
               d_off_status = d_off_late + round64(chunk * 4), d_off_hcs = d_off_status + round64(chunk * (size_t)Q * 4),
               d_off_parts = d_off_hcs + round64(dev_head ? chunk * sizeof(HeadChallenges) : 0),
               d_work_bytes = d_off_parts + (dev_head ? chunk * (size_t)(v.num_gates + 1) * HEAD_MAX_CHALLENGES * sizeof(gl2) : 0);
  const size_t down_bytes = d_off_hcs - d_off_flags;
  // host staging: [outside words | public inputs] [the mirror of flags .. status] [challenge blocks (host head)]
  const size_t off_flags = round64(dev_head ? chunk * pis_bytes : on_device ? chunk * outside * 8 : 0), off_chal = off_flags + round64(down_bytes);
  u64 *h_outside = (u64 *)stage, *h_pis = (u64 *)stage;
  u32 *h_flags = (u32 *)(stage + off_flags), *h_codes = (u32 *)(stage + off_flags + (d_off_codes - d_off_flags)),
      *h_late = (u32 *)(stage + off_flags + (d_off_late - d_off_flags)), *h_status = (u32 *)(stage + off_flags + (d_off_status - d_off_flags));
  VqChallenge *h_chal = (VqChallenge *)(stage + off_chal);

  // device, slot 0: [scratch proofs][offsets of the chunk][compressed words of the chunk (host proofs)]
  const size_t s_off_offsets = round64(chunk * proof_words * 8), s_off_comp = s_off_offsets + round64((chunk + 1) * 8),
               s_bytes = s_off_comp + (on_device ? 0 : span_max * 8);
  char *d_work = nullptr, *d_circ = nullptr, *d_slot0 = nullptr;
  u64 *d_cap = nullptr, *d_outside = nullptr;
  LCP2_TRY(scratch_ensure(ctx, 0, s_bytes, (void **)&d_slot0));
  LCP2_TRY(scratch_ensure(ctx, 1, d_work_bytes, (void **)&d_work));
  LCP2_TRY(scratch_ensure(ctx, 3, L.capw * 8, (void **)&d_cap));
  const size_t c_off_gates = round64(chunk * pis_bytes), c_off_code = c_off_gates + round64(v.num_gates * sizeof(lcp2_gate)),
               c_off_imm = c_off_code + round64(v.code_words * 4), c_off_kis = c_off_imm + round64(v.num_imm * 8),
               c_off_digest = c_off_kis + round64((size_t)p.num_routed_wires * 8), c_bytes = c_off_digest + 64;
  if (dev_head) LCP2_TRY(scratch_ensure(ctx, 2, c_bytes, (void **)&d_circ));
  else if (on_device) LCP2_TRY(scratch_ensure(ctx, 2, chunk * outside * 8, (void **)&d_outside));
  u64 *d_proofs = (u64 *)d_slot0, *d_offsets = (u64 *)(d_slot0 + s_off_offsets), *d_comp_up = (u64 *)(d_slot0 + s_off_comp);
  VqChallenge *d_chal = (VqChallenge *)d_work;
  u32 *d_flags = (u32 *)(d_work + d_off_flags), *d_codes = (u32 *)(d_work + d_off_codes), *d_late = (u32 *)(d_work + d_off_late),
      *d_status = (u32 *)(d_work + d_off_status);
  LCP2_HIP(ctx, hipMemcpyAsync(d_cap, v.cs_cap, L.capw * 8, hipMemcpyHostToDevice, ctx->stream));
  if (dev_head) {
    LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_gates, v.gates, v.num_gates * sizeof(lcp2_gate), hipMemcpyHostToDevice, ctx->stream));
    if (v.code_words) LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_code, v.code, v.code_words * 4, hipMemcpyHostToDevice, ctx->stream));
    if (v.num_imm) LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_imm, v.imm, v.num_imm * 8, hipMemcpyHostToDevice, ctx->stream));
    LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_kis, v.k_is, (size_t)p.num_routed_wires * 8, hipMemcpyHostToDevice, ctx->stream));
    LCP2_HIP(ctx, hipMemcpyAsync(d_circ + c_off_digest, v.digest, 32, hipMemcpyHostToDevice, ctx->stream));
  }
  const unsigned pieces = (unsigned)std::min<u64>((proof_words + 4 * DECOMP_THREADS - 1) / (4 * DECOMP_THREADS), 64);
  std::vector<u64> rel(chunk + 1);

  bool all_accepted = true;
  for (size_t at = 0; at < count; at += chunk) {
    const size_t B = std::min(chunk, count - at);
    const u64 base = offsets[at], span = offsets[at + B] - base;
    for (size_t i = 0; i <= B; i++) rel[i] = offsets[at + i] - base;
    // (the synchronisation that ended the chunk before has released `rel`)
    LCP2_HIP(ctx, hipMemcpyAsync(d_offsets, rel.data(), (B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    const u64 *d_comps = (const u64 *)comps + base;
    if (!on_device) {
      if (span) LCP2_HIP(ctx, hipMemcpyAsync(d_comp_up, (const u64 *)comps + base, span * 8, hipMemcpyHostToDevice, ctx->stream));
      d_comps = d_comp_up;
    }
    LCP2_HIP(ctx, hipMemsetAsync(d_flags, 0, d_off_status - d_off_flags, ctx->stream));          // flags, head codes, late flags
    LCP2_HIP(ctx, hipMemsetAsync(d_status, 0xFF, B * (size_t)Q * 4, ctx->stream));               // VQ_STATUS_NONE
    auto queries = [&]() {  // stages c and d
      hipLaunchKernelGGL(k_decompress_paths, dim3(V.num_trees, (unsigned)B), dim3(DECOMP_THREADS), 0, ctx->stream, V, d_comps, (const u64 *)d_offsets, d_proofs,
                         (const VqChallenge *)d_chal, (const u32 *)d_flags, (const u32 *)d_codes, d_late, (const u64 *)ctx->d_rc);
      launch_verify_canon(ctx->stream, d_proofs, proof_words, B, d_late);
      launch_verify_paths(ctx->stream, V, d_proofs, B, d_chal, d_cap, d_status, ctx->d_rc);
      launch_verify_fri(ctx->stream, V, d_proofs, B, d_chal, d_status);
    };
    if (dev_head) {
      if (pis_bytes) {
        memcpy(h_pis, (const u64 *)public_inputs + at * v.npi, B * pis_bytes);
        LCP2_HIP(ctx, hipMemcpyAsync(d_circ, h_pis, B * pis_bytes, hipMemcpyHostToDevice, ctx->stream));
      }
      {
        ProfScope ps(ctx, LCP2_K_OTHER, (double)span * 8 + (double)B * proof_words * 8);
        hipLaunchKernelGGL(k_compress_scatter, dim3(pieces, (unsigned)B), dim3(DECOMP_THREADS), 0, ctx->stream, V, d_comps, (const u64 *)d_offsets, d_proofs, d_flags);
        launch_verify_canon(ctx->stream, d_proofs, proof_words, B, d_flags);
        launch_verify_head(ctx->stream, H, d_proofs, proof_words, B, (const u64 *)d_circ, (const u64 *)(d_circ + c_off_digest),
                           (const lcp2_gate *)(d_circ + c_off_gates), (const uint32_t *)(d_circ + c_off_code), (const u64 *)(d_circ + c_off_imm),
                           (const u64 *)(d_circ + c_off_kis), d_flags, d_codes, (HeadChallenges *)(d_work + d_off_hcs), (gl2 *)(d_work + d_off_parts), d_chal,
                           ctx->d_rc);
        queries();
      }
      LCP2_HIP(ctx, hipGetLastError());
      LCP2_HIP(ctx, hipMemcpyAsync(h_flags, d_flags, down_bytes, hipMemcpyDeviceToHost, ctx->stream));
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
      for (size_t i = 0; i < B; i++) {
        const u32 check = h_flags[i] || h_late[i] ? 1 : h_codes[i] ? h_codes[i] : vq_reduce_statuses(h_status + i * Q, Q);
        failed_checks[at + i] = (int32_t)check;
        if (check) all_accepted = false;
      }
      continue;
    }
    // ---- host head: the scratch proofs, check 1 on their outside words, and those words of device proofs
    {
      ProfScope ps(ctx, LCP2_K_OTHER, (double)span * 8 + (double)B * proof_words * 8);
      hipLaunchKernelGGL(k_compress_scatter, dim3(pieces, (unsigned)B), dim3(DECOMP_THREADS), 0, ctx->stream, V, d_comps, (const u64 *)d_offsets, d_proofs, d_flags);
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
    size_t decoded = 0;
    for (size_t i = 0; i < B; i++) {
      VqChallenge &ch = h_chal[i];
      memset(&ch, 0, sizeof ch);
      int rc = 1;
      if (!h_flags[i]) {  // (a flagged proof may be shorter than its outside words)
        const u64 *head = on_device ? h_outside + i * outside : (const u64 *)comps + offsets[at + i];
        rc = verify_head(v, L, head, head + head_words, (const u64 *)public_inputs + (at + i) * v.npi, ch);
        if (rc) { ch.live = 0; ch.pad = 0; }  // (check 3 leaves the indices: the trees are decoded, and check 1 still looks at them)
        if (rc != 2) decoded++;
      }
      h_codes[i] = (u32)rc;
    }
    if (decoded) {
      LCP2_HIP(ctx, hipMemcpyAsync(d_chal, h_chal, B * sizeof(VqChallenge), hipMemcpyHostToDevice, ctx->stream));
      LCP2_HIP(ctx, hipMemcpyAsync(d_codes, h_codes, B * 4, hipMemcpyHostToDevice, ctx->stream));
      {
        ProfScope ps(ctx, LCP2_K_OTHER, (double)decoded * Q * L.query_words * 8);
        queries();
      }
      LCP2_HIP(ctx, hipGetLastError());
      LCP2_HIP(ctx, hipMemcpyAsync(h_late, d_late, d_off_hcs - d_off_late, hipMemcpyDeviceToHost, ctx->stream));
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (size_t i = 0; i < B; i++) {
      const u32 rc = h_codes[i];
      const u32 check = rc == 1 || (decoded && h_late[i]) ? 1 : rc ? rc : vq_reduce_statuses(h_status + i * Q, Q);
      failed_checks[at + i] = (int32_t)check;
      if (check) all_accepted = false;
    }
  }
  return all_accepted ? LCP2_OK : LCP2_E_VERIFY;
}
