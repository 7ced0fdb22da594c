// TEST HARNESS (not product code): the sponge of the leaf and Merkle kernels (csrc/poseidon.hpp pos_sponge_absorb, pos_permute_body,
// pos_permute_tail) compiled for the CPU, each kernel of csrc/kernels_hash.hip as a loop over its lanes.  In this build a tail sets
// the rows outside its mask to POS_POISON, so a sponge that read a row its tail left out gives a wrong digest here.
// Built by tests/test_sponge_tails.py with g++; never loaded by the package.
#include "emu_rc.hpp"

using namespace lcp2;

extern "C" {

const unsigned long long *emu_sponge_round_constants() { return emu_round_constants(); }
unsigned emu_sponge_rc_words() { return POS_RC_WORDS; }
unsigned emu_sponge_rc_zero_cap() { return POS_RC_ZERO_CAP; }

// k_hash_leaves
void emu_hash_leaves(const unsigned long long *data, unsigned long long leaf_stride, unsigned long long col_stride, unsigned leaf_len,
                     unsigned long long nleaves, unsigned long long *digests) {
  const u64 *rc = emu_round_constants();
  for (u64 i = 0; i < nleaves; i++) {
    const u64 *row = data + i * leaf_stride;
    u64 s[12] = {0};
    if (leaf_len <= 4) {
      for (u32 c = 0; c < leaf_len; c++) s[c] = gl_canon(row[c * col_stride]);
    } else {
      pos_sponge_absorb(s, leaf_len, rc, true, true, [&](u32 c0, int j) { return row[(u64)(c0 + j) * col_stride]; });
    }
    for (int j = 0; j < 4; j++) digests[4 * i + j] = s[j];
  }
}

// k_hash_leaves_absorb: one chunk of the columns, the state [12][nleaves] kept between calls
void emu_hash_leaves_absorb(const unsigned long long *data, unsigned long long col_stride, unsigned ncols, unsigned long long nleaves,
                            unsigned long long *state, unsigned first, unsigned last, unsigned long long *digests) {
  const u64 *rc = emu_round_constants();
  for (u64 i = 0; i < nleaves; i++) {
    const u64 *row = data + i;
    u64 s[12];
    for (int j = 0; j < 12; j++) s[j] = first ? 0 : state[(u64)j * nleaves + i];
    pos_sponge_absorb(s, ncols, rc, first != 0, last != 0, [&](u32 c0, int j) { return row[(u64)(c0 + j) * col_stride]; });
    if (last) for (int j = 0; j < 4; j++) digests[4 * i + j] = s[j];
    else for (int j = 0; j < 12; j++) state[(u64)j * nleaves + i] = s[j];
  }
}

// k_hash_ext_leaves
void emu_hash_ext_leaves(const unsigned long long *p0, const unsigned long long *p1, unsigned arity, unsigned long long nleaves,
                         unsigned long long *digests) {
  const u64 *rc = emu_round_constants();
  for (u64 i = 0; i < nleaves; i++) {
    const u64 *a = p0 + i * arity, *b = p1 + i * arity;
    u64 s[12] = {0};
    const u32 len = 2 * arity;
    if (len <= 4) {
      for (u32 e = 0; e < arity; e++) { s[2 * e] = a[e]; s[2 * e + 1] = b[e]; }
    } else {
      pos_sponge_absorb(s, len, rc, true, true, [&](u32 c0, int j) { return (j & 1) ? b[(c0 >> 1) + (j >> 1)] : a[(c0 >> 1) + (j >> 1)]; });
    }
    for (int j = 0; j < 4; j++) digests[4 * i + j] = s[j];
  }
}

// k_merkle_level
void emu_merkle_level(const unsigned long long *children, unsigned long long *parents, unsigned long long nparents) {
  const u64 *rc = emu_round_constants();
  for (u64 i = 0; i < nparents; i++) {
    u64 s[12] = {0};
    for (int j = 0; j < 8; j++) s[j] = children[8 * i + j];
    pos_permute_body(s, rc, true);
    pos_permute_tail<POS_TAIL_FINAL>(s);
    for (int j = 0; j < 4; j++) parents[4 * i + j] = s[j];
  }
}

}  // extern "C"
