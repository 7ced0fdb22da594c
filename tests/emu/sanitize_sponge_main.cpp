// TEST HARNESS (not product code): emu_sponge.cpp (the sponge of the leaf and Merkle kernels on the CPU, rows outside a tail's mask
// poisoned) under ASan + UBSan as a stand-alone program, linked against nothing else (tests/checks/sponge_sanitize.sh,
// tests/test_sponge_tails.py).
// Every digest is held to the plain sponge written here on pos_permute_portable (the full permutation, canonicalised words, one
// permutation per chunk of 8): leaves of every length class (no permutation, one, CAPACITY -> FINAL, FULL -> ragged FINAL), the
// same leaves absorbed in chunks, extension leaves, two_to_one.  Every buffer is sized exactly, so a read past a leaf's last word
// is a heap overflow.  The appended constants are held to pos_sbox of the round constants.  Prints one summary line.
#include <vector>
#include "emu_sponge.cpp"
#include "sanitize_common.hpp"

static void plain_hash(const u64 *words, u32 len, bool noop, u64 out[4]) {  // hash_or_noop (noop) / hash_no_pad
  const u64 *rc = emu_round_constants();
  u64 s[12] = {0};
  if (noop && len <= 4) {
    for (u32 c = 0; c < len; c++) s[c] = gl_canon(words[c]);
  } else {
    for (u32 c0 = 0; c0 < len; c0 += 8) {
      for (u32 j = 0; j < 8 && c0 + j < len; j++) s[j] = gl_canon(words[c0 + j]);
      pos_permute_portable(s, rc);
    }
  }
  for (int j = 0; j < 4; j++) out[j] = s[j];
}

int main() {
  const u64 *rc = emu_round_constants();
  {  // the table: the 360 derived constants first, the four zero-capacity constants last
    u64 plain[POS_ROUNDS * POS_W];
    pos_derive_round_constants(plain);
    for (int i = 0; i < POS_ROUNDS * POS_W; i++) CHECK(rc[i] == plain[i]);
    CHECK(POS_RC_ZERO_CAP + 4 == POS_RC_WORDS);
    for (int i = 0; i < 4; i++) {
      CHECK(rc[POS_RC_ZERO_CAP + i] == gl_canon(pos_sbox(plain[8 + i])));
      CHECK(rc[POS_RC_ZERO_CAP + i] == gl_pow(plain[8 + i], 7));
    }
  }
  {  // this build poisons: after a FINAL tail rows 4..11 hold the poison word, after CAPACITY rows 0..7
    u64 s[12], t[12];
    for (int i = 0; i < 12; i++) s[i] = t[i] = rnd();
    pos_permute_body(s, rc, false);
    pos_permute_body(t, rc, false);
    pos_permute_tail<POS_TAIL_FINAL>(s);
    pos_permute_tail<POS_TAIL_CAPACITY>(t);
    for (int i = 0; i < 12; i++) {
      CHECK((s[i] == POS_POISON) == (i >= 4));
      CHECK((t[i] == POS_POISON) == (i < 8));
    }
  }
  // ---- leaves: row-major [nleaves][len], column-major [len][nleaves] (what the prover hashes) and in chunks
  const u32 lens[] = {1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 135};
  const u64 nleaves = 37;
  unsigned digests_checked = 0, chunked = 0;
  for (u32 len : lens) {
    std::vector<u64> rows(nleaves * len);
    for (auto &w : rows) w = rnd();  // any u64: one word in 2^32 is not canonical ...
    for (u32 c = 0; c < len; c++) {
      rows[0 * len + c] = 0;
      rows[1 * len + c] = GL_P - 1;
      rows[2 * len + c] = c + 1 == len ? 7 : 0;  // only the last word
      rows[3 * len + c] = ~0ull;                 // ... and these all are
      rows[4 * len + c] = GL_P + c;
    }
    std::vector<u64> want(4 * nleaves), got(4 * nleaves), cols(nleaves * len);
    for (u64 i = 0; i < nleaves; i++) {
      plain_hash(&rows[i * len], len, true, &want[4 * i]);
      for (u32 c = 0; c < len; c++) cols[c * nleaves + i] = rows[i * len + c];
    }
    emu_hash_leaves(rows.data(), len, 1, len, nleaves, got.data());
    CHECK(got == want);
    std::fill(got.begin(), got.end(), 1);
    emu_hash_leaves(cols.data(), 1, nleaves, len, nleaves, got.data());
    CHECK(got == want);
    digests_checked += 2 * nleaves;
    if (len <= 4) continue;  // the chunked commitment hashes every leaf (hash_no_pad); its circuits have more than 4 wires
    for (u32 chunk : {8u, 16u, 64u}) {  // chunks of `chunk` columns, the last one what is left
      std::vector<u64> state(12 * nleaves, POS_POISON);
      std::fill(got.begin(), got.end(), 1);
      for (u32 first = 0; first < len; first += chunk) {
        const u32 n = first + chunk < len ? chunk : len - first;
        emu_hash_leaves_absorb(&cols[(u64)first * nleaves], nleaves, n, nleaves, state.data(), first == 0, first + n == len, got.data());
        if (first + n < len) for (u64 v : state) CHECK(v < GL_P);  // a kept state is whole and canonical
      }
      CHECK(got == want);
      chunked++;
    }
  }
  // ---- extension leaves: 2 * arity words, a[e] and b[e] interleaved
  for (u32 arity : {1u, 2u, 3u, 4u, 5u, 8u, 12u, 16u}) {
    std::vector<u64> a(nleaves * arity), b(nleaves * arity), flat(2 * arity), want(4 * nleaves), got(4 * nleaves);
    for (auto &w : a) w = rnd() % GL_P;
    for (auto &w : b) w = rnd() % GL_P;
    for (u64 i = 0; i < nleaves; i++) {
      for (u32 e = 0; e < arity; e++) { flat[2 * e] = a[i * arity + e]; flat[2 * e + 1] = b[i * arity + e]; }
      plain_hash(flat.data(), 2 * arity, true, &want[4 * i]);
    }
    emu_hash_ext_leaves(a.data(), b.data(), arity, nleaves, got.data());
    CHECK(got == want);
    digests_checked += nleaves;
  }
  // ---- two_to_one
  {
    std::vector<u64> children(8 * nleaves), want(4 * nleaves), got(4 * nleaves);
    for (auto &w : children) w = rnd() % GL_P;
    for (int j = 0; j < 8; j++) { children[j] = 0; children[8 + j] = GL_P - 1; }
    for (u64 i = 0; i < nleaves; i++) plain_hash(&children[8 * i], 8, false, &want[4 * i]);
    emu_merkle_level(children.data(), got.data(), nleaves);
    CHECK(got == want);
    digests_checked += nleaves;
  }
  printf("sanitize_sponge: %u digests of the poisoned sponge equal the plain sponge (leaves of %u lengths, row- and column-major, %u chunked runs, "
         "extension leaves, two_to_one); zero-capacity constants equal rc[8..11]^7\n",
         digests_checked, (unsigned)(sizeof lens / sizeof lens[0]), chunked);
  return 0;
}
