// TEST HARNESS (not product code): emu_sha.cpp (csrc/sha_rows.hpp on the CPU) under ASan + UBSan as a stand-alone program, linked
// against nothing else (tests/checks/emu_sanitize.sh).
// Random jobs in three levels (sources: words_in, digests one and two levels back) into a matrix of exactly [108][n] with a job
// flush against its end, so one store too far is a heap overflow; every list is sized exactly, so a read behind a refused index is
// one too.  The digests are held to a plain SHA-256 written here, the owned cells must all be written and no other, and the
// validation cases of the entry point are refused with nothing written.  Prints one summary line.
#include <cstring>
#include <vector>
#include "emu_sha.cpp"
#include "sanitize_common.hpp"

// SHA-256 of a 64-byte message given as 16 big-endian words, the textbook way (FIPS 180-4 section 6.2), constants recomputed from
// the primes so that nothing is shared with the tables of sha_rows.hpp
static uint32_t frac_root(unsigned prime, int root) {  // the first 32 fractional bits of prime^(1/root), by bisection on integers
  unsigned __int128 lo = 0, hi = (unsigned __int128)1 << 40;  // x / 2^32 with x^root <= prime * 2^(32 root)
  while (hi - lo > 1) {
    const unsigned __int128 mid = (lo + hi) / 2;
    // compare mid^root with prime << (32 * root) without overflow: root is 2 or 3 and mid < 2^36
    bool le;
    if (root == 2) le = mid * mid <= ((unsigned __int128)prime << 64);
    else {
      const unsigned __int128 sq = mid * mid;                       // < 2^72
      const unsigned __int128 want = (unsigned __int128)prime << 96;  // prime < 2^9: < 2^105
      le = sq <= want / mid;                                        // floor comparison is exact enough: mid^3 <= want <=> sq <= want / mid
    }
    if (le) lo = mid; else hi = mid;
  }
  return (uint32_t)lo;
}
static void plain_sha256(const uint32_t msg[16], uint32_t out[8]) {
  static uint32_t k[64], iv[8];
  if (!k[0]) {
    unsigned found = 0;
    for (unsigned p = 2; found < 64; p++) {
      bool prime = true;
      for (unsigned d = 2; d * d <= p; d++) if (p % d == 0) prime = false;
      if (!prime) continue;
      if (found < 8) iv[found] = frac_root(p, 2);
      k[found++] = frac_root(p, 3);
    }
  }
  auto rr = [](uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
  uint32_t h[8];
  memcpy(h, iv, sizeof h);
  for (int block = 0; block < 2; block++) {
    uint32_t w[64] = {0};
    if (block == 0) memcpy(w, msg, 64);
    else { w[0] = 0x80000000u; w[15] = 512; }
    for (int t = 16; t < 64; t++)
      w[t] = w[t - 16] + (rr(w[t - 15], 7) ^ rr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 7] + (rr(w[t - 2], 17) ^ rr(w[t - 2], 19) ^ (w[t - 2] >> 10));
    uint32_t s[8];
    memcpy(s, h, sizeof s);
    for (int t = 0; t < 64; t++) {
      const uint32_t t1 = s[7] + (rr(s[4], 6) ^ rr(s[4], 11) ^ rr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + k[t] + w[t];
      const uint32_t t2 = (rr(s[0], 2) ^ rr(s[0], 13) ^ rr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
      for (int i = 7; i > 0; i--) s[i] = s[i - 1];
      s[4] += t1; s[0] = t1 + t2;
    }
    for (int i = 0; i < 8; i++) h[i] += s[i];
  }
  memcpy(out, h, sizeof h);
}

int main() {
  const u64 TAG = 0xA5A5A5A5A5A5A5A5ull;
  { // the plain SHA-256 itself: the digest of 64 zero bytes is f5a5fd42 ... 2759fb4b (the zero hash of a depth-1 Merkle tree of 32-byte leaves)
    uint32_t zero[16] = {0}, d[8];
    plain_sha256(zero, d);
    CHECK(d[0] == 0xf5a5fd42u && d[7] == 0x2759fb4bu);
  }
  // ---- random jobs in three levels
  const unsigned L0 = 70, L1 = 67, L2 = 3, njobs = L0 + L1 + L2, nwords = 16 * L0 + 5;
  const u64 n = 310ull * njobs + 9;
  std::vector<unsigned> levels = {0, L0, L0 + L1, njobs};
  std::vector<unsigned> words(nwords);
  for (auto &w : words) w = (unsigned)rnd();
  std::vector<ShaJobDev> jobs(njobs);
  std::vector<u64> firsts(njobs);
  for (unsigned j = 0; j < njobs; j++) firsts[j] = 310ull * j + (j * 9) / (njobs - 1);  // gaps, the last block ends on row n
  CHECK(firsts[njobs - 1] + 310 == n);
  for (unsigned j = 0; j < njobs; j++) {
    jobs[j].first_row = (uint32_t)firsts[(j * 37 + 11) % njobs];  // 37 is coprime to 140: a permutation, not the row order
    for (int i = 0; i < 16; i++) {
      const unsigned level = j < L0 ? 0 : j < L0 + L1 ? 1 : 2;
      const unsigned before = levels[level];  // jobs of earlier levels
      if (level == 0 || rnd() % 4 == 0) jobs[j].in_src[i] = (int32_t)(rnd() % nwords);
      else jobs[j].in_src[i] = ~(int32_t)((rnd() % before) * 8 + rnd() % 8);
    }
  }
  jobs[njobs - 1].in_src[0] = ~(int32_t)(0 * 8 + 7);           // two levels back
  jobs[njobs - 1].in_src[1] = ~(int32_t)((L0 + L1 - 1) * 8);   // the last job of the level before
  jobs[njobs - 1].in_src[2] = (int32_t)(nwords - 1);
  std::vector<u64> wires(SHA_ROW_COLUMNS * n, TAG);  // exactly [108][n]
  std::vector<unsigned> digests(8 * njobs, 0);
  CHECK(emu_sha256_witness(jobs.data(), njobs, levels.data(), 3, words.data(), nwords, (unsigned long long *)wires.data(), n, digests.data()) == 0);
  for (unsigned j = 0; j < njobs; j++) {
    uint32_t msg[16], want[8];
    for (int i = 0; i < 16; i++) {
      const int32_t s = jobs[j].in_src[i];
      msg[i] = s >= 0 ? words[s] : digests[(size_t)((~s) >> 3) * 8 + ((~s) & 7)];
    }
    plain_sha256(msg, want);
    CHECK(memcmp(want, &digests[8 * j], 32) == 0);
    // the matrix shows the message in its first schedule row (W_0 is w16 of the row of W_16) and the digest in its last rows
    CHECK(wires[3 * n + jobs[j].first_row] == msg[0]);
    for (int i = 0; i < 8; i++) CHECK(wires[(3 * (i % 3) + 2) * n + jobs[j].first_row + 307 + i / 3] == want[i]);
  }
  std::vector<char> owned(n, 0);
  for (unsigned j = 0; j < njobs; j++) for (unsigned r = 0; r < SHA_ROWS; r++) owned[jobs[j].first_row + r]++;
  u64 written = 0;
  for (u64 c = 0; c < SHA_ROW_COLUMNS; c++)
    for (u64 r = 0; r < n; r++) {
      CHECK(owned[r] <= 1);
      CHECK((wires[c * n + r] != TAG) == (owned[r] == 1));  // every cell of an owned row is written (no value of a row is the tag), no other
      written += owned[r];
    }
  // without digests: the same matrix
  std::vector<u64> again(SHA_ROW_COLUMNS * n, TAG);
  CHECK(emu_sha256_witness(jobs.data(), njobs, levels.data(), 3, words.data(), nwords, (unsigned long long *)again.data(), n, nullptr) == 0);
  CHECK(again == wires);
  // ---- refusals: nothing is written, nothing behind a list is read
  unsigned refused = 0;
  auto refuse = [&](const std::vector<ShaJobDev> &js, const std::vector<unsigned> &lv, u64 nw, u64 rows, unsigned problem) {
    std::vector<u64> m(SHA_ROW_COLUMNS * rows, TAG);
    std::vector<unsigned> w(nw, 7);
    const unsigned got = emu_sha256_witness(js.data(), js.size(), lv.data(), (unsigned)lv.size() - 1, w.data(), nw, (unsigned long long *)m.data(), rows, nullptr);
    for (u64 v : m) if (v != TAG) return false;
    refused++;
    return got == problem;
  };
  std::vector<ShaJobDev> four(4);
  for (unsigned j = 0; j < 4; j++) { four[j].first_row = 310 * j; for (int i = 0; i < 16; i++) four[j].in_src[i] = j < 2 ? i : ~(int32_t)(8 * (j - 2) + i % 8); }
  const u64 n4 = 1240;
  CHECK(emu_sha256_witness(four.data(), 4, std::vector<unsigned>{0, 2, 4}.data(), 2, words.data(), 16, (unsigned long long *)std::vector<u64>(SHA_ROW_COLUMNS * n4).data(), n4, nullptr) == 0);
  CHECK(refuse(four, {1, 2, 4}, 16, n4, SHA_LEVELS_DO_NOT_COVER));
  CHECK(refuse(four, {0, 2, 3}, 16, n4, SHA_LEVELS_DO_NOT_COVER));
  CHECK(refuse(four, {0, 2, 1, 4}, 16, n4, SHA_LEVELS_NOT_MONOTONE));
  CHECK(refuse(four, {0, 100, 2, 4}, 16, n4, SHA_LEVELS_NOT_MONOTONE));  // jobs 4..99 do not exist
  CHECK(refuse(four, {0, 2, 4}, 16, n4 - 1, SHA_ROWS_OUT_OF_RANGE));      // first_row + 310 == n + 1
  CHECK(refuse(four, {0, 2, 4}, 15, n4, SHA_BAD_SOURCE));                 // in_src == nwords
  CHECK(refuse(four, {0, 1, 4}, 16, n4, SHA_BAD_SOURCE));                 // job 3 reads job 1, now of its own level
  CHECK(refuse(four, {0, 0, 4}, 16, n4, SHA_BAD_SOURCE));                 // an empty first level: every digest source is of a later level
  CHECK(refuse(four, {0}, 16, n4, SHA_NO_LEVELS));
  { auto big = four; big[3].first_row = 0xFFFFFFFFu; CHECK(refuse(big, {0, 2, 4}, 16, n4, SHA_ROWS_OUT_OF_RANGE)); }
  { auto neg = four; neg[3].in_src[5] = INT32_MIN; CHECK(refuse(neg, {0, 2, 4}, 16, n4, SHA_BAD_SOURCE)); }
  CHECK(emu_sha256_witness(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == 0);
  // ---- scatter: 257 cells into exactly [4][64], the last cell of the matrix among them; row == n refused
  std::vector<CellDev> cells(257);
  for (unsigned i = 0; i < 257; i++) cells[i] = {i % 64, (i / 64) % 4, rnd()};
  cells[256] = {63, 3, ~0ull};
  std::vector<u64> small(4 * 64, TAG);
  CHECK(emu_scatter_cells(cells.data(), cells.size(), (unsigned long long *)small.data(), 64) == 0);
  CHECK(small[3 * 64 + 63] == ~0ull && small[1 * 64 + 5] == cells[64 + 5].value);
  cells[200].row = 64;
  std::fill(small.begin(), small.end(), TAG);
  CHECK(emu_scatter_cells(cells.data(), cells.size(), (unsigned long long *)small.data(), 64) == 1);
  for (u64 v : small) CHECK(v == TAG);
  CHECK(emu_scatter_cells(nullptr, 0, (unsigned long long *)small.data(), 64) == 0);
  printf("sanitize_sha: %u jobs in 3 levels, %llu cells written and checked in a [108][%llu] matrix, digests equal a plain SHA-256, %u refusals wrote nothing, scatter ok\n",
         njobs, written, n, refused);
  return 0;
}
