"""The 310 witness rows of one two_to_one_sha256 (lcp2_sha256_witness) over Python integers.

Written from the row layout of csrc/sha_layout.hpp and the gates of host/gates.cpp (prog_sha_sched, prog_sha_round_e, prog_sha_round_a,
prog_sha_add) as host/builder.cpp two_to_one_sha256 lays them out; it includes nothing from csrc/ and shares no text with the
kernels.  tests/test_sha_rows.py pins it to hashlib and to the gates' own constraint programs, then holds the kernels to it.

  rows [0, 48)     schedule rows for W_16 .. W_63    w2 w7 w15 w16 wt | bits of w2 at 8, of w15 at 40 | carry bits at 104, 105
  rows [48, 176)   64 x (round E row, round A row) of the data block
        E row      e f g h d w e_new t1 | bits of e, f, g at 8, 40, 72 | three carry bits of t1 at 104..106, the carry of e_new at 107
        A row      a b c t1 a_new       | bits of a, b, c at 8, 40, 72 | two carry bits at 104, 105
  rows [176, 179)  additions chain_i + state_i, three per row: (x, y, out) at 3j, the 32 bits of out and the carry at 9 + 33j
  rows [179, 307)  the rounds of the constant padding block (w = 0: its schedule word is part of the row's gate constant)
  rows [307, 310)  its additions: the outputs are the digest
Every other cell of columns 0..107 is 0; columns 108.. are not the hash's."""
M32 = 0xFFFFFFFF
ROWS, COLUMNS = 310, 108
K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
GATE_SCHEDULE, GATE_ROUND_E, GATE_ROUND_A, GATE_ADD = "ShaScheduleGate", "ShaRoundEGate", "ShaRoundAGate", "ShaAddGate"


def rotr(x, r):
    return ((x >> r) | (x << (32 - r))) & M32


def small_sigma0(x):
    return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)


def small_sigma1(x):
    return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10)


def big_sigma0(x):
    return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22)


def big_sigma1(x):
    return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25)


def schedule(words16):
    """W_0 .. W_63 and, for t >= 16, the unreduced sum W_t comes from"""
    w, sums = list(words16), [None] * 16
    for t in range(16, 64):
        sums.append(small_sigma1(w[t - 2]) + w[t - 7] + small_sigma0(w[t - 15]) + w[t - 16])
        w.append(sums[t] & M32)
    return w, sums


PAD_W = schedule([0x80000000] + [0] * 14 + [512])[0]   # the schedule of the second block of every 64-byte message


def compress(chain, w64):
    """-> (the registers (a..h) BEFORE every round and after the last one: 65 tuples, the (a, e) after every round: 64 pairs,
    the new chaining value)"""
    s, before, ae = tuple(chain), [], []
    for t in range(64):
        before.append(s)
        a, b, c, d, e, f, g, h = s
        t1 = (h + big_sigma1(e) + ((e & f) ^ (~e & g & M32)) + K[t] + w64[t]) & M32
        t2 = (big_sigma0(a) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        s = ((t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g)
        ae.append((s[0], s[4]))
    before.append(s)
    return before, ae, [(x + y) & M32 for x, y in zip(chain, s)]


def digest_words(words16):
    """the 8 words of SHA-256 of the 64-byte message: data block, then the padding block"""
    mid = compress(IV, schedule(words16)[0])[2]
    return compress(mid, PAD_W)[2]


def _bits(x):
    return [(x >> i) & 1 for i in range(32)]


def row_gates():
    """[(gate name, gate constant 0)] of the 310 rows.  The constant of a round E row is K_t in the data block and K_t + W_pad_t in the
    padding block, as a field element - NOT reduced mod 2^32 (host/builder.cpp two_to_one_sha256: kconst)."""
    out = [(GATE_SCHEDULE, 0)] * 48
    for block in range(2):
        for t in range(64):
            out += [(GATE_ROUND_E, K[t] + (PAD_W[t] if block else 0)), (GATE_ROUND_A, 0)]
        out += [(GATE_ADD, 0)] * 3
    return out


def expected_rows(words16, carries=None):
    """310 x 108 cells.  carries: a dict of sets that collects the value every carry field takes
    ("schedule", "round_e", "e_new", "round_a", "add")"""
    note = (lambda field, v: carries.setdefault(field, set()).add(v)) if carries is not None else (lambda field, v: None)
    words16 = [int(x) for x in words16]
    assert len(words16) == 16 and all(0 <= x <= M32 for x in words16)
    rows = []
    w, sums = schedule(words16)
    for t in range(16, 64):
        r = [0] * COLUMNS
        r[0:5] = [w[t - 2], w[t - 7], w[t - 15], w[t - 16], w[t]]
        r[8:40], r[40:72] = _bits(w[t - 2]), _bits(w[t - 15])
        carry = sums[t] >> 32
        note("schedule", carry)
        r[104], r[105] = carry & 1, carry >> 1
        rows.append(r)
    chain = list(IV)
    for block in range(2):
        w64 = w if block == 0 else PAD_W
        before, _, out = compress(chain, w64)
        for t in range(64):
            a, b, c, d, e, f, g, h = before[t]
            a_new, e_new = before[t + 1][0], before[t + 1][4]
            wire_w = w64[t] if block == 0 else 0
            sum1 = h + big_sigma1(e) + ((e & f) ^ (~e & g & M32)) + K[t] + w64[t]
            t1, k1 = sum1 & M32, sum1 >> 32
            sume = d + t1
            assert sume & M32 == e_new
            note("round_e", k1)
            note("e_new", sume >> 32)
            r = [0] * COLUMNS
            r[0:8] = [e, f, g, h, d, wire_w, e_new, t1]
            r[8:40], r[40:72], r[72:104] = _bits(e), _bits(f), _bits(g)
            r[104:108] = [k1 & 1, (k1 >> 1) & 1, k1 >> 2, sume >> 32]
            rows.append(r)
            suma = t1 + big_sigma0(a) + ((a & b) ^ (a & c) ^ (b & c))
            assert suma & M32 == a_new
            note("round_a", suma >> 32)
            r = [0] * COLUMNS
            r[0:5] = [a, b, c, t1, a_new]
            r[8:40], r[40:72], r[72:104] = _bits(a), _bits(b), _bits(c)
            r[104], r[105] = (suma >> 32) & 1, suma >> 33
            rows.append(r)
        state = before[64]
        for first in (0, 3, 6):
            r = [0] * COLUMNS
            for j, i in enumerate(range(first, min(first + 3, 8))):
                total = chain[i] + state[i]
                assert total & M32 == out[i]
                note("add", total >> 32)
                r[3 * j:3 * j + 3] = [chain[i], state[i], out[i]]
                r[9 + 33 * j:9 + 33 * j + 32] = _bits(out[i])
                r[9 + 33 * j + 32] = total >> 32
            rows.append(r)
        chain = out
    assert len(rows) == ROWS and all(len(r) == COLUMNS for r in rows)
    return rows


def resolve(jobs, level_start, words_in):
    """jobs: [(first_row, [16 sources])] sorted by level; level_start: nlevels + 1 indices.  Resolves the sources level by level - a
    source s >= 0 is words_in[s], s < 0 digest word (~s) & 7 of job (~s) >> 3, which must be of an earlier level - and returns
    (the 16 message words of every job, the 8 digest words of every job)"""
    messages, digests = [None] * len(jobs), [None] * len(jobs)
    assert level_start[0] == 0 and level_start[-1] == len(jobs)
    for l in range(len(level_start) - 1):
        assert level_start[l] <= level_start[l + 1]
        for j in range(level_start[l], level_start[l + 1]):
            msg = []
            for s in jobs[j][1]:
                s = int(s)
                if s >= 0:
                    msg.append(int(words_in[s]))
                else:
                    job, word = (-1 - s) // 8, (-1 - s) % 8
                    assert job < level_start[l]
                    msg.append(digests[job][word])
            messages[j] = msg
        for j in range(level_start[l], level_start[l + 1]):   # only now: no job of a level sees a digest of its own level
            digests[j] = digest_words(messages[j])
    return messages, digests


def expected_digests(jobs, level_start, words_in):
    return resolve(jobs, level_start, words_in)[1]
