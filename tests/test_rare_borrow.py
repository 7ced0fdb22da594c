"""The rare borrow of the device multiply, taken off the Poseidon hot path (csrc/poseidon.hpp pos_sbox_h, csrc/gl64.hpp
gl_mul_halves_spec): the S-box multiplies without the borrow correction of lo - (hi >> 32), ORs the four borrow masks of the wave and
recomputes the S-box exactly when any lane borrowed.  Random operands borrow once in 2^32, so nothing but planted operands ever runs
the cold path, and since it is skipped per WAVE the cases are about which lanes of a wave take it.

* field_op_batch: `mul` (the exact multiply, unchanged: the control) and `pow7` (pos_sbox_h) with borrowing operands in chosen lanes;
* poseidon_permute_batch: states whose first-round S-box input is m * 2^32, whose square has a zero low word;
* merkle_cap: the same words planted in the leaves, through k_hash_leaves and its tails, the lane-cooperative Merkle kernel
  (2^7 leaves) and k_merkle_level (2^14 leaves: levels above 4096 nodes).

Every planted operand is checked in Python integers to borrow where it is meant to; no case is skipped.

The PoseidonGate evaluator of the quotient (k_q_gate) is NOT steered into the cold path here: its S-box inputs are values of the
low-degree extension, which no small circuit can set.  It uses the same pos_sbox_h text as the kernels above and is covered by the
quotient parity tests (tests/test_gpu_prover.py) on the hot path."""
import numpy as np
import pytest

from oracle_lib import P, merkle_cap, rand_field, vp

pytestmark = pytest.mark.gpu
M = 1 << 64
EPS = 0xFFFFFFFF
WAVE = 64
BLOCK_WAVES = 4  # HASH_THREADS = 256
LANES = 64 * WAVE  # 64 waves, 16 blocks


def _borrows(a, b):
    """does the reduction of a * b borrow in lo - (hi >> 32) ?"""
    prod = a * b
    return prod % M < (prod >> 64) >> 32


def _mul_lazy(a, b):
    """the u64 the device multiply returns (gl_reduce128_nc on the 128-bit product), and whether it borrowed"""
    prod = a * b
    lo, hi = prod % M, prod >> 64
    hh, hl = hi >> 32, hi & EPS
    t = (lo - hh) % M
    if lo < hh:
        t = (t - EPS) % M
    r = t + hl * EPS
    if r >= M:
        r = (r + EPS) % M
    return r, lo < hh


def _pow7_borrows(x):
    """which of the four products of x^7 (x^2, x^4, x^3, x^7, in the order pos_sbox_h computes them) borrow"""
    x2, f0 = _mul_lazy(x, x)
    x4, f1 = _mul_lazy(x2, x2)
    x3, f2 = _mul_lazy(x, x2)
    x7, f3 = _mul_lazy(x3, x4)
    assert x7 % P == pow(x, 7, P)
    return (f0, f1, f2, f3)


def _mul_pairs(rng, n, borrow):
    """operand pairs that do / do not borrow, by the method of test_gpu_primitives._field_mul_operands: b is solved for from a
    chosen low word of the product"""
    a, b = [], []
    while len(a) < n:
        x = int(rng.integers(0, M, dtype=np.uint64)) | 1
        if borrow:
            lo = int(rng.integers(0, 1 << int(rng.integers(1, 31))))
            y = lo * pow(x, -1, M) % M
        else:
            y = int(rng.integers(0, M, dtype=np.uint64))
        if _borrows(x, y) == borrow:
            a.append(x); b.append(y)
    return a, b


def _lane_patterns():
    lane = np.arange(LANES)
    wave = lane // WAVE
    return {
        "one_lane_each_position": lane % WAVE == wave,  # wave w: lane w alone, every position 0..63 in turn
        "every_lane": np.ones(LANES, dtype=bool),
        "even_lanes": lane % 2 == 0,
        "odd_lanes": lane % 2 == 1,
        "first_and_last_wave_of_a_block": (wave % BLOCK_WAVES == 0) | (wave % BLOCK_WAVES == BLOCK_WAVES - 1),
        "no_lane": np.zeros(LANES, dtype=bool),
    }


def _pow7_classes():
    """x = c * 2^k: the product of two such values has a zero low word from 2^64 on and borrows from about 2^96 on, so k
    chooses the first product that borrows"""
    cls = {"first": [], "middle": [], "last": [], "none": []}
    for k in range(64):
        for c in (1, 3, 5, 7, 11, 0x1F, 0xFF, 0x101):
            x = c << k
            if x >= M:
                continue
            f = _pow7_borrows(x)
            if f[0]:
                cls["first"].append(x)
            elif f[1] or f[2]:
                cls["middle"].append(x)
            elif f[3]:
                cls["last"].append(x)
            else:
                cls["none"].append(x)
    return cls


def test_mul_and_pow7_lane_patterns(gpu_ctx):
    rng = np.random.default_rng(4242)
    pats = _lane_patterns()
    assert [int(m.sum()) for m in pats.values()] == [64, LANES, LANES // 2, LANES // 2, LANES // 2, 0]
    for w in range(64):  # exactly one lane of wave w, at position w
        assert np.nonzero(pats["one_lane_each_position"][w * WAVE:(w + 1) * WAVE])[0].tolist() == [w]
    ba, bb = _mul_pairs(rng, LANES, True)
    na, nb = _mul_pairs(rng, LANES, False)
    assert all(_borrows(x, y) for x, y in zip(ba, bb)) and not any(_borrows(x, y) for x, y in zip(na, nb))
    for name, mask in pats.items():
        A = [ba[i] if mask[i] else na[i] for i in range(LANES)]
        B = [bb[i] if mask[i] else nb[i] for i in range(LANES)]
        assert [_borrows(x, y) for x, y in zip(A, B)] == mask.tolist(), name
        got = gpu_ctx.field_op_batch("mul", np.array(A, dtype=np.uint64), np.array(B, dtype=np.uint64))
        want = np.array([x * y % P for x, y in zip(A, B)], dtype=np.uint64)
        assert (got == want).all(), ("mul", name, np.nonzero(got != want)[0][:4])

    cls = _pow7_classes()
    assert min(len(v) for v in cls.values()) >= 8, {k: len(v) for k, v in cls.items()}
    seen = set()
    for kind in ("first", "middle", "last"):
        hot = [cls[kind][int(i)] for i in rng.integers(0, len(cls[kind]), LANES)]
        cold = []
        while len(cold) < LANES:  # random values and the structured ones that never borrow
            x = int(rng.integers(0, M, dtype=np.uint64)) if len(cold) % 2 else cls["none"][len(cold) % len(cls["none"])]
            if not any(_pow7_borrows(x)):
                cold.append(x)
        for name, mask in pats.items():
            X = [hot[i] if mask[i] else cold[i] for i in range(LANES)]
            flags = [_pow7_borrows(x) for x in X]
            assert [any(f) for f in flags] == mask.tolist(), (kind, name)
            for i in np.nonzero(mask)[0]:
                f = flags[i]
                assert {"first": f[0], "middle": not f[0] and (f[1] or f[2]), "last": f == (False, False, False, True)}[kind], (kind, hex(X[i]), f)
                seen.add(f)
            got = gpu_ctx.field_op_batch("pow7", np.array(X, dtype=np.uint64), None)
            want = np.array([pow(x, 7, P) for x in X], dtype=np.uint64)
            assert (got == want).all(), ("pow7", kind, name, np.nonzero(got != want)[0][:4])
    # each of the four products is the one that borrows somewhere: x^2 (first), x^4 and x^3 (middle), x^7 alone (last)
    assert any(f[0] for f in seen) and any(f[1] for f in seen) and any(f[2] for f in seen) and (False, False, False, True) in seen, seen


def _plant(rng, rc, word):
    """a canonical s with s + rc[word] = m * 2^32 exactly (no wrap), 2^31 <= m <= 2^32 - 2: the square of the first-round S-box
    input of state word `word` then has a zero low word and borrows"""
    c = int(rc[word])
    lo_m = max(1 << 31, -(-c >> 32))
    assert lo_m <= (1 << 32) - 2, "round constant %d leaves no room" % word
    m = int(rng.integers(lo_m, (1 << 32) - 1))
    y = m << 32
    s = y - c
    assert 0 <= s < P and s + c == y < M and 1 << 31 <= m <= (1 << 32) - 2
    assert (y * y) % M == 0 and _borrows(y, y)
    return s


def _planted_lanes(count, all_lanes):
    if all_lanes:
        return list(range(count))
    return [i for i in range(count) if i % WAVE == (7 * (i // WAVE) + 3) % WAVE] or [0]  # one lane per wave, its position moving


@pytest.mark.parametrize("count", [1, 63, 64, 65, 5000])
def test_permutation_with_planted_first_round(gpu_ctx, oracle, count):
    rc = oracle.orc_poseidon_round_constants()
    rng = np.random.default_rng(900 + count)
    ran = 0
    for words in ([0], [11], [0, 5, 8, 11], list(range(12))):
        for all_lanes in (False, True):
            s = rand_field(rng, (count, 12), canonical=True)
            lanes = _planted_lanes(count, all_lanes)
            assert len(lanes) == count if all_lanes else 1 <= len(lanes) <= -(-count // WAVE)
            for i in lanes:
                for w in words:
                    s[i, w] = _plant(rng, rc, w)
            got = gpu_ctx.poseidon_permute_batch(s)
            want = np.zeros_like(s)
            oracle.orc_poseidon_permute_batch(vp(s), vp(want), count)
            assert (got == want).all(), (words, all_lanes, np.nonzero((got != want).any(axis=1))[0][:4])
            ran += 1
    assert ran == 8


@pytest.mark.parametrize("log_leaves,leaf_len,cap_height", [(7, 9, 1), (7, 135, 1), (7, 4, 1), (7, 4, 0), (14, 4, 4)])
def test_merkle_cap_with_planted_leaves(gpu_ctx, oracle, log_leaves, leaf_len, cap_height):
    """leaf_len 9 / 135: the first absorbed words are state words 0..7 of the first permutation of k_hash_leaves.  leaf_len 4: the
    leaves pass through unhashed and two of them are state words 0..7 of the first two_to_one: the lane-cooperative kernel at 2^7
    leaves (64 parents), k_merkle_level at 2^14 (8192 parents, above POS_COOP_MAX_NODES)."""
    rc = oracle.orc_poseidon_round_constants()
    rng = np.random.default_rng(70 + leaf_len + log_leaves)
    n = 1 << log_leaves
    ran = 0
    for words in ([0], [2, 7], list(range(8))):
        for all_lanes in (False, True):
            leaves = rand_field(rng, (n, leaf_len), canonical=True)
            if leaf_len == 4:  # parent i takes leaf 2i as words 0..3 and leaf 2i + 1 as words 4..7
                parents = _planted_lanes(n // 2, all_lanes)
                assert parents
                for i in parents:
                    for w in words:
                        leaves[2 * i + w // 4, w % 4] = _plant(rng, rc, w)
            else:
                rows = _planted_lanes(n, all_lanes)
                assert rows
                for i in rows:
                    for w in words:
                        leaves[i, w] = _plant(rng, rc, w)
            got = gpu_ctx.merkle_cap(leaves, cap_height)
            assert (got == merkle_cap(oracle, leaves, cap_height)).all(), (words, all_lanes)
            ran += 1
    assert ran == 6
