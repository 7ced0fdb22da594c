"""Openings of bare oracles (lcp2_fri_prove_openings / lcp2_fri_verify_openings): an independent model of the proof layout, of the
verifier and - for small shapes - of the prover, written from the definitions in include/lcp2.h over Python integers: the
challenger and the Merkle paths hash with poseidon_py, a fold is the interpolant through the coset evaluated at beta (Lagrange, from
the points themselves), the final polynomial is Horner.  No arithmetic is shared with csrc/fri_openings.hpp.
cfg is anything with rate_bits, cap_height, proof_of_work_bits, num_query_rounds, num_fri_layers and fri_arity_bits (binding.FriConfig
does); an instance is points_ranges = [[(oracle, first_poly, num_polys), ...] per point]; extension elements are pairs (c0, c1)."""
from types import SimpleNamespace

import numpy as np

from . import poseidon_py

P = poseidon_py.P
W = 7          # F_p[X] / (X^2 - 7)
GENERATOR = 7  # the coset shift of every LDE
ROOT_2_32 = 1753635133440165772
CHECKS = {1: "non-canonical word", 2: "proof of work", 3: "initial Merkle path", 4: "FRI layer path", 5: "fold consistency",
          6: "final polynomial", 7: "query at an opened point"}


# ------------------------------------------------------------------ field
def root_of_unity(bits):
    return pow(ROOT_2_32, 1 << (32 - bits), P)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_inv(a):
    norm = pow((a[0] * a[0] - W * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * norm % P, (-a[1]) * norm % P)


def e_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = e_mul(r, a)
        a, e = e_mul(a, a), e >> 1
    return r


def e_horner(coeffs, x):
    """sum_i coeffs[i] x^i for extension or base coefficients"""
    r = (0, 0)
    for c in reversed(list(coeffs)):
        r = e_add(e_mul(r, x), c if isinstance(c, tuple) else (int(c) % P, 0))
    return r


# ------------------------------------------------------------------ layout
def layout(cfg, log_n, oracle_cols, points_ranges):
    """word offsets of the proof: the openings of each point, the FRI caps, the query rounds (per round the leaf and siblings of
    every oracle, then evaluations and siblings of every layer), the final polynomial, the PoW witness"""
    capw, lg = 4 << cfg.cap_height, log_n + cfg.rate_bits
    point_polys = [sum(r[2] for r in ranges) for ranges in points_ranges]
    point_off = [2 * sum(point_polys[:b]) for b in range(len(point_polys))]
    fri_caps = 2 * sum(point_polys)
    init_sib, at, init_off = lg - cfg.cap_height, 0, []
    for cols in oracle_cols:
        init_off.append(at)
        at += cols + 4 * init_sib
    step_off, step_sib, final_bits = [], [], log_n
    arity = [cfg.fri_arity_bits[l] for l in range(cfg.num_fri_layers)]
    for a in arity:
        lg, final_bits = lg - a, final_bits - a
        step_off.append(at)
        step_sib.append(lg - cfg.cap_height)
        at += (2 << a) + 4 * (lg - cfg.cap_height)
    queries = fri_caps + len(arity) * capw
    final_poly = queries + at * cfg.num_query_rounds
    return SimpleNamespace(point_polys=point_polys, point_off=point_off, fri_caps=fri_caps, capw=capw, queries=queries, query_words=at,
                           init_off=init_off, init_cols=list(oracle_cols), init_sib=init_sib, step_off=step_off, step_sib=step_sib, arity=arity,
                           final_poly=final_poly, final_len=1 << final_bits, pow_witness=final_poly + 2 * (1 << final_bits),
                           total=final_poly + 2 * (1 << final_bits) + 1, lgN=log_n + cfg.rate_bits)


def sections(L):
    """(name, first word, words) of every section, for tests that spread positions over them"""
    return [("openings", 0, L.fri_caps), ("fri_caps", L.fri_caps, L.queries - L.fri_caps), ("queries", L.queries, L.final_poly - L.queries),
            ("final_poly", L.final_poly, 2 * L.final_len), ("pow_witness", L.pow_witness, 1)]


# ------------------------------------------------------------------ transcript and hashing
class Challenger:
    """plonky2's Challenger: duplex sponge in overwrite mode, rate 8, challenges popped from the back of the output"""

    def __init__(self, state=None):
        if state is None:
            self.sponge, self.inp, self.out = [0] * 12, [], []
        else:  # a binding.ChallengerState
            self.sponge = [int(v) for v in state.sponge]
            self.inp = [int(v) for v in state.input][:state.input_len]
            self.out = [int(v) for v in state.output][:state.output_len]

    def _duplex(self):
        self.sponge[:len(self.inp)] = self.inp
        self.inp = []
        self.sponge = poseidon_py.permute(self.sponge)
        self.out = self.sponge[:8]

    def observe(self, values):
        for v in values:
            self.out = []
            self.inp.append(int(v) % P)
            if len(self.inp) == 8:
                self._duplex()

    def get(self):
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def get_ext(self):
        a = self.get()
        return (a, self.get())

    def words(self):
        """(sponge, pending inputs, remaining outputs): what two transcripts must agree in"""
        return list(self.sponge), list(self.inp), list(self.out)


def state_words(state):
    """the same triple of a binding.ChallengerState"""
    return Challenger(state).words()


def hash_or_noop(words):
    words = [int(w) % P for w in words]
    return words + [0] * (4 - len(words)) if len(words) <= 4 else poseidon_py.hash_no_pad(words)


def two_to_one(left, right):
    return poseidon_py.permute(list(left) + list(right) + [0] * 4)[:4]


def merkle_root_of_path(leaf, index, siblings):
    """the cap entry a path leads to, and its index in the cap"""
    cur = hash_or_noop(leaf)
    for k in range(len(siblings) // 4):
        sib = [int(v) for v in siblings[4 * k:4 * k + 4]]
        cur = two_to_one(sib, cur) if index & 1 else two_to_one(cur, sib)
        index >>= 1
    return cur, index


def merkle_tree(leaves, cap_height):
    """levels[0] = leaf digests ... levels[-1] = the cap"""
    levels = [[hash_or_noop(l) for l in leaves]]
    while len(levels[-1]) > (1 << cap_height):
        prev = levels[-1]
        levels.append([two_to_one(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
    return levels


# ------------------------------------------------------------------ the verifier
def query_points(L, x_index):
    return GENERATOR * pow(root_of_unity(L.lgN), bitrev(x_index, L.lgN), P) % P


def verify(caps, cfg, log_n, oracle_cols, points_ranges, points, challenger, proof):
    """0 if the proof is accepted, else the failed check (CHECKS); the challenger ends in the state after the query indices.
    caps[o]: the 4 << cap_height words of oracle o; points: [(c0, c1)]; proof: the words"""
    L = layout(cfg, log_n, oracle_cols, points_ranges)
    proof = [int(w) for w in proof]
    assert len(proof) == L.total
    if any(w >= P for w in proof):
        return 1
    points = [(int(z[0]) % P, int(z[1]) % P) for z in points]
    ch = challenger
    ch.observe(proof[:L.fri_caps])
    alpha = ch.get_ext()
    ext = lambda at: (proof[at], proof[at + 1])
    reduced = [e_horner([ext(L.point_off[b] + 2 * j) for j in range(L.point_polys[b])], alpha) for b in range(len(points))]
    betas = []
    for l in range(len(L.arity)):
        ch.observe(proof[L.fri_caps + l * L.capw:L.fri_caps + (l + 1) * L.capw])
        betas.append(ch.get_ext())
    ch.observe(proof[L.final_poly:L.final_poly + 2 * L.final_len])
    ch.observe([proof[L.pow_witness]])
    response = ch.get()
    indices = [ch.get() % (1 << L.lgN) for _ in range(cfg.num_query_rounds)]
    if cfg.proof_of_work_bits and response >> (64 - cfg.proof_of_work_bits):
        return 2
    final = [ext(L.final_poly + 2 * j) for j in range(L.final_len)]
    for q, x_index in enumerate(indices):
        R = proof[L.queries + q * L.query_words:L.queries + (q + 1) * L.query_words]
        leaves = []
        for o, cols in enumerate(oracle_cols):
            leaf = R[L.init_off[o]:L.init_off[o] + cols]
            root, at = merkle_root_of_path(leaf, x_index, R[L.init_off[o] + cols:L.init_off[o] + cols + 4 * L.init_sib])
            if root != [int(v) % P for v in np.asarray(caps[o]).ravel()[4 * at:4 * at + 4]]:
                return 3
            leaves.append(leaf)
        x = query_points(L, x_index)
        if any(z == (x, 0) for z in points):
            return 7
        value = (0, 0)
        for b, ranges in enumerate(points_ranges):
            at_x = e_horner([leaves[o][first + j] for (o, first, count) in ranges for j in range(count)], alpha)
            term = e_mul(e_sub(at_x, reduced[b]), e_inv(e_sub((x, 0), points[b])))
            value = e_add(e_mul(value, e_pow(alpha, L.point_polys[b])), term)
        lg, shift, idx = L.lgN, GENERATOR, x_index
        for l, a in enumerate(L.arity):
            evals = [ext(L.queries + q * L.query_words + L.step_off[l] + 2 * j) for j in range(1 << a)]
            if evals[idx & ((1 << a) - 1)] != value:
                return 5
            leaf_index = idx >> a
            leaf = R[L.step_off[l]:L.step_off[l] + (2 << a)]
            root, at = merkle_root_of_path(leaf, leaf_index, R[L.step_off[l] + (2 << a):L.step_off[l] + (2 << a) + 4 * L.step_sib[l]])
            if root != proof[L.fri_caps + l * L.capw + 4 * at:L.fri_caps + l * L.capw + 4 * at + 4]:
                return 4
            # the interpolant through the coset's points, at beta
            w = root_of_unity(lg)
            xs = [shift * pow(w, bitrev((leaf_index << a) + j, lg), P) % P for j in range(1 << a)]
            value = (0, 0)
            for j, xj in enumerate(xs):
                num, den = (1, 0), 1
                for k, xk in enumerate(xs):
                    if k != j:
                        num, den = e_mul(num, e_sub(betas[l], (xk, 0))), den * (xj - xk) % P
                inv = pow(den, P - 2, P)
                value = e_add(value, e_mul(evals[j], (num[0] * inv % P, num[1] * inv % P)))
            lg, shift, idx = lg - a, pow(shift, 1 << a, P), leaf_index
        y = shift * pow(root_of_unity(lg), bitrev(idx, lg), P) % P if lg else shift
        if e_horner(final, (y, 0)) != value:
            return 6
    return 0


def query_indices(cfg, log_n, oracle_cols, points_ranges, challenger, proof):
    """the indices the transcript gives for this proof (a copy of the challenger is advanced, not the argument)"""
    L = layout(cfg, log_n, oracle_cols, points_ranges)
    ch = Challenger()
    ch.sponge, ch.inp, ch.out = challenger.words()
    proof = [int(w) for w in proof]
    ch.observe(proof[:L.fri_caps])
    ch.get_ext()
    for l in range(len(L.arity)):
        ch.observe(proof[L.fri_caps + l * L.capw:L.fri_caps + (l + 1) * L.capw])
        ch.get_ext()
    ch.observe(proof[L.final_poly:L.final_poly + 2 * L.final_len])
    ch.observe([proof[L.pow_witness]])
    ch.get()
    return [ch.get() % (1 << L.lgN) for _ in range(cfg.num_query_rounds)]


# ------------------------------------------------------------------ the prover, for small shapes (every step by definition, O(N n) evaluation)
def poly_div_linear(coeffs, z):
    """(C - C(z)) / (X - z) by synthetic division; coeffs extension, ascending"""
    out, carry = [(0, 0)] * len(coeffs), (0, 0)
    for i in range(len(coeffs) - 1, 0, -1):
        carry = e_add(coeffs[i], e_mul(carry, z))
        out[i - 1] = carry
    return out


def lde(coeffs, lg, shift):
    """values in leaf order: out[i] = C(shift w^bitrev(i))"""
    w = root_of_unity(lg)
    return [e_horner(coeffs, (shift * pow(w, bitrev(i, lg), P) % P, 0)) for i in range(1 << lg)]


def commit(coeff_cols, log_n, rate_bits, cap_height):
    """an oracle of base-field coefficient columns: (leaves in leaf order, Merkle levels)"""
    lg = log_n + rate_bits
    vals = [[v[0] for v in lde([int(c) for c in col], lg, GENERATOR)] for col in coeff_cols]
    leaves = [[vals[c][i] for c in range(len(coeff_cols))] for i in range(1 << lg)]
    return leaves, merkle_tree(leaves, cap_height)


def path(levels, index):
    out = []
    for lv in levels[:-1]:
        out += lv[index ^ 1]
        index >>= 1
    return out


def prove(coeff_cols_per_oracle, cfg, log_n, points_ranges, points, challenger, oracles=None, first_witness=0):
    """(proof words, caps of the oracles); the challenger ends in the state after the query indices.  oracles: the commit() of every
    oracle, where the caller has them already.  first_witness: where the proof-of-work scan starts - a caller that has shown by other
    means that no smaller witness passes spares the model a scan of millions of permutations in Python"""
    oracle_cols = [len(c) for c in coeff_cols_per_oracle]
    L = layout(cfg, log_n, oracle_cols, points_ranges)
    points = [(int(z[0]) % P, int(z[1]) % P) for z in points]
    if oracles is None:
        oracles = [commit(cols, log_n, cfg.rate_bits, cfg.cap_height) for cols in coeff_cols_per_oracle]
    proof = [0] * L.total
    batches = [[[int(c) for c in coeff_cols_per_oracle[o][first + j]] for (o, first, count) in ranges for j in range(count)] for ranges in points_ranges]
    at = 0
    for b, polys in enumerate(batches):
        for poly in polys:
            proof[at], proof[at + 1] = e_horner(poly, points[b])
            at += 2
    ch = challenger
    ch.observe(proof[:L.fri_caps])
    alpha = ch.get_ext()
    n = 1 << log_n
    total = [(0, 0)] * n
    for b, polys in enumerate(batches):
        comb, w = [(0, 0)] * n, (1, 0)
        for poly in polys:
            comb = [e_add(comb[i], (w[0] * poly[i] % P, w[1] * poly[i] % P)) for i in range(n)]
            w = e_mul(w, alpha)
        quot = poly_div_linear(comb, points[b])
        total = [e_add(e_mul(total[i], w), quot[i]) for i in range(n)]   # w = alpha^(polynomials of the batch)
    coeffs, lg, shift, layers = total, L.lgN, GENERATOR, []
    for l, a in enumerate(L.arity):
        vals = lde(coeffs, lg, shift)
        leaves = [[w for v in vals[i << a:(i + 1) << a] for w in v] for i in range(len(vals) >> a)]
        levels = merkle_tree(leaves, cfg.cap_height)
        layers.append((leaves, levels))
        cap = [w for d in levels[-1] for w in d]
        proof[L.fri_caps + l * L.capw:L.fri_caps + (l + 1) * L.capw] = cap
        ch.observe(cap)
        beta = ch.get_ext()
        coeffs = [e_horner(coeffs[k << a:(k + 1) << a], beta) for k in range(len(coeffs) >> a)]
        lg, shift = lg - a, pow(shift, 1 << a, P)
    assert len(coeffs) == L.final_len
    proof[L.final_poly:L.final_poly + 2 * L.final_len] = [w for c in coeffs for w in c]
    ch.observe(proof[L.final_poly:L.final_poly + 2 * L.final_len])
    witness = first_witness
    while cfg.proof_of_work_bits:
        trial = Challenger()
        trial.sponge, trial.inp, trial.out = ch.words()
        trial.observe([witness])
        if trial.get() >> (64 - cfg.proof_of_work_bits) == 0:
            break
        witness += 1
    proof[L.pow_witness] = witness
    ch.observe([witness])
    ch.get()
    for q in range(cfg.num_query_rounds):
        idx = ch.get() % (1 << L.lgN)
        R = L.queries + q * L.query_words
        for o, (leaves, levels) in enumerate(oracles):
            row = leaves[idx] + path(levels, idx)
            proof[R + L.init_off[o]:R + L.init_off[o] + len(row)] = row
        for l, a in enumerate(L.arity):
            idx >>= a
            row = layers[l][0][idx] + path(layers[l][1], idx)
            proof[R + L.step_off[l]:R + L.step_off[l] + len(row)] = row
    caps = [np.array([w for d in levels[-1] for w in d], dtype=np.uint64) for (_, levels) in oracles]
    return np.array(proof, dtype=np.uint64), caps
