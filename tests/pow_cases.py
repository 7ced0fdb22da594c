"""Shared by test_pow_search.py: the parameter sets of the proof-of-work tests, the transcript of a proof replayed on the oracle's
permutation up to the point where fri_proof_of_work takes over (the full duplex sponge: state, pending inputs, witness slot), and
the same walk with the counts alone (how many inputs are pending), which needs no proof."""
import functools

import numpy as np

import oracle_lib

P = oracle_lib.P
BATCH = 1 << 20       # fri_proof_of_work (csrc/fri_commit.hip): candidates per k_pow_search launch
LATE_BITS = 20        # proof_of_work_bits of the late-batch cases
POW_CHECK = 2         # the verdict of a proof whose proof-of-work response has a leading one (orc_verify, lcp2_verify, lcp2_verify_batch)
CANON_CHECK = 1       # a proof word >= p

LATE_SEED = 21        # synthetic_circuit at degree_bits 5: ONE circuit for the three cases, which differ in the witness alone

# name -> (tag of circuit.tag_witness: a value in the free cells of the padding row, the oracle's minimum witness, [lo, hi) the witness
# must lie in).  The tags were chosen with the oracle alone, among tags 1 to 44: for A and B the witnesses closest to the start of their
# range (the oracle scans every candidate below the witness), for C a small one.
LATE_CASES = {
    "A_second_batch": (31, 1067102, (BATCH, 2 * BATCH)),
    "B_third_batch": (28, 2408444, (2 * BATCH, 3 * BATCH)),
    "C_first_batch": (21, 35113, (0, BATCH)),
}
# case B: a witness above the minimum that solves the same puzzle (found by scanning on with orc_poseidon_permute_batch)
B_LATER_SOLUTION = 3727059


def variant(m, degree_bits, **kw):
    """standard_params with fields replaced; fri_arity_bits=[...] sets the whole schedule (test_gpu_prover._variant)"""
    p = m.standard_params(degree_bits, 4)
    arities = kw.pop("fri_arity_bits", None)
    for k, v in kw.items():
        setattr(p, k, v)
    if arities is not None:
        p.num_fri_layers = len(arities)
        for i in range(8):
            p.fri_arity_bits[i] = arities[i] if i < len(arities) else 0
    return p


def late_params(m):
    return variant(m, 5, proof_of_work_bits=LATE_BITS, num_query_rounds=3)


@functools.lru_cache(maxsize=None)
def late_circuit():
    import eth_lc_plonky2_amd as m
    circ, wires, pis = m.circuit.synthetic_circuit(late_params(m), seed=LATE_SEED)
    return circ, wires, np.ascontiguousarray(pis, dtype=np.uint64)


def late_witness(tag):
    import eth_lc_plonky2_amd as m
    return m.circuit.tag_witness(late_circuit()[1].copy(), tag)


def oracle_proof(circ, wires, pis):
    """(the oracle's proof, its challenges, digest, cap)"""
    oc = oracle_lib.OracleCircuit(oracle_lib.load(), circ)
    proof = oc.prove(wires, pis)
    ch = oc.challenges()
    digest, cap = oc.digest()
    oc.close()
    return proof, ch, digest, cap


@functools.lru_cache(maxsize=None)
def late_case(name):
    """(circ, wires, public inputs, the oracle's proof, its challenges, digest, cap) of a case of LATE_CASES; the proof is read-only.
    This is where the oracle scans for the witness: the one expensive step, done once per session and case."""
    circ, _, pis = late_circuit()
    wires = late_witness(LATE_CASES[name][0])
    proof, ch, digest, cap = oracle_proof(circ, wires, pis)
    proof.setflags(write=False)
    return circ, wires, pis, proof, ch, digest, cap


# ---- the witness slot
SLOT_CASES = {
    # name: (degree_bits, fields, final_len, slot)
    "final_1": (5, dict(cap_height=2, fri_arity_bits=[3, 2]), 1, 2),
    "final_1_one_challenge": (5, dict(cap_height=2, fri_arity_bits=[3, 2], num_challenges=1), 1, 2),
    "final_2": (6, dict(cap_height=2, fri_arity_bits=[3, 2]), 2, 4),
    "final_2_wide_trace": (6, dict(cap_height=2, fri_arity_bits=[5], num_wires=150), 2, 4),
    "final_4": (6, dict(fri_arity_bits=[4]), 4, 0),
    "final_16": (8, dict(fri_arity_bits=[4]), 16, 0),
    "no_layers": (5, dict(fri_arity_bits=[]), 32, 0),
    "no_layers_one_challenge": (6, dict(fri_arity_bits=[], num_challenges=1), 64, 0),
}
REACHABLE_SLOTS = {0, 2, 4}


def slot_params(m, name):
    degree_bits, kw, _, _ = SLOT_CASES[name]
    return variant(m, degree_bits, proof_of_work_bits=8, num_query_rounds=3, **dict(kw))


class PendingCount:
    """HostChallenger with the values left out: the number of observed words no permutation has absorbed yet.  The eighth pending word
    is absorbed at once; a draw absorbs whatever is pending (and a draw that finds outputs left and nothing pending changes nothing)."""

    def __init__(self):
        self.pending = 0

    def observe(self, count):
        self.pending = (self.pending + count) % 8

    def draw(self, count=1):
        assert count >= 1
        self.pending = 0


def walk(t, p, words_of):
    """the prover's observes and draws from the circuit digest to the final polynomial (prove() in oracle/plonk.c; fri_open_commit in
    csrc/prover_open.hip and fri_commit_phase in csrc/fri_commit.hip) on a transcript `t` with observe(x) and draw(count);
    words_of(first, count) is what is observed for a span of the proof.  Returns the drawn values by name."""
    CH, NC, NR, W, Q = p.num_challenges, p.num_constants, p.num_routed_wires, p.num_wires, p.quotient_degree_factor
    npp = -(-NR // Q) - 1
    capw = 4 << p.cap_height
    final_len = 1 << (p.degree_bits - sum(p.fri_arity_bits[l] for l in range(p.num_fri_layers)))
    o = 3 * capw
    op_constants = o
    o += 2 * (NC + NR + W)
    op_zs = o
    o += 2 * CH
    op_zs_next = o
    o += 2 * CH
    op_pp = o
    o += 2 * CH * npp
    op_quot = o
    o += 2 * CH * Q
    fri_caps = o
    drawn = {}
    t.observe(words_of("digest", 4))
    t.observe(words_of("public_inputs_hash", 4))
    t.observe(words_of(0, capw))
    drawn["betas"], drawn["gammas"] = t.draw(CH), t.draw(CH)
    t.observe(words_of(capw, capw))
    drawn["alphas"] = t.draw(CH)
    t.observe(words_of(2 * capw, capw))
    drawn["zeta"] = t.draw(2)
    t.observe(words_of(op_constants, 2 * (NC + NR + W)))
    t.observe(words_of(op_zs, 2 * CH))
    t.observe(words_of(op_pp, 2 * CH * npp))
    t.observe(words_of(op_quot, 2 * CH * Q))
    t.observe(words_of(op_zs_next, 2 * CH))
    drawn["fri_alpha"] = t.draw(2)
    drawn["fri_betas"] = []
    for l in range(p.num_fri_layers):
        t.observe(words_of(fri_caps + l * capw, capw))
        drawn["fri_betas"].append(t.draw(2))
    return drawn, final_len


def slot_by_counting(p):
    """the slot fri_proof_of_work writes its candidates to under parameters p: the words pending once the final polynomial is observed"""
    t = PendingCount()
    _, final_len = walk(t, p, lambda first, count: count)
    t.observe(2 * final_len)
    return t.pending


class Replay:
    """oracle_lib.Challenger under the names walk() calls"""

    def __init__(self, oracle):
        self.ch = oracle_lib.Challenger(oracle)

    def observe(self, xs):
        self.ch.observe(xs)

    def draw(self, count=1):
        return [int(v) for v in self.ch.get(count)]


def replay(m, oracle, p, digest, pis, proof):
    """(Challenger as fri_proof_of_work finds it, drawn challenges): the transcript of `proof` up to and including the final polynomial"""
    pis = np.ascontiguousarray(pis, dtype=np.uint64)
    pi_hash = np.zeros(4, dtype=np.uint64)
    oracle.orc_hash_no_pad(oracle_lib.vp(pis), len(pis), oracle_lib.vp(pi_hash))
    given = {"digest": np.asarray(digest, dtype=np.uint64), "public_inputs_hash": pi_hash}
    t = Replay(oracle)
    drawn, final_len = walk(t, p, lambda first, count: given[first] if isinstance(first, str) else proof[first:first + count])
    L = m.proof_layout(p)
    assert final_len == L.final_len and L.pow_witness == L.final_poly + 2 * final_len   # walk() and the library lay the proof out alike
    assert L.op_quotient + 2 * p.num_challenges * p.quotient_degree_factor == L.fri_caps and L.op_zs_next + 2 * p.num_challenges == L.op_partial_products
    t.observe(proof[L.final_poly:L.final_poly + 2 * final_len])
    return t.ch, drawn


def pow_response(oracle, ch, witness):
    """the challenge drawn after `witness` is observed on a copy of `ch` (the word whose leading proof_of_work_bits must be zero), as
    k_pow_search computes it: the state with the pending inputs and the candidate written, one permutation, word 7"""
    s = ch.s.copy()
    for i, v in enumerate(ch.inp):
        s[i] = v
    s[len(ch.inp)] = int(witness) % P
    oracle.orc_poseidon_permute(oracle_lib.vp(s))
    return int(s[7])


def solves(oracle, ch, witness, bits):
    return pow_response(oracle, ch, witness) >> (64 - bits) == 0


def next_solution(oracle, ch, after, bits, chunk=1 << 16):
    """the smallest witness above `after` that solves the puzzle (orc_poseidon_permute_batch over chunks of candidates)"""
    base = ch.s.copy()
    for i, v in enumerate(ch.inp):
        base[i] = v
    start = after + 1
    while True:
        states = np.repeat(base[None, :], chunk, axis=0)
        states[:, len(ch.inp)] = np.arange(start, start + chunk, dtype=np.uint64)
        out = np.zeros_like(states)
        oracle.orc_poseidon_permute_batch(oracle_lib.vp(states), oracle_lib.vp(out), chunk)
        hit = np.nonzero(out[:, 7] >> np.uint64(64 - bits) == 0)[0]
        if hit.size:
            return start + int(hit[0])
        start += chunk
