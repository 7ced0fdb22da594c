"""Shared by test_verify_batch_emu.py (CPU) and test_verify_batch.py (GPU): proofs of the circuits the suite already proves in
seconds, made by the ORACLE prover, and the tamper cases of the batch verifier with the code orc_verify gives each of them: batch(), a clean
proof and some fifteen hand-picked defects per circuit, and sweep(), one proof per changed word over whole sections of the layout."""
import concurrent.futures
import functools

import numpy as np

import oracle_lib

SYNTHETIC = (5, 6, 9)


def circuit_names():
    import test_high_rate
    return ["synthetic_%d" % d for d in SYNTHETIC] + list(test_high_rate.ORACLE_CONFIGS)


def make_circuit(m, name):
    import test_high_rate
    if name.startswith("synthetic_"):
        d = int(name.split("_")[1])
        return m.circuit.synthetic_circuit(m.standard_params(d, 4), seed=d)
    return test_high_rate.oracle_config(m, name)


def bump(m, proof, pos):
    bad = proof.copy()
    bad[pos] = np.uint64((int(bad[pos]) + 1) % m.GOLDILOCKS_P)
    return bad


STRATA = ("head", "queries", "noncanonical")
HIGH_RATE = "shrink_2"   # the high-rate config of the sweeps: its caps are a single digest, so a path is 14 siblings and ends at index 0
PIN_BYTES = 4 << 20      # lcp2_ctx::PIN_BYTES (csrc/internal.hpp)
HOST_CHUNK = 4096        # verify_batch.hip: no chunk holds more proofs
ORACLE_THREADS = 8       # a stratum is some hundred orc_verify calls of 10 to 30 ms


def device_chunk_bound(L):
    """verify_batch.hip stages the words outside the queries of every device proof of a chunk in the pinned buffer: no chunk of
    device proofs holds more than this many"""
    return PIN_BYTES // (8 * (L.queries + L.total - L.final_poly))


def stratum_spots(m, p, stratum):
    """(labels, positions, None | values) of a stratum: one proof per entry, word `position` of it changed - by bump where values is
    None.  head: every word outside the query section, label ("head", position).  queries: label (j, q), word j of query q - every
    offset j of a query once, the query rotating with j, and every word of the last query.  noncanonical: every 16th word of the
    proof set to p, every 16th from word 8 on to 2^64 - 1, label ("p" | "max", position)."""
    L = m.proof_layout(p)
    Q, qw = p.num_query_rounds, int(L.query_words)
    if stratum == "head":
        pos = list(range(0, L.queries)) + list(range(L.final_poly, L.total))
        return [("head", x) for x in pos], np.array(pos, dtype=np.int64), None
    if stratum == "queries":
        labels = [(j, j % Q) for j in range(qw)] + [(j, Q - 1) for j in range(qw) if j % Q != Q - 1]
        assert {j for j, q in labels} == set(range(qw)) and {q for j, q in labels} == set(range(Q)) and len(set(labels)) == len(labels)
        return labels, np.array([L.queries + q * qw + j for j, q in labels], dtype=np.int64), None
    assert stratum == "noncanonical"
    at_p, at_max = list(range(0, L.total, 16)), list(range(8, L.total, 16))
    values = np.array([m.GOLDILOCKS_P] * len(at_p) + [2 ** 64 - 1] * len(at_max), dtype=np.uint64)
    return [("p", x) for x in at_p] + [("max", x) for x in at_max], np.array(at_p + at_max, dtype=np.int64), values


@functools.lru_cache(maxsize=None)
def _proved(name):
    """(circ, digest, cap, the oracle's proof, public inputs) of circuit `name`"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = make_circuit(m, name)
    oc = oracle_lib.OracleCircuit(oracle_lib.load(), circ)
    proof = oc.prove(wires, pis)
    assert oc.verify(proof, pis) == 0
    digest, cap = oc.digest()
    oc.close()
    proof.setflags(write=False)
    return circ, digest, cap, proof, np.ascontiguousarray(pis, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _sweep_codes(name, stratum):
    """(labels, positions, values, want) of a stratum of circuit `name`: what costs oracle time, kept for the session; the proofs
    themselves (a hundred megabytes and more per stratum) are written out per call of sweep()"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, proof, pis = _proved(name)
    p = circ.params
    labels, pos, values = stratum_spots(m, p, stratum)
    if values is None:
        values = proof[pos] + np.uint64(1)  # proof words are < p < 2^64 - 1
        values[values == np.uint64(m.GOLDILOCKS_P)] = 0
    assert (values != proof[pos]).all()
    ov = oracle_lib.OracleCircuit.verifier_only(oracle_lib.load(), circ, digest, cap)
    want = np.zeros(len(labels), dtype=np.int32)

    def codes(mine):  # orc_verify keeps its state on its stack and ctypes drops the GIL for the call: the cases go over threads
        work = proof.copy()
        for i in mine:
            work[pos[i]] = values[i]
            want[i] = ov.verify(work, pis)
            work[pos[i]] = proof[pos[i]]
    with concurrent.futures.ThreadPoolExecutor(ORACLE_THREADS) as pool:
        list(pool.map(codes, [range(k, len(labels), ORACLE_THREADS) for k in range(ORACLE_THREADS)]))
    ov.close()
    bad = [(l, int(w)) for l, w in zip(labels, want) if w == 0]
    assert not bad, (name, stratum, bad[:8])  # a case is valid only if the oracle alone rejects it
    if stratum == "noncanonical":
        assert (want == 1).all(), (name, [(l, int(w)) for l, w in zip(labels, want) if w != 1][:8])
    if stratum == "queries":
        L = m.proof_layout(p)
        assert sorted({j for j, q in labels}) == list(range(L.query_words))  # no part of the layout has been dropped
        assert set(want) >= ({4, 5, 6} if p.num_fri_layers else {4}), (name, sorted(set(want)))
    for a in (pos, values, want):
        a.setflags(write=False)
    return labels, pos, values, want


def sweep(name, stratum):
    """(circ, digest, cap, labels, proofs (k, proof_words), public inputs (k, npi), want (k,) int32) of a stratum (STRATA,
    stratum_spots) of circuit `name`: k copies of the oracle's proof with one word changed each; want[i] is orc_verify's code, never 0.
    Read-only."""
    circ, digest, cap, proof, pis = _proved(name)
    labels, pos, values, want = _sweep_codes(name, stratum)
    proofs = np.repeat(proof[None, :], len(labels), axis=0)
    proofs[np.arange(len(labels)), pos] = values
    pis_all = np.repeat(pis[None, :], len(labels), axis=0)
    for a in (proofs, pis_all):
        a.setflags(write=False)
    return circ, digest, cap, labels, proofs, pis_all, want


@functools.lru_cache(maxsize=None)
def changed_public_input(name):
    """(public inputs with one bit changed, orc_verify's code for them with the clean proof)"""
    circ, digest, cap, proof, pis = _proved(name)
    bad_pis = pis.copy()
    bad_pis[1] ^= np.uint64(2)
    ov = oracle_lib.OracleCircuit.verifier_only(oracle_lib.load(), circ, digest, cap)
    code = ov.verify(proof, bad_pis)
    ov.close()
    assert code != 0
    bad_pis.setflags(write=False)
    return bad_pis, code


def clean(name):
    """(the oracle's proof, its public inputs) of circuit `name`: orc_verify accepts them"""
    return _proved(name)[3:]


@functools.lru_cache(maxsize=None)
def batch(name):
    """(circ, digest, cap, labels, proofs (k, proof_words), public inputs (k, npi), want (k,) int32) of circuit `name`: the clean proof
    and every tampered copy the issue lists; want[i] is orc_verify's code, and lcp2_verify names the same check.  Read-only."""
    import eth_lc_plonky2_amd as m
    import test_high_rate
    oracle = oracle_lib.load()
    circ, wires, pis = make_circuit(m, name)
    p = circ.params
    oc = oracle_lib.OracleCircuit(oracle, circ)
    proof = oc.prove(wires, pis)
    digest, cap = oc.digest()
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    L = m.proof_layout(p)
    Q, last = p.num_query_rounds, L.queries + (p.num_query_rounds - 1) * L.query_words
    cases = [("clean", proof, pis)]
    for section, pos in test_high_rate.tamper_spots(m, p).items():
        cases.append((section, bump(m, proof, pos), pis))
    cases.append(("last_query_leaf", bump(m, proof, last + L.q_init_off[1] + 2), pis))
    cases.append(("last_query_last_sibling", bump(m, proof, last + L.q_init_off[0] + L.q_init_cols[0] + 4 * (L.q_init_sib - 1) + 1), pis))
    for layer in range(p.num_fri_layers):
        q = (layer + 1) % Q
        cases.append(("fri_eval_layer_%d" % layer, bump(m, proof, L.queries + q * L.query_words + L.q_step_off[layer] + 1), pis))
    bad = proof.copy()
    bad[L.op_wires + 3] = np.uint64(m.GOLDILOCKS_P)
    cases.append(("noncanonical_head", bad, pis))
    bad = proof.copy()
    bad[L.queries + (Q // 2) * L.query_words + 7] = np.uint64(2 ** 64 - 1)
    cases.append(("noncanonical_query", bad, pis))
    bad_pis = pis.copy()
    bad_pis[1] ^= np.uint64(2)
    cases.append(("public_input", proof, bad_pis))
    # two defects: an initial sibling of query 3 and a final-polynomial word (which shows at query 0)
    q3 = L.queries + min(3, Q - 1) * L.query_words
    two = bump(m, bump(m, proof, q3 + L.q_init_off[2] + L.q_init_cols[2] + 5), L.final_poly + 1)
    cases.append(("two_defects", two, pis))
    if p.num_fri_layers and Q > 3:  # both inside the queries, so the transcript stands: an eval of query 0 (check 5) and a sibling of query 3 (check 4)
        cases.append(("two_query_defects", bump(m, bump(m, proof, q3 + L.q_init_off[2] + L.q_init_cols[2] + 5), L.queries + L.q_step_off[0] + 1), pis))
    want = []
    for label, pr, pi in cases:
        code = oc.verify(pr, pi)
        assert (code == 0) == (label == "clean"), (name, label, code)  # a case is valid only if the oracle rejects it
        got = 0
        try:
            vd.verify(pr, pi)
        except m.ProofRejected as e:
            got = e.check
        assert got == code, (name, label, got, code)
        want.append(code)
    oc.close()
    vd.close()
    proofs = np.ascontiguousarray(np.stack([c[1] for c in cases]), dtype=np.uint64)
    pis_all = np.ascontiguousarray(np.stack([c[2] for c in cases]), dtype=np.uint64)
    for a in (proofs, pis_all):
        a.setflags(write=False)
    return circ, digest, cap, [c[0] for c in cases], proofs, pis_all, np.array(want, dtype=np.int32)
