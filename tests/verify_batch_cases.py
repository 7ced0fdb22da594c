"""Shared by test_verify_batch_emu.py (CPU) and test_verify_batch.py (GPU): proofs of the circuits the suite already proves in
seconds, made by the ORACLE prover, and the tamper cases of the batch verifier with the code orc_verify gives each of them."""
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
