"""The proof-of-work search of the FRI tail (fri_proof_of_work and k_pow_search) beyond its first batch, the slot the candidate is
written to, and the verifiers at the witness word - against the oracle, word for word.

fri_proof_of_work scans 2^20 candidates per launch.  Every other proof of the suite has at most 16 proof-of-work bits, so its
witness lies in the first batch and the second reset of the result word, a non-zero start, and the exit after an empty batch
never ran.  Here proof_of_work_bits = 20 on the smallest circuit (2^5 rows, one circuit and one CircuitData), and the witnesses of
pow_cases.LATE_CASES - the synthetic witness with another value in the free cells of its padding row - were chosen on the CPU
with the oracle alone, so that the minimum proof-of-work witness lies in the second batch (A: [2^20, 2^21)), in the third, behind
an empty batch (B: [2^21, 3 * 2^20)), and in the first (C, the control).  The only cost is the oracle's own scan of every candidate
below the witness, about 2.4 us per candidate on 8 cores: measured at 3.7 s for A (witness 1.02 * 2^20), 5.9 s for B (2.30 * 2^20)
and 0.2 s for C there, and at 0.5 s, 1.05 s and under 0.1 s on the 16 threads of a GPU host; once per session (the GPU side of
each proof is milliseconds).  At 21 bits and ranges up to 2^22 the scan of a
case B took 6.4 s and could take 10 s, so the cases use 20 bits and these narrower ranges; no witness of 2^21 or more can be had
for less than 2^21 permutations of the oracle.

The witness slot.  k_pow_search writes the candidate to word `pos` of the duplex state, pos = the number of words that are
pending when the witness is observed (HostChallenger::pow_state).  What is observed last before the witness is the final
polynomial, 2 final_len words (final_len extension-field coefficients), and right before it a challenge was drawn - the last
FRI beta, or with no FRI layers the FRI alpha, which follows the openings - and a draw absorbs whatever was pending.  So
pos = 2 final_len mod 8, whatever num_challenges, num_wires and num_constants are (they change only what is absorbed before
that draw):

    schedule                                       final_len    pos
    degree_bits 5, arities [3, 2]                   1            2     (also with num_challenges 1)
    degree_bits 6, arities [3, 2] or [5]            2            4     (also with 150 wires)
    degree_bits 6, arities [4]                      4            0     (8 words: absorbed at once)
    degree_bits 8, arities [4]                      16           0
    no layers, degree_bits 5 or 6                   32, 64       0     (final_len = 2^degree_bits; also with num_challenges 1)

Reachable: {0, 2, 4}.  Not reachable under the checks of lcp2_circuit_create: the odd positions (extension-field elements are
two words and the count starts at zero after a draw), 6 (2 * 2^k mod 8 is 2, 4 or 0), and 8 to 11 (the eighth pending word is
absorbed at once, so the capacity words of the 12-way compare in k_pow_search never hold the candidate).  A caller of the staged
seam cannot reach them either: lcp2_fri_open_begin takes a transcript state, but the FRI alpha is drawn after it.
pow_cases.SLOT_CASES holds one or more parameter sets per reachable position; test_slot_table_is_the_reachable_set derives the
position of each with a sponge model of its own and holds the table above to it."""
import ctypes

import numpy as np
import pytest

import oracle_lib
import pow_cases as pc
from oracle_lib import first_mismatch as _first_mismatch

gpu = pytest.mark.gpu
LATE = list(pc.LATE_CASES)
CASE_A, CASE_B, CASE_C = LATE


# ------------------------------------------------------------------ on the CPU: the fixtures themselves
@pytest.mark.parametrize("name", LATE)
def test_oracle_witness_lies_in_its_batch(oracle, name):
    """the recorded witness of each case is what the oracle finds today, and it lies in the batch the case is named after: a change
    to the synthetic circuit must not turn a late-batch case into a first-batch case unnoticed.  The replayed transcript agrees with
    the oracle's (same FRI alpha), the witness solves the puzzle in the model and its predecessor does not."""
    import eth_lc_plonky2_amd as m
    seed, recorded, (lo, hi) = pc.LATE_CASES[name]
    circ, wires, pis, proof, ch, digest, cap = pc.late_case(name)
    assert circ.params.proof_of_work_bits == pc.LATE_BITS == 20 and circ.params.degree_bits == 5
    assert pc.LATE_CASES[CASE_A][2] == (1 << 20, 1 << 21) and pc.LATE_CASES[CASE_B][2] == (1 << 21, 3 << 20) and pc.LATE_CASES[CASE_C][2] == (0, 1 << 20)
    witness = int(ch.pow_witness)
    assert witness == recorded == int(proof[m.proof_layout(circ.params).pow_witness])
    assert lo <= witness < hi, (name, witness, witness / pc.BATCH)
    t, drawn = pc.replay(m, oracle, circ.params, digest, pis, proof)
    assert drawn["fri_alpha"] == list(ch.fri_alpha) and drawn["zeta"] == list(ch.zeta)
    assert len(t.inp) == pc.slot_by_counting(circ.params) == 0   # final_len 32
    assert pc.solves(oracle, t, witness, pc.LATE_BITS)
    assert witness == 0 or not pc.solves(oracle, t, witness - 1, pc.LATE_BITS)


def test_slot_table_is_the_reachable_set():
    """the position in each row of pow_cases.SLOT_CASES is what the counting model gives for its parameters, the positions covered are
    exactly the reachable set of the module docstring, and no column count, challenge count or schedule that the parameter checks
    admit gives another position"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    covered = set()
    for name, (degree_bits, kw, final_len, slot) in pc.SLOT_CASES.items():
        p = pc.slot_params(m, name)
        assert lib.lcp2_proof_words(ctypes.byref(p)) > 0, name   # the parameter checks of build() accept it
        assert m.proof_layout(p).final_len == final_len, name
        assert pc.slot_by_counting(p) == slot == 2 * final_len % 8, name
        covered.add(slot)
    assert covered == pc.REACHABLE_SLOTS == {0, 2, 4}
    assert {f for _, _, f, _ in pc.SLOT_CASES.values()} >= {1, 2, 4, 16}
    seen = set()
    for degree_bits in range(1, 9):
        for arities in ([], [1], [2], [3], [4], [5], [1, 1], [2, 1], [3, 2], [1, 1, 1], [4, 4]):
            for ch in (1, 2):
                for wires, routed, constants in ((135, 80, 4), (150, 80, 4), (136, 79, 5), (9, 3, 1)):
                    p = pc.variant(m, degree_bits, cap_height=0, fri_arity_bits=arities, num_challenges=ch, num_wires=wires,
                                   num_routed_wires=routed, num_constants=constants, proof_of_work_bits=8)
                    if lib.lcp2_proof_words(ctypes.byref(p)) == 0:
                        continue   # refused: the schedule takes more than degree_bits
                    assert pc.slot_by_counting(p) == 2 * m.proof_layout(p).final_len % 8
                    seen.add(pc.slot_by_counting(p))
    assert seen == pc.REACHABLE_SLOTS


# ------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("bits,accepted", [(0, False), (1, True), (40, True), (41, False)])
def test_circuit_create_bounds_of_proof_of_work_bits(gpu_ctx, bits, accepted):
    """lcp2_circuit_create (which needs a context, hence a device) refuses 0 and 41 bits with a reason that names the parameter and
    builds at 1 and 40; nothing is proved at 40 bits.  The same bounds of lcp2_verifier_create, on the CPU: test_host_verifier.py.
    (lcp2_params_config checks no proof_of_work_bits: it fills the structure and the constructors judge it.)"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = m.circuit.synthetic_circuit(m.standard_params(5, 4), seed=3)
    circ.params = pc.variant(m, 5, proof_of_work_bits=bits)
    if accepted:
        m.CircuitData.build(gpu_ctx, circ).close()
        return
    with pytest.raises(m.Lcp2Error) as e:
        m.CircuitData.build(gpu_ctx, circ)
    assert e.value.status == -6 and "proof_of_work_bits" in str(e.value)


@pytest.fixture(scope="module")
def late(gpu_ctx):
    """ONE CircuitData for the three cases (they differ in the witness alone) and, for each case, the first proof lcp2_prove gives
    on it with the challenges of that proof, proved in the order A, B, C.  The handle is shared by the tests below."""
    import eth_lc_plonky2_amd as m
    out = {"data": m.CircuitData.build(gpu_ctx, pc.late_circuit()[0]), "first": {}, "challenges": {}}
    for name in LATE:
        circ, wires, pis = pc.late_case(name)[:3]
        out["first"][name] = out["data"].prove(wires, pis)
        out["challenges"][name] = out["data"].last_challenges()
    yield out
    out["data"].close()


@gpu
@pytest.mark.parametrize("name", LATE)
def test_late_batch_proof_equals_oracle(gpu_ctx, oracle, late, name):
    """lcp2_prove with the witness in the second batch (A), behind at least one empty batch (B) and in the first (C): the proof is the
    oracle's in every word, the witness is the oracle's minimum, the query indices - drawn after the witness is observed - are the
    oracle's, and the host verifier, a verifier-only handle, lcp2_verify_batch (host and device head) and the oracle accept it"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, want, ch_o, digest, cap = pc.late_case(name)
    data, got, ch_g = late["data"], late["first"][name], late["challenges"][name]
    lo, hi = pc.LATE_CASES[name][2]
    assert lo <= int(ch_o.pow_witness) < hi
    assert ch_g["pow_witness"] == int(ch_o.pow_witness), (name, ch_g["pow_witness"], int(ch_o.pow_witness))
    assert list(ch_g["query_indices"]) == list(ch_o.query_indices)
    assert list(ch_g["fri_alpha"]) == list(ch_o.fri_alpha)
    assert _first_mismatch(m, circ.params, got, want) is None, name + ": " + _first_mismatch(m, circ.params, got, want)
    d_gpu, cap_gpu = data.digest()
    assert (d_gpu == digest).all() and (cap_gpu == cap).all()
    data.verify(got, pis)
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    vd.verify(got, pis)
    for head in ("host", "device"):
        assert list(gpu_ctx.verify_batch(vd, got[None, :], pis[None, :], head=head)) == [0], head
        assert list(gpu_ctx.verify_batch(data, got[None, :], pis[None, :], head=head)) == [0], head
    ov = oracle_lib.OracleCircuit.verifier_only(oracle, circ, digest, cap)
    assert ov.verify(got, pis) == 0
    ov.close()
    vd.close()


@gpu
def test_no_result_word_leaks_between_proofs(gpu_ctx, late):
    """B, then C, then B again - and A, C, A after them - on the same CircuitData: every proof is the first proof of its case (which
    is the oracle's) and reports its own witness.  A result word left by a late-batch proof does not reach the next proof, and a
    first-batch proof after a late one does not start from a late batch."""
    data = late["data"]
    for name in (CASE_B, CASE_C, CASE_B, CASE_A, CASE_C, CASE_A):
        circ, wires, pis, want, ch_o = pc.late_case(name)[:5]
        again = data.prove(wires, pis)
        assert data.last_challenges()["pow_witness"] == int(ch_o.pow_witness), name
        assert (again == late["first"][name]).all() and (again == want).all(), name


@gpu
def test_late_batch_through_the_staged_seam(gpu_ctx, oracle, late):
    """case A through lcp2_commit_wires -> lcp2_perm_zs -> lcp2_quotient -> lcp2_fri_open_begin / _commit / _finish with the
    transcript run by the caller (test_staged_seams_compose_to_prove): the proof of lcp2_prove, which is the oracle's"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, want, ch_o, digest, cap = pc.late_case(CASE_A)
    params, data = circ.params, late["data"]
    capw, CH = 4 << params.cap_height, params.num_challenges
    proof = np.zeros(data.proof_words, dtype=np.uint64)
    pi_hash = np.zeros(4, dtype=np.uint64)
    oracle.orc_hash_no_pad(oracle_lib.vp(pis), len(pis), oracle_lib.vp(pi_hash))
    t = oracle_lib.Challenger(oracle)
    t.observe(digest)
    t.observe(pi_hash)
    proof[0:capw] = data.commit_wires(wires).ravel()
    t.observe(proof[0:capw])
    betas, gammas = t.get(CH), t.get(CH)
    proof[capw:2 * capw] = data.perm_zs(betas, gammas).ravel()
    t.observe(proof[capw:2 * capw])
    alphas = t.get(CH)
    proof[2 * capw:3 * capw] = data.quotient(alphas, pi_hash).ravel()
    t.observe(proof[2 * capw:3 * capw])
    zeta = t.get(2)
    assert list(zeta) == list(ch_o.zeta)
    st = t.state(m)
    data.fri_open_begin(zeta, st, proof)
    data.fri_open_commit(proof)
    data.fri_open_finish(proof, st)
    assert int(proof[m.proof_layout(params).pow_witness]) == int(ch_o.pow_witness) >= pc.BATCH   # (lcp2_last_challenges records lcp2_prove alone)
    assert _first_mismatch(m, params, proof, want) is None, _first_mismatch(m, params, proof, want)
    assert (proof == late["first"][CASE_A]).all()
    # and lcp2_prove after the seam gives its proof again
    assert (data.prove(wires, pis) == late["first"][CASE_A]).all()


@gpu
@pytest.mark.parametrize("name", list(pc.SLOT_CASES))
def test_every_reachable_witness_slot_equals_oracle(gpu_ctx, oracle, name):
    """one proof per row of pow_cases.SLOT_CASES (module docstring): the witness slot is the one the table names - by counting and in
    the replayed transcript - and the GPU proof is the oracle's in every word, witness and query indices included"""
    import eth_lc_plonky2_amd as m
    degree_bits, kw, final_len, slot = pc.SLOT_CASES[name]
    params = pc.slot_params(m, name)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=900 + degree_bits)
    oc = oracle_lib.OracleCircuit(oracle, circ)
    assert oc.check_witness(wires, pis)[0] == 0
    want = oc.prove(wires, pis)
    ch_o = oc.challenges()
    assert oc.verify(want, pis) == 0
    digest, cap = oc.digest()
    t, drawn = pc.replay(m, oracle, params, digest, pis, want)
    assert drawn["fri_alpha"] == list(ch_o.fri_alpha)
    assert len(t.inp) == pc.slot_by_counting(params) == slot
    assert pc.solves(oracle, t, int(ch_o.pow_witness), params.proof_of_work_bits)
    data = m.CircuitData.build(gpu_ctx, circ)
    got = data.prove(wires, pis)
    ch_g = data.last_challenges()
    assert ch_g["pow_witness"] == int(ch_o.pow_witness), (name, slot)
    assert list(ch_g["query_indices"]) == list(ch_o.query_indices)
    assert _first_mismatch(m, params, got, want) is None, name + ": " + _first_mismatch(m, params, got, want)
    data.verify(got, pis)
    for head in ("host", "device"):
        assert list(gpu_ctx.verify_batch(data, got[None, :], pis[None, :], head=head)) == [0], head
    data.close()
    oc.close()


def _verdict(m, vd, proof, pis):
    try:
        vd.verify(proof, pis)
    except m.ProofRejected as e:
        return e.check
    return 0


@pytest.fixture(scope="module")
def witness_word_cases(oracle):
    """(circ, digest, cap, labels, proofs, public inputs, want) around the witness word of the case-B proof (witness >= 2^21):
    clean; witness - 1, which the minimum property makes a non-solution (check 2); witness + p, the same field element in a word that is not
    canonical (check 1, before any permutation); a later solution of the same puzzle (the response passes, so the verdict moves
    off check 2: the query indices it leads to are not the ones the proof answers).  want is orc_verify's code for each."""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, proof, ch, digest, cap = pc.late_case(CASE_B)
    L = m.proof_layout(circ.params)
    witness = int(proof[L.pow_witness])
    assert witness >= 2 * pc.BATCH and witness + pc.P < 1 << 64
    t, _ = pc.replay(m, oracle, circ.params, digest, pis, proof)
    assert pc.solves(oracle, t, witness, pc.LATE_BITS) and not pc.solves(oracle, t, witness - 1, pc.LATE_BITS)
    assert pc.B_LATER_SOLUTION > witness and pc.solves(oracle, t, pc.B_LATER_SOLUTION, pc.LATE_BITS)

    def with_witness(w):
        bad = proof.copy()
        bad[L.pow_witness] = np.uint64(w)
        return bad
    cases = [("clean", proof), ("witness_minus_1", with_witness(witness - 1)), ("witness_plus_p", with_witness(witness + pc.P)),
             ("later_solution", with_witness(pc.B_LATER_SOLUTION))]
    ov = oracle_lib.OracleCircuit.verifier_only(oracle, circ, digest, cap)
    want = [ov.verify(pr, pis) for _, pr in cases]
    ov.close()
    proofs = np.ascontiguousarray(np.stack([pr for _, pr in cases]), dtype=np.uint64)
    pis_all = np.repeat(pis[None, :], len(cases), axis=0)
    return circ, digest, cap, [l for l, _ in cases], proofs, pis_all, np.array(want, dtype=np.int32)


def test_host_verifier_at_the_witness_word(witness_word_cases):
    """lcp2_verify on the CPU: a non-solution is refused at the proof-of-work check, a witness word >= p at the canonical-words check,
    and a later solution passes the proof-of-work check - the verifier evaluates a predicate on the witness, it does not ask for the
    minimum.  (Acceptance of a whole proof under a later solution is not tested: the query section would have to be answered again for
    the indices that witness leads to, and the oracle has no entry point that proves with a given witness.)"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = witness_word_cases
    assert list(want[:3]) == [0, pc.POW_CHECK, pc.CANON_CHECK] and want[3] > pc.POW_CHECK, list(zip(labels, want))
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    got = [_verdict(m, vd, pr, pi) for pr, pi in zip(proofs, pis)]
    assert got == list(want), list(zip(labels, got, want))
    vd.close()


@gpu
def test_batch_verifier_at_the_witness_word(gpu_ctx, late, witness_word_cases):
    """lcp2_verify_batch over the same four proofs, from a host list and from a device buffer, transcript on the host and on the
    device (k_verify_transcript, head_pow_fails): the oracle's verdicts, element for element; the prover's own handle agrees"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = witness_word_cases
    assert (late["first"][CASE_B] == proofs[0]).all()
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    dev = gpu_ctx.buffer_alloc(proofs.size)
    try:
        gpu_ctx.buffer_write(dev, proofs)
        for head in ("host", "device"):
            for handle in (vd, late["data"]):
                from_host = gpu_ctx.verify_batch(handle, proofs, pis, head=head)
                assert list(from_host) == list(want), (head, list(zip(labels, from_host, want)))
                from_device = gpu_ctx.verify_batch(handle, dev, pis, mem=m.binding.MEM_DEVICE, count=len(labels), head=head)
                assert list(from_device) == list(want), (head, list(zip(labels, from_device, want)))
    finally:
        gpu_ctx.buffer_free(dev)
    vd.close()
