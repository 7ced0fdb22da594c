"""The two light native gates of K6, ArithmeticGate and BaseSumGate<2> (csrc/light_gates.hpp: one walk, each gate alone or both at once)
through whole circuits: the native forms against the interpreted programs, proof and quotient values word for word, in circuits that
have one of the gates, both, and a second BaseSumGate (so that one launch of k_q_light runs the pair and a single form); build()'s
check of the claims with both gates present; the limit the alpha-limb table puts on a claimed gate.  The shapes of the walk itself are
tests/test_generated_gates.py's, on the CPU."""
import numpy as np
import pytest

P = 0xFFFFFFFF00000001
E_INVALID = -1


def light_circuit(m, limbs=(), arithmetic=True, num_challenges=2, seed=5):
    """A satisfiable circuit of 2^5 rows: PublicInput, Constant, Noop, one BaseSumGate<2> per entry of `limbs` (three rows each), and
    ArithmeticGate { 20 } rows (or Noop rows instead); no copy constraints.  Returns (circuit, wires, public_inputs)."""
    from eth_lc_plonky2_amd import circuit as cm
    from eth_lc_plonky2_amd import gl_np as gl
    from eth_lc_plonky2_amd import poseidon_py as pos
    gates = [("NoopGate", 0, cm.gate_noop), ("ConstantGate", 1, cm.gate_constant), ("PublicInputGate", 1, cm.gate_public_input)]
    gates += [("BaseSumGate%03d" % l, 2, cm.gate_base_sum(l)) for l in sorted(limbs)]
    if arithmetic:
        gates.append(("ArithmeticGate", 3, cm.gate_arithmetic))
    gs = cm.GateSet(gates, max_degree=9)
    assert gs.num_selectors == 1
    params = m.standard_params(5, gs.num_selectors + 2)
    params.num_challenges = num_challenges
    rng = np.random.default_rng(seed)
    n, Wn, NR = 1 << params.degree_bits, params.num_wires, params.num_routed_wires
    G = {name: gs.index(name) for name in gs.names}
    gate_of_row = np.full(n, G["ArithmeticGate"] if arithmetic else G["NoopGate"], dtype=np.int64)
    gate_of_row[0] = G["PublicInputGate"]
    gate_of_row[1:3] = G["ConstantGate"]
    gate_of_row[n - 4:] = G["NoopGate"]
    wires = rng.integers(0, P, size=(Wn, n), dtype=np.uint64)
    c0, c1 = (rng.integers(0, P, size=n, dtype=np.uint64) for _ in range(2))
    wires[0, 1:3], wires[1, 1:3] = c0[1:3], c1[1:3]
    for k, l in enumerate(sorted(limbs)):
        for row in (3 + 3 * k, 4 + 3 * k, 5 + 3 * k):
            gate_of_row[row] = G["BaseSumGate%03d" % l]
            bits = [int(b) for b in rng.integers(0, 2, size=l)]
            wires[0, row] = np.uint64(sum(b << i for i, b in enumerate(bits)) % P)
            wires[1:1 + l, row] = np.array(bits, dtype=np.uint64)
    ar = np.nonzero(gate_of_row == G.get("ArithmeticGate", -1))[0]
    for k in range(cm.ARITH_OPS):
        x, y, z = wires[4 * k, ar], wires[4 * k + 1, ar], wires[4 * k + 2, ar]
        wires[4 * k + 3, ar] = gl.add(gl.mul(gl.mul(x, y), c0[ar]), gl.mul(z, c1[ar]))
    pis = rng.integers(0, P, size=2, dtype=np.uint64)
    wires[:4, 0] = np.array(pos.hash_no_pad(pis), dtype=np.uint64)
    k_is = gl.powers(7, NR)
    sig = cm.sigma_values(np.tile(np.arange(n), (NR, 1)), np.tile(np.arange(NR)[:, None], (1, n)), k_is, params.degree_bits)
    consts = np.concatenate([gs.selector_columns(gate_of_row), c0[None, :], c1[None, :]])
    return cm.Circuit(params, gs, np.concatenate([consts, sig]), k_is, len(pis)), wires, pis


def _native_gates(m, circ):
    return [g for g in circ.gateset.gates if g.flags & m.circuit.GATE_NATIVE_MASK]


def _proof_and_quotients(m, ctx, circ, wires, pis, alpha_sets):
    """the proof, and the quotient values [num_challenges][2^q n] under each forced set of alphas"""
    data = m.CircuitData.build(ctx, circ)
    try:
        proof = data.prove(wires, pis)
        data.verify(proof, pis)
        ch = data.last_challenges()
        CH = circ.params.num_challenges
        data.commit_wires(wires)
        data.perm_zs(ch["betas"][:CH], ch["gammas"][:CH])
        quotients = []
        for alphas in alpha_sets:
            data.quotient_values(np.array(alphas, dtype=np.uint64), m.binding.hash_no_pad(pis))
            ptr, words = data.quotient_buffer()
            quotients.append(ctx.buffer_read(ptr, words))
        return proof, quotients
    finally:
        data.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,limbs,arithmetic,num_challenges", [
    ("arithmetic_alone", (), True, 2), ("base_sum_63_alone", (63,), False, 2), ("base_sum_17_alone", (17,), False, 2),
    ("both", (63,), True, 2), ("both_one_challenge", (63,), True, 1), ("pair_and_a_single_base_sum", (17, 63), True, 2),
])
def test_native_light_gates_equal_their_interpreted_programs(gpu_ctx, name, limbs, arithmetic, num_challenges):
    """the same circuit with its LCP2_GATE_NATIVE_ARITHMETIC / _BASE_SUM2 claims and with the claims cleared: one proof, and one
    table of quotient values under random alphas and under alpha = 0 (the first constraint alone)"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = light_circuit(m, limbs, arithmetic, num_challenges, seed=50 + len(name))
    native = _native_gates(m, circ)
    assert len(native) == len(limbs) + arithmetic
    rng = np.random.default_rng(9)
    a = [int(v) for v in rng.integers(1, P, size=2, dtype=np.uint64)]
    alpha_sets = [a[:num_challenges], [0, a[0]][:num_challenges]]
    got = _proof_and_quotients(m, gpu_ctx, circ, wires, pis, alpha_sets)
    for g in native:
        g.flags &= ~m.circuit.GATE_NATIVE_MASK   # unclaimed: interpreted
    want = _proof_and_quotients(m, gpu_ctx, circ, wires, pis, alpha_sets)
    assert (got[0] == want[0]).all()
    for q_native, q_interpreted, alphas in zip(got[1], want[1], alpha_sets):
        assert q_native.size == num_challenges << (5 + 3) and (q_native == q_interpreted).all(), alphas


@pytest.mark.gpu
def test_claims_of_a_pair_are_checked_at_build(gpu_ctx):
    """with both gates in the circuit (the light list pairs them): one operand index off in the BaseSumGate program, then in the
    ArithmeticGate program, and build() refuses the claim; restored, it builds.  The single-gate claim checks alone refuse these
    programs too (they instantiate the same text), so this does not show that the pair's launch exists: what holds the pair
    instantiation to the programs is test_generated_gates.test_light_gate_walk_equals_the_programs_on_the_cpu."""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = light_circuit(m, (63,), True)
    gs = circ.gateset
    m.CircuitData.build(gpu_ctx, circ).close()
    bs = gs.gates[gs.index("BaseSumGate063")]
    pc_b = bs.code_offset + bs.code_len - 2      # SUB acc, acc, wire 0
    ar = gs.gates[gs.index("ArithmeticGate")]
    pc_a = ar.code_offset + 6 * 7 + 2            # operation 12 (the eighth from the top): MUL u, wire 50, const 1
    assert gs.code[2 * pc_b] & 0xF == m.circuit.OP_SUB and gs.code[2 * pc_b + 1] >> 16 == 0
    assert gs.code[2 * pc_a] & 0xF == m.circuit.OP_MUL and gs.code[2 * pc_a + 1] & 0xFFFF == 4 * 12 + 2
    for pc, bit in ((pc_b, 1 << 16), (pc_a, 1)):
        gs.code[2 * pc + 1] ^= np.uint32(bit)
        with pytest.raises(m.Lcp2Error) as e:
            m.CircuitData.build(gpu_ctx, circ)
        assert e.value.status == E_INVALID and "NATIVE" in str(e.value) and "does not compute what its program computes" in str(e.value)
        gs.code[2 * pc + 1] ^= np.uint32(bit)
    m.CircuitData.build(gpu_ctx, circ).close()


@pytest.mark.gpu
def test_claimed_gate_beyond_the_alpha_limb_table_is_refused(gpu_ctx):
    """BaseSumGate<2> { 128 } has 129 constraints, one more than the alpha power table weights (QUOTIENT_TERM_POWS): claimed native it
    is refused by name of the limit, before anything runs; unclaimed it is interpreted, builds and proves"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = light_circuit(m, (128,), True)
    bs = circ.gateset.gates[circ.gateset.index("BaseSumGate128")]
    assert bs.num_constraints == 129 and bs.flags & m.circuit.GATE_NATIVE_MASK == m.circuit.GATE_NATIVE_BASE_SUM2
    with pytest.raises(m.Lcp2Error) as e:
        m.CircuitData.build(gpu_ctx, circ)
    assert e.value.status == E_INVALID and "at most 128 constraints" in str(e.value)
    bs.flags &= ~m.circuit.GATE_NATIVE_MASK
    data = m.CircuitData.build(gpu_ctx, circ)
    data.verify(data.prove(wires, pis), pis)
    data.close()


def test_verifier_refuses_the_same_claim_without_a_device():
    """lcp2_verifier_create runs build()'s check of the programs: 129 constraints claimed LCP2_GATE_NATIVE_BASE_SUM2 are LCP2_E_INVALID,
    128 constraints (127 limbs) and the unclaimed gate are accepted; the circuits' witnesses satisfy the oracle's row check"""
    import eth_lc_plonky2_amd as m
    import oracle_lib
    L = oracle_lib.load()
    for limbs, ok in ((127, True), (128, False)):
        circ, wires, pis = light_circuit(m, (limbs, 17), True)
        oc = oracle_lib.OracleCircuit(L, circ)
        assert oc.check_witness(wires, pis)[0] == 0
        oc.close()
        digest, cap = np.zeros(4, np.uint64), np.zeros(4 << circ.params.cap_height, np.uint64)
        if ok:
            m.CircuitData.verifier_only(circ, digest, cap).close()
            continue
        with pytest.raises(m.Lcp2Error) as e:
            m.CircuitData.verifier_only(circ, digest, cap)
        assert e.value.status == E_INVALID
        circ.gateset.gates[circ.gateset.index("BaseSumGate128")].flags &= ~m.circuit.GATE_NATIVE_MASK
        m.CircuitData.verifier_only(circ, digest, cap).close()
