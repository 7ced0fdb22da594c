"""Shared by test_verify_head_emu.py (CPU) and test_verify_head.py (GPU): what verify_batch_cases.py cannot reach.  A changed head
word changes the transcript, so its sweeps end at check 2; here are proofs with an honest proof of work that fail at check 3 (the
identity stratum: the oracle prover proves an unsatisfied witness), a circuit with the reference's gate mix, circuits whose
public-input count is ragged, and the scan that shows every opcode and operand kind of the gate-program format is executed."""
import functools

import numpy as np

import oracle_lib
import verify_batch_cases as vc
import witness_check_cases as wc

MIXED = "mixed_9"                 # synthetic_circuit(extra=ReferenceMix) at 2^9 rows
RAGGED = ("pi13_6", "pi20_6")     # 13 public inputs: neither 0 mod 8 nor below 8; 20: above 16 (three absorptions, the last ragged)
IDENTITY_CIRCUITS = ("synthetic_6", MIXED)


def circuit_names():
    return vc.circuit_names() + [MIXED] + list(RAGGED)


def gate_bit_ops(asm):
    """A gate of this module, for the two opcodes no gate of the reference mix executes: wire 5 = wire 2 + wire 3 * wire 4 (MULADD)
    and wire 2 = wire 0 + wire 1 - 2 wire 0 wire 1 (XOR), listed last to first.  Degree 2."""
    from eth_lc_plonky2_amd.circuit import W
    acc = asm.add(W(2), asm.imm(0))
    asm.muladd(acc, W(3), W(4))
    asm.emit(asm.sub(W(5), acc))
    asm.emit(asm.sub(W(2), asm.xor(W(0), W(1))))


def mixed_extra():
    """the reference's gate mix (u32_gates.ReferenceMix) with BitOpsGate rows on every 16th row"""
    import eth_lc_plonky2_amd as m
    P = m.GOLDILOCKS_P

    class Mix(m.u32_gates.ReferenceMix):
        def gateset(self):
            C, U = m.circuit, m.u32_gates   # ReferenceMix.gateset() with one more entry, sorted by (degree, name)
            return C.GateSet([
                ("NoopGate", 0, C.gate_noop), ("ConstantGate", 1, C.gate_constant), ("PublicInputGate", 1, C.gate_public_input),
                ("BaseSumGate", 2, C.gate_base_sum(C.BASE_SUM_LIMBS)), ("BitOpsGate", 2, gate_bit_ops), ("ArithmeticGate", 3, C.gate_arithmetic),
                ("ComparisonGate", 4, U.gate_comparison), ("U32AddManyGate", 4, U.gate_u32_add_many), ("U32ArithmeticGate", 4, U.gate_u32_arithmetic),
                ("U32RangeCheckGate", 4, U.gate_u32_range_check), ("U32SubtractionGate", 4, U.gate_u32_subtraction), ("PoseidonGate", 7, C.gate_poseidon),
            ], native=self.native)

        def assign(self, gate_of_row, G, rng):
            rows = np.arange(gate_of_row.size)
            gate_of_row[(gate_of_row == G["ArithmeticGate"]) & (rows % 16 == 12)] = G["BitOpsGate"]
            super().assign(gate_of_row, G, rng)

        def fill(self, wires, gate_of_row, G, rng, link2):
            super().fill(wires, gate_of_row, G, rng, link2)
            for r in np.nonzero(gate_of_row == G["BitOpsGate"])[0]:
                a, b, x, y = (int(wires[j, r]) for j in (0, 1, 3, 4))
                w2 = (a + b - 2 * a * b) % P
                wires[2, r], wires[5, r] = np.uint64(w2), np.uint64((w2 + x * y) % P)

    return Mix()


@functools.lru_cache(maxsize=None)
def make_circuit(name):
    """(Circuit, wires, public inputs) of a name of circuit_names()"""
    import eth_lc_plonky2_amd as m
    if name == MIXED:
        extra = mixed_extra()
        return m.circuit.synthetic_circuit(m.standard_params(9, extra.gateset().num_selectors + 2), seed=9, extra=extra)
    if name in RAGGED:
        npi, d = int(name[2:4]), int(name.split("_")[1])
        return m.circuit.synthetic_circuit(m.standard_params(d, 4), seed=npi, npi=npi)
    return vc.make_circuit(m, name)


def executed_code(circ):
    """(opcodes, operand kinds) of the instructions inside some gate's program"""
    ops, kinds = set(), set()
    code = np.asarray(circ.gateset.code, dtype=np.uint32)
    for G in circ.gateset.gates:
        for pc in range(G.code_offset, G.code_offset + G.code_len):
            w0 = int(code[2 * pc])
            op = w0 & 0xF
            ops.add(op)
            if op == 9:          # PMDS: a window of registers and a block of immediates
                kinds |= {0, 3}
                continue
            kinds.add((w0 >> 16) & 0xF)
            if op not in (3, 6, 8):   # EMIT, EMITBOOL and SBOX have one operand
                kinds.add((w0 >> 20) & 0xF)
    return ops, kinds


def assert_format_is_covered():
    """across the circuits of the head tests every opcode 0..9 and every operand kind 0..4 is executed"""
    ops, kinds = set(), set()
    for name in ("synthetic_5", MIXED):
        o, k = executed_code(make_circuit(name)[0])
        ops |= o
        kinds |= k
    assert ops == set(range(10)) and kinds == set(range(5)), (sorted(ops), sorted(kinds))


@functools.lru_cache(maxsize=None)
def proved(name):
    """(circ, digest, cap, the oracle's proof, public inputs) of a circuit of this module"""
    circ, wires, pis = make_circuit(name)
    oc = oracle_lib.OracleCircuit(oracle_lib.load(), circ)
    proof = oc.prove(wires, pis)
    assert oc.verify(proof, pis) == 0
    digest, cap = oc.digest()
    oc.close()
    proof.setflags(write=False)
    return circ, digest, cap, proof, np.ascontiguousarray(pis, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def identity_stratum(name):
    """(circ, digest, cap, labels, proofs (k, proof_words), public inputs (k, npi), want (k,) int32): the clean proof (want 0), then
    proofs of unsatisfied witnesses - one broken cell in a row of each gate that has constraints, one broken cell of a copy cycle, one
    proof made under alpha = 0 - each of which orc_verify rejects with exactly 3 (a case it judges otherwise is dropped; at most one
    gate may end without a case).  Read-only."""
    circ, wires, pis = make_circuit(name)
    oc = oracle_lib.OracleCircuit(oracle_lib.load(), circ)
    clean = oc.prove(wires, pis)
    assert oc.verify(clean, pis) == 0
    digest, cap = oc.digest()
    cases, gates = [("clean", clean)], []
    for label, cells in wc.gate_cases(circ).items():
        if label not in circ.gateset.names:
            continue
        gates.append(label)
        cases.append((label, oc.try_prove(wc.corrupt(wires, cells), pis)))
    row, wire = wc.cycles(circ)[-1][0]
    cases.append(("copy", oc.try_prove(wc.corrupt(wires, [(wire, row)]), pis)))
    cases.append(("alpha_0", oc.prove_forced(wires, pis, alphas=[0] * circ.params.num_challenges)))
    kept, want = [cases[0]], [0]
    for label, (rc, proof) in cases[1:]:
        if rc == 0 and oc.verify(proof, pis) == 3:
            kept.append((label, proof))
            want.append(3)
    oc.close()
    labels = [l for l, _ in kept]
    assert len([g for g in gates if g not in labels]) <= 1, (name, gates, labels)
    assert "copy" in labels and "alpha_0" in labels, (name, labels)
    proofs = np.ascontiguousarray(np.stack([p for _, p in kept]), dtype=np.uint64)
    pis_all = np.repeat(np.ascontiguousarray(pis, dtype=np.uint64)[None, :], len(kept), axis=0)
    for a in (proofs, pis_all):
        a.setflags(write=False)
    return circ, digest, cap, labels, proofs, pis_all, np.array(want, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def small_batch(name):
    """(circ, digest, cap, labels, proofs, public inputs, want) of a circuit vc.batch() does not know (MIXED, RAGGED): the clean proof,
    a changed opening (the transcript moves: check 2), a changed query word, a word >= p, and a changed public input - the last one
    of them when there are more than 8, so that the ragged absorption is the one that differs; want is orc_verify's"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, proof, pis = proved(name)
    L = m.proof_layout(circ.params)
    bad_pis = pis.copy()
    bad_pis[-1] ^= np.uint64(4)
    noncanon = proof.copy()
    noncanon[L.op_wires + 1] = np.uint64(m.GOLDILOCKS_P)
    cases = [("clean", proof, pis), ("opening", vc.bump(m, proof, L.op_wires + 5), pis), ("query", vc.bump(m, proof, L.queries + 3), pis),
             ("noncanonical", noncanon, pis), ("public_input", proof, bad_pis)]
    ov = oracle_lib.OracleCircuit.verifier_only(oracle_lib.load(), circ, digest, cap)
    want = [ov.verify(pr, pi) for _, pr, pi in cases]
    ov.close()
    assert want[0] == 0 and all(w != 0 for w in want[1:]) and want[3] == 1, (name, want)
    proofs = np.ascontiguousarray(np.stack([c[1] for c in cases]), dtype=np.uint64)
    pis_all = np.ascontiguousarray(np.stack([c[2] for c in cases]), dtype=np.uint64)
    for a in (proofs, pis_all):
        a.setflags(write=False)
    return circ, digest, cap, [c[0] for c in cases], proofs, pis_all, np.array(want, dtype=np.int32)


def batch(name):
    """vc.batch for its circuits, small_batch for the ones of this module"""
    return small_batch(name) if name == MIXED or name in RAGGED else vc.batch(name)
