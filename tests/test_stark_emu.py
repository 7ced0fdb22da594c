"""The portable STARK text (csrc/stark.hpp) on the CPU, through tests/emu/emu_stark.cpp, against the model
(eth_lc_plonky2_amd.stark): the per-point quotient values and the verdicts of the witness check, the next-row leaf index, and
lcp2_stark_verify - host only, so tested here from the library itself and from the harness - on the model's proofs, on one-word
changes and on refused descriptions.  No GPU."""
import ctypes

import numpy as np
import pytest

import stark_cases as sc
from rows_lib import vp

P = sc.P
AIR_Q = {"fibonacci": 0, "cubic": 2, "poseidon_round": 3}   # the smallest q the AIR's degree admits


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def emu_quotient(s, lde, alphas):
    out = np.zeros((s.challenges, 1 << (s.log_n + s.q)), dtype=np.uint64)
    assert sc.emu().emu_stark_quotient(ctypes.byref(s.desc), vp(s.pis), vp(lde), vp(np.array(alphas, dtype=np.uint64)), vp(out)) == 0
    return out


def emu_check(s, trace, pis=None):
    import eth_lc_plonky2_amd as m
    v = m.StarkViolation()
    t = np.ascontiguousarray(trace, dtype=np.uint64)
    rc = sc.emu().emu_stark_check(ctypes.byref(s.desc), vp(np.ascontiguousarray(s.pis if pis is None else pis, dtype=np.uint64)), vp(t), ctypes.byref(v))
    assert rc in (0, 1)
    return (v.kind, v.constraint, v.row) if rc else None


@pytest.mark.parametrize("air_name", list(AIR_Q))
def test_quotient_values_and_check_verdicts_equal_the_model(air_name):
    """log_n 1 .. 6 (n = 2: the next row of row 1 is row 0, and the first and last filters sit on adjacent rows), rate_bits 1 .. 3,
    every q from the AIR's smallest up to rate_bits, 1, 2 and 4 challenges"""
    from eth_lc_plonky2_amd import stark
    rng = np.random.default_rng(3)
    shapes = 0
    for log_n in range(1, 7):
        for rate_bits in range(1, 4):
            for q in range(AIR_Q[air_name], rate_bits + 1):
                lde = leaves = None
                for challenges in (1, 2, 4):
                    s = sc.shape(air_name, log_n, rate_bits, q, challenges)
                    assert sc.emu().emu_stark_words(s.desc) == stark.layout(s.air, s.cfg, log_n, q, challenges).total == stark_words(s)
                    if lde is None:
                        cols = [stark.coset_values(stark.interpolate(s.trace[c]), log_n + rate_bits) for c in range(s.air.width)]
                        lde = np.array(cols, dtype=np.uint64)
                        leaves = [[col[i] for col in cols] for i in range(1 << (log_n + rate_bits))]
                        assert emu_check(s, s.trace) is None
                    alphas = [int(a) for a in rng.integers(1, P, challenges, dtype=np.uint64)]
                    want = stark.quotient_values(s.air, log_n, rate_bits, q, leaves, [int(v) for v in s.pis], alphas)
                    got = emu_quotient(s, lde, alphas)
                    assert [[int(v) for v in row] for row in got] == want, (log_n, rate_bits, q, challenges)
                    shapes += 1
    assert shapes >= 18
    # the quotient of a satisfying trace is a polynomial of degree < 2^q n - 1: the top coefficient of its interpolant is zero
    coeffs = stark.coset_interpolate(want[0], log_n + q)
    assert coeffs[-1] == 0


def stark_words(s):
    import eth_lc_plonky2_amd as m
    return m.stark_proof_words(s.desc)


def test_next_leaf_equals_the_formula_and_the_point_g_x():
    from eth_lc_plonky2_amd import fri_openings as fo
    for lgN in range(2, 10):
        for rate_bits in range(1, min(3, lgN - 1) + 1):
            N, g = 1 << lgN, fo.root_of_unity(lgN - rate_bits)
            xs = [fo.GENERATOR * pow(fo.root_of_unity(lgN), bitrev(i, lgN), P) % P for i in range(N)]
            at = {x: i for i, x in enumerate(xs)}
            for i in range(N):
                got = sc.emu().emu_stark_next_leaf(i, lgN, rate_bits)
                assert got == bitrev((bitrev(i, lgN) + (1 << rate_bits)) % N, lgN) == at[xs[i] * g % P]


@pytest.mark.parametrize("air_name", list(AIR_Q))
def test_check_locates_violations_like_the_model(air_name):
    from eth_lc_plonky2_amd import stark
    s = sc.shape(air_name, 4, 3, 3, 1)
    n = 1 << s.log_n
    rng = np.random.default_rng(8)

    def both(trace, pis=None):
        got = emu_check(s, trace, pis)
        assert got == stark.check_trace(s.air, trace, s.pis if pis is None else pis)
        return got

    # the trace breaks the transition across the wrap-around (row n - 1 -> row 0) like every trace of these AIRs: not enforced
    last, first = [int(v) for v in s.trace[:, n - 1]], [int(v) for v in s.trace[:, 0]]
    assert any(stark.emitted(s.air, 1, last, first, [int(v) for v in s.pis], stark.BASE))
    assert both(s.trace) is None
    # wrong only in row 0: a first-row constraint.  Only in row n - 1: with the transition into it kept, the last-row constraint
    t = s.trace.copy()
    t[0, 0] = (int(t[0, 0]) + 5) % P
    assert both(t) == (0, 0, 0)
    pis = s.pis.copy()
    pis[-1] = (int(pis[-1]) + 1) % P
    assert both(s.trace, pis)[::2] == (2, n - 1)
    # elsewhere: kind 1 and the smallest row, whatever else is wrong later; non-canonical words are reduced, not refused
    for _ in range(4):
        rows = sorted(int(r) for r in rng.choice(np.arange(2, n - 1), size=2, replace=False))
        t = s.trace.copy()
        for r in rows:
            t[int(rng.integers(0, s.air.width)), r] ^= np.uint64(1)
        assert both(t)[::2] == (1, rows[0] - 1)
    t = s.trace.copy()
    small = np.argwhere(t < np.uint64((1 << 64) - P))
    for c, r in small[:5]:
        t[c, r] += np.uint64(P)
    assert len(small) and both(t) is None


VERIFY_CASES = ["fib_n2", "fib_n8", "cubic_n2", "poseidon_n2"]


def verdicts(s, proof, pis=None):
    """(library, harness, model): the failed check, 0 if accepted"""
    lib, lib_after = sc.lib_verdict(s, proof, pis)
    rc, failed, emu_after = sc.emu_verdict(s, proof, pis)
    assert rc in (0, -7) and (rc == 0) == (failed == 0)
    model, model_after = sc.model_verdict(s, proof, pis)
    if lib == 0:
        assert lib_after == emu_after == model_after
    return lib, failed, model


@pytest.mark.parametrize("name", VERIFY_CASES)
def test_verifier_accepts_the_models_proofs(name):
    s = sc.case(name)
    proof, after = sc.model_proof(name)
    assert verdicts(s, proof) == (0, 0, 0)
    assert sc.lib_verdict(s, proof)[1] == after
    pis = s.pis.copy()
    pis[0] = (int(pis[0]) + 1) % P
    v = verdicts(s, proof, pis)
    assert v[0] == v[1] == v[2] != 0


@pytest.mark.parametrize("name", ["fib_n2", "cubic_n2"])   # no proof of work: a changed opening reaches the identity
def test_changed_words_fail_the_check_the_model_names(name):
    from eth_lc_plonky2_amd import stark
    s = sc.case(name)
    proof, _ = sc.model_proof(name)
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges)
    seen = {}
    for section, first, words in stark.sections(L):
        for w in sorted({first, first + words // 2, first + words - 1}) if words else ():
            bad = proof.copy()
            bad[w] = (int(bad[w]) + 1) % P
            v = verdicts(s, bad)
            assert v[0] == v[1] == v[2] != 0, (section, w, v)
            seen.setdefault(section, set()).add(v[0])
    # every opening - the trace at zeta, the quotient chunks, the trace at g zeta - enters the identity: check 9
    for w in (L.op_local, L.op_quotient, L.op_quotient + 2 * (s.challenges * L.Q) - 1, L.op_next + 1):
        bad = proof.copy()
        bad[w] = (int(bad[w]) + 1) % P
        assert verdicts(s, bad) == (9, 9, 9), w
    assert seen["openings"] == {9}
    # inside the FRI proof the opening layer's numbers come through
    assert seen["queries"] <= {3, 4, 5, 6} and seen["pow_witness"] <= {3, 4, 5, 6, 7}
    # a cap word that is not canonical: check 8, before anything else; a canonical change moves the transcript
    for w in (0, L.capw - 1, L.capw, 2 * L.capw - 1):
        bad = proof.copy()
        bad[w] = int(bad[w]) + P if int(bad[w]) < (1 << 64) - P else P
        assert verdicts(s, bad) == (8, 8, 8)
    # a non-canonical word behind the caps is the opening layer's check 1
    bad = proof.copy()
    bad[L.openings] = (1 << 64) - 1
    assert verdicts(s, bad) == (1, 1, 1)


def test_proof_of_work_failure_comes_before_the_identity():
    """the order 8, then the opening layer's 1 and 2, then 9: with 3 proof-of-work bits some changed opening fails check 2"""
    from eth_lc_plonky2_amd import stark
    s = sc.case("fib_n8")
    proof, _ = sc.model_proof("fib_n8")
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges)
    seen = set()
    for w in range(L.op_local, L.op_local + 12):
        bad = proof.copy()
        bad[w] = (int(bad[w]) + 1) % P
        v = verdicts(s, bad)
        assert v[0] == v[1] == v[2] and v[0] in (2, 9)
        seen.add(v[0])
    assert 2 in seen


def test_refusals():
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    s = sc.case("cubic_n2")
    proof, _ = sc.model_proof("cubic_n2")
    assert m.stark_proof_words(s.desc) == proof.size

    def refused(desc, pr=proof):
        assert m.stark_proof_words(desc) == 0 or pr is not proof
        ch = sc.lib_challenger()
        before = bytes(ch.state)
        with pytest.raises(m.Lcp2Error) as e:
            m.stark_verify(desc, s.pis, ch.state, pr)
        assert e.value.status == -1 and bytes(ch.state) == before   # the transcript was not touched
        assert sc.emu_verdict(s, pr, desc=desc)[0] == -1
        return True

    def with_air(change, q=s.q, cfg=s.cfg, log_n=s.log_n, challenges=s.challenges):
        air = stark.cubic_air()
        change(air)
        return stark.pack_stark_desc(air, cfg, log_n, q, challenges)

    def set_word(air, pc, words):
        air.code[2 * pc:2 * pc + 2] = words

    trans = stark.cubic_air().programs[1][0]
    # a wrong proof_words (the description is fine)
    assert refused(s.desc, proof[:-1]) and refused(s.desc, np.concatenate([proof, proof[:1]]))
    # a CONST operand; WIRE idx >= 2 width; PI idx >= num_public_inputs; an immediate and a register past their tables; a bad op
    assert refused(with_air(lambda a: set_word(a, trans, stark.insn(stark.OP_MUL, 0, (stark.CONST, 0), (stark.WIRE, 0)))))
    assert refused(with_air(lambda a: set_word(a, trans, stark.insn(stark.OP_MUL, 0, (stark.WIRE, 6), (stark.WIRE, 0)))))
    assert m.stark_proof_words(with_air(lambda a: set_word(a, trans, stark.insn(stark.OP_MUL, 0, (stark.WIRE, 5), (stark.WIRE, 0))))) == proof.size
    assert refused(with_air(lambda a: set_word(a, 0, stark.insn(stark.OP_SUB, 0, (stark.WIRE, 0), (stark.PI, 3)))))
    assert refused(with_air(lambda a: set_word(a, trans + 2, stark.insn(stark.OP_MULADD, 1, (stark.WIRE, 1), (stark.IMM, 2)))))
    assert refused(with_air(lambda a: set_word(a, trans, stark.insn(stark.OP_MUL, 3, (stark.WIRE, 0), (stark.WIRE, 0)))))
    assert refused(with_air(lambda a: set_word(a, trans, [10, 0])))
    # a degree above what q allows (degree 3 needs Q >= 3), q above rate_bits, and the shapes around them
    assert refused(with_air(lambda a: None, q=1)) and refused(with_air(lambda a: None, q=0))
    assert m.stark_proof_words(with_air(lambda a: None, q=3)) not in (0, proof.size)
    assert refused(with_air(lambda a: None, q=4))
    # a constraint count that is not the program's, a program past the code, challenges, width, registers
    def count(a):
        a.programs[1] = (a.programs[1][0], a.programs[1][1], a.programs[1][2] + 1)
    def past(a):
        a.programs[2] = (a.programs[2][0], a.programs[2][1] + 1, a.programs[2][2])
    assert refused(with_air(count)) and refused(with_air(past))
    assert refused(with_air(lambda a: None, challenges=0)) and refused(with_air(lambda a: None, challenges=5))
    for field, value in (("width", 0), ("width", 32768), ("num_regs", 65), ("log_n", 0)):
        d = with_air(lambda a: None)
        setattr(d, field, value)
        assert refused(d)
    # what the opening layer refuses of the config
    assert refused(with_air(lambda a: None, cfg=m.fri_config(1, 3, 5, 0, 2, 1, 1, schedule=[1])))
    assert refused(with_air(lambda a: None, cfg=m.fri_config(1, 3, 2, 0, 65, 1, 1, schedule=[1])))
    assert refused(with_air(lambda a: None, cfg=m.fri_config(1, 3, 2, 0, 2, 1, 1, schedule=[2])))
    # null arguments
    lib = m.load_library()
    ch = sc.lib_challenger()
    assert lib.lcp2_stark_proof_words(None) == 0
    assert lib.lcp2_stark_verify(None, vp(s.pis), ctypes.byref(ch.state), vp(np.ascontiguousarray(proof)), proof.size, None) == -1
    assert lib.lcp2_stark_verify(ctypes.byref(s.desc), vp(s.pis), None, vp(np.ascontiguousarray(proof)), proof.size, None) == -1
    assert lib.lcp2_stark_verify(ctypes.byref(s.desc), vp(s.pis), ctypes.byref(ch.state), None, proof.size, None) == -1
    assert lib.lcp2_stark_verify(ctypes.byref(s.desc), None, ctypes.byref(ch.state), vp(np.ascontiguousarray(proof)), proof.size, None) == -1
    assert lib.lcp2_stark_verify(ctypes.byref(s.desc), vp(s.pis), ctypes.byref(ch.state), vp(np.ascontiguousarray(proof)), proof.size, None) == 0
    # lcp2_stark_prove without a context
    assert lib.lcp2_stark_prove(None, ctypes.byref(s.desc), vp(s.trace), 0, vp(s.pis), ctypes.byref(ch.state), vp(np.zeros(proof.size, dtype=np.uint64)), proof.size, None) == -1
