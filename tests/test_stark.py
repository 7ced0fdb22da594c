"""lcp2_stark_prove on the GPU: for the three sample AIRs the device proof equals the model's proof word for word (the prover is
deterministic: smallest proof-of-work witness), lcp2_stark_verify and the model's verifier accept it with the transcript the prover
left, a host and a device trace and non-canonical trace words give the same proof, planted violations are located, and refused
descriptions are refused on the host before anything is launched."""
import ctypes

import numpy as np
import pytest

import stark_cases as sc
from rows_lib import DeviceMatrix

P = sc.P
pytestmark = pytest.mark.gpu


def prove(ctx, s, trace=None, pis=None, mem=0):
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = sc.lib_challenger()
    proof = ctx.stark_prove(s.desc, s.trace if trace is None else trace, s.pis if pis is None else pis, ch.state, mem=mem)
    return proof, fo.state_words(ch.state)


@pytest.mark.parametrize("name", list(sc.GPU_CASES))
def test_device_proof_equals_the_models(gpu_ctx, name):
    s = sc.case(name)
    want, after = sc.model_proof(name)
    proof, transcript = prove(gpu_ctx, s)
    assert proof.size == want.size
    assert [int(w) for w in proof] == [int(w) for w in want]
    assert transcript == after
    verdict, verifier_transcript = sc.lib_verdict(s, proof)
    assert verdict == 0 and verifier_transcript == transcript
    if s.log_n <= 5:   # (the model's verifier on the large case only repeats, slowly, what the equality above says)
        assert sc.model_verdict(s, proof) == (0, after)


@pytest.mark.parametrize("name", ["fib_n8", "cubic_n32", "poseidon_n8"])
def test_device_trace_and_noncanonical_words_give_the_same_proof(gpu_ctx, name):
    import eth_lc_plonky2_amd as m
    s = sc.case(name)
    want, after = sc.model_proof(name)
    dev = DeviceMatrix(gpu_ctx, s.trace)
    try:
        proof, transcript = prove(gpu_ctx, s, trace=dev.ptr, mem=m.MEM_DEVICE)
        assert (proof == want).all() and transcript == after
        assert (dev.read() == s.trace).all()   # the caller's trace is read, not written
    finally:
        dev.free()
    t = s.trace.copy()
    small = np.argwhere(t < np.uint64((1 << 64) - P))
    assert len(small)
    for c, r in small:
        t[c, r] += np.uint64(P)
    pis = s.pis.copy()
    pis[0] += np.uint64(P) if int(pis[0]) < (1 << 64) - P else np.uint64(0)
    proof, transcript = prove(gpu_ctx, s, trace=t, pis=pis)
    assert (proof == want).all() and transcript == after


@pytest.mark.parametrize("name", ["fib_n8", "cubic_n32", "poseidon_n32", "fib_crosses_workgroup"])
def test_planted_violations_are_located(gpu_ctx, name):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    s = sc.case(name)
    n = 1 << s.log_n
    want, after = sc.model_proof(name)

    def violation(trace, pis=None):
        ch = sc.lib_challenger()
        before = bytes(ch.state)
        with pytest.raises(m.Lcp2Error) as e:
            gpu_ctx.stark_prove(s.desc, trace, s.pis if pis is None else pis, ch.state)
        assert e.value.status == -5 and bytes(ch.state) == before and "violated on row" in str(e.value)
        v = e.value.violation
        got = (v.kind, v.constraint, v.row)
        assert got == stark.check_trace(s.air, trace, s.pis if pis is None else pis)
        return got

    t = s.trace.copy()
    t[0, 0] = (int(t[0, 0]) + 1) % P
    assert violation(t) == (0, 0, 0)
    pis = s.pis.copy()
    pis[-1] = (int(pis[-1]) + 1) % P
    assert violation(s.trace, pis)[::2] == (2, n - 1)
    # two violations: the earlier row wins, whichever lane finds it; the later one sits in the last workgroup
    early, late = n // 2 - 1, n - 2
    t = s.trace.copy()
    t[s.air.width - 1, late] ^= np.uint64(1)
    t[0, early] ^= np.uint64(1)
    assert violation(t)[::2] == (1, early - 1)
    # after a refusal the same context proves a good trace
    proof, transcript = prove(gpu_ctx, s)
    assert (proof == want).all() and transcript == after


def test_refused_descriptions_name_their_reason(gpu_ctx):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    s = sc.case("cubic_n8")

    def refused(desc, trace=s.trace, words=None):
        ch = sc.lib_challenger()
        before = bytes(ch.state)
        with pytest.raises(m.Lcp2Error) as e:
            if words is None:
                gpu_ctx.stark_prove(desc, trace, s.pis, ch.state)
            else:
                proof = np.zeros(words, dtype=np.uint64)
                gpu_ctx._check(gpu_ctx.lib.lcp2_stark_prove(gpu_ctx.handle, ctypes.byref(desc), trace.ctypes.data, 0, s.pis.ctypes.data, ctypes.byref(ch.state),
                                                             proof.ctypes.data, words, None))
        assert e.value.status == -1 and bytes(ch.state) == before
        return str(e.value)

    def with_air(change, q=s.q):
        air = stark.cubic_air()
        change(air)
        return stark.pack_stark_desc(air, s.cfg, s.log_n, q, s.challenges)

    def set_word(air, pc, words):
        air.code[2 * pc:2 * pc + 2] = words

    trans = stark.cubic_air().programs[1][0]
    assert "constraint degree above" in refused(with_air(lambda a: None, q=1))
    assert "quotient_degree_bits exceeds rate_bits" in refused(with_air(lambda a: None, q=4))
    assert "operand out of range" in refused(with_air(lambda a: set_word(a, trans, stark.insn(stark.OP_MUL, 0, (stark.CONST, 0), (stark.WIRE, 0)))))
    assert "operand out of range" in refused(with_air(lambda a: set_word(a, trans, stark.insn(stark.OP_MUL, 0, (stark.WIRE, 6), (stark.WIRE, 0)))))
    assert "first_row: instruction 0: operand out of range" in refused(with_air(lambda a: set_word(a, 0, stark.insn(stark.OP_SUB, 0, (stark.WIRE, 0), (stark.PI, 3)))))
    assert "proof_words is not lcp2_stark_proof_words" in refused(s.desc, words=m.stark_proof_words(s.desc) - 1)
    # and the context still proves
    want, after = sc.model_proof("cubic_n8")
    proof, transcript = prove(gpu_ctx, s)
    assert (proof == want).all() and transcript == after
