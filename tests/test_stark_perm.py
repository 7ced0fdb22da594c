"""lcp2_stark_prove_perm on the GPU: for the three sample AIRs with a permutation argument the device proof equals the model's proof
word for word (the prover is deterministic: smallest proof-of-work witness) with the same transcript, lcp2_stark_verify_perm accepts
it, a host and a device trace and non-canonical trace words give the same proof, a broken permutation is located as kind 3 with the
transcript untouched, refused descriptions are refused on the host before anything is launched, perm=None is lcp2_stark_prove, and
the running product crosses the blocks of the scan at 2^11 rows."""
import ctypes

import numpy as np
import pytest

import stark_cases as sc
import stark_perm_cases as pc
from rows_lib import DeviceMatrix

P = sc.P
pytestmark = pytest.mark.gpu


def prove(ctx, s, trace=None, pis=None, mem=0):
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = sc.lib_challenger()
    proof = ctx.stark_prove(s.desc, s.trace if trace is None else trace, s.pis if pis is None else pis, ch.state, mem=mem, perm=s.sperm)
    return proof, fo.state_words(ch.state)


@pytest.mark.parametrize("name", list(pc.GPU_CASES))
def test_device_proof_equals_the_models(gpu_ctx, name):
    s = pc.case(name)
    want, after = pc.model_proof(name)
    proof, transcript = prove(gpu_ctx, s)
    assert proof.size == want.size
    assert [int(w) for w in proof] == [int(w) for w in want]
    assert transcript == after
    verdict, verifier_transcript = pc.lib_verdict(s, proof)
    assert verdict == 0 and verifier_transcript == transcript
    if s.log_n <= 5:   # (the model's verifier on the large case only repeats, slowly, what the equality above says)
        assert pc.model_verdict(s, proof) == (0, after)


@pytest.mark.parametrize("name", ["range_n8", "tuples_n32"])
def test_device_trace_and_noncanonical_words_give_the_same_proof(gpu_ctx, name):
    import eth_lc_plonky2_amd as m
    s = pc.case(name)
    want, after = pc.model_proof(name)
    dev = DeviceMatrix(gpu_ctx, s.trace)
    try:
        proof, transcript = prove(gpu_ctx, s, trace=dev.ptr, mem=m.MEM_DEVICE)
        assert (proof == want).all() and transcript == after
        assert (dev.read() == s.trace).all()   # the caller's trace is read, not written
    finally:
        dev.free()
    if name == "range_n8":   # (its values are small: every cell has a second representation)
        t = s.trace + np.uint64(P)
        assert (t >= np.uint64(P)).all()
        proof, transcript = prove(gpu_ctx, s, trace=t)
        assert (proof == want).all() and transcript == after


@pytest.mark.parametrize("name", ["shuffle_n2", "tuples_n32", "range_crosses_workgroup"])
def test_broken_permutation_is_located_as_kind_3(gpu_ctx, name):
    import eth_lc_plonky2_amd as m
    s = pc.case(name)
    n = 1 << s.log_n
    want, after = pc.model_proof(name)

    def violation(trace):
        ch = sc.lib_challenger()
        before = bytes(ch.state)
        with pytest.raises(m.Lcp2Error) as e:
            gpu_ctx.stark_prove(s.desc, trace, s.pis, ch.state, perm=s.sperm)
        assert e.value.status == -5 and bytes(ch.state) == before and "violated on row" in str(e.value)
        v = e.value.violation
        return v.kind, v.constraint, v.row

    # an rhs cell of the last pair: the last Z column stays open; with one of the first pair as well: Z 0, the smallest.  (In the
    # range check the two values swapped keep the AIR's own constraints: b stays sorted only if a, column 0, is what changes.)
    l, r = s.perm.pairs[-1][-1]
    col = l if name == "range_crosses_workgroup" else r
    t = s.trace.copy()
    t[col, n // 2] = (int(t[col, n // 2]) + (1 << 40)) % P
    assert violation(t) == (3, s.perm.num_z(s.challenges) - 1, n - 1)
    t[s.perm.pairs[0][0][0], n - 1] ^= np.uint64(1)
    assert violation(t) == (3, 0, n - 1)
    # after the refusal the same context proves a good trace
    proof, transcript = prove(gpu_ctx, s)
    assert (proof == want).all() and transcript == after


def test_refused_descriptions_name_their_reason(gpu_ctx):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    s = pc.case("tuples_n32")

    def refused(perm=None, desc=None, words=None):
        sperm = stark.pack_stark_perm(perm) if perm is not None else s.sperm
        desc = desc or s.desc
        ch = sc.lib_challenger()
        before = bytes(ch.state)
        with pytest.raises(m.Lcp2Error) as e:
            if words is None:
                gpu_ctx.stark_prove(desc, s.trace, s.pis, ch.state, perm=sperm)
            else:
                proof = np.zeros(words, dtype=np.uint64)
                gpu_ctx._check(gpu_ctx.lib.lcp2_stark_prove_perm(gpu_ctx.handle, ctypes.byref(desc), ctypes.byref(sperm), s.trace.ctypes.data, 0, s.pis.ctypes.data,
                                                                  ctypes.byref(ch.state), proof.ctypes.data, words, None))
        assert e.value.status == -1 and bytes(ch.state) == before
        return str(e.value)

    Pm, one = stark.Permutation, [(0, 6)]
    assert "num_pairs above 64" in refused(Pm([one] * 65, 1))
    assert "pair 1 has no columns" in refused(Pm([one, []], 1))
    assert "num_column_pairs above 4096" in refused(Pm([one * 4097], 1))
    assert "column not below width" in refused(Pm([[(0, 12)]], 1))
    assert "batch_size outside" in refused(Pm([one], 5)) and "batch_size outside" in refused(Pm([one], 0))
    assert "more than 64 Z columns" in refused(Pm([one] * 33, 1))
    assert "quotient_degree_bits exceeds rate_bits" in refused(desc=stark.pack_stark_desc(s.air, s.cfg, s.log_n, 4, 2))
    assert "proof_words is not lcp2_stark_proof_words" in refused(words=m.stark_proof_words(s.desc, s.sperm) - 1)
    assert "proof_words is not lcp2_stark_proof_words" in refused(words=m.stark_proof_words(s.desc))   # the count without the argument
    # and the context still proves
    want, after = pc.model_proof("tuples_n32")
    proof, transcript = prove(gpu_ctx, s)
    assert (proof == want).all() and transcript == after


@pytest.mark.parametrize("name", ["fib_n8", "cubic_n2"])
def test_without_a_permutation_the_call_is_stark_prove(gpu_ctx, name):
    from eth_lc_plonky2_amd import fri_openings as fo
    from eth_lc_plonky2_amd import stark
    s = sc.case(name)
    want, after = sc.model_proof(name)
    for sperm in (None, stark.pack_stark_perm(stark.Permutation([], 1))):
        ch = sc.lib_challenger()
        if sperm is None:   # a null pointer, through the entry point itself
            proof = np.zeros(want.size, dtype=np.uint64)
            gpu_ctx._check(gpu_ctx.lib.lcp2_stark_prove_perm(gpu_ctx.handle, ctypes.byref(s.desc), None, s.trace.ctypes.data, 0, s.pis.ctypes.data,
                                                              ctypes.byref(ch.state), proof.ctypes.data, proof.size, None))
        else:
            proof = gpu_ctx.stark_prove(s.desc, s.trace, s.pis, ch.state, perm=sperm)
        assert (proof == want).all() and fo.state_words(ch.state) == after
    ch = sc.lib_challenger()
    assert (gpu_ctx.stark_prove(s.desc, s.trace, s.pis, ch.state) == want).all()


def test_running_product_across_the_blocks_of_the_scan(gpu_ctx):
    """2^11 rows are two 1024-element blocks of the scan.  The model's prover would take too long on a whole proof of that size:
    the library's verifier accepts the device proof, and the Z cap inside it is the cap of lcp2_commit_values over the model's Z
    columns, the challenges re-derived from the proof's trace cap."""
    from eth_lc_plonky2_amd import stark
    s = pc.shape("shuffle", 11, 1, 0, 1, 1, cap_height=1, pow_bits=0, queries=2, schedule=[3, 3, 3])
    proof, transcript = prove(gpu_ctx, s)
    assert pc.lib_verdict(s, proof) == (0, transcript)
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges, perm=s.perm)
    ch = sc.model_challenger()
    ch.observe([int(v) for v in s.pis])
    ch.observe([int(w) for w in proof[:L.capw]])
    zs = stark.perm_z_columns(s.trace, s.perm, stark.draw_challenge_sets(s.perm, s.challenges, ch))
    assert zs.shape == (1, 1 << 11) and int(zs[0, 0]) == 1 and len({int(v) for v in zs[0]}) > 2000
    oracle = gpu_ctx.commit_values(zs, rate_bits=s.cfg.rate_bits, cap_height=s.cfg.cap_height)
    try:
        assert [int(w) for w in np.asarray(oracle.cap).ravel()] == [int(w) for w in proof[L.z_cap:L.z_cap + L.capw]]
    finally:
        oracle.close()
    # one changed cell far from the end: the product does not close
    import eth_lc_plonky2_amd as m
    t = s.trace.copy()
    t[1, 1500] ^= np.uint64(1)
    with pytest.raises(m.Lcp2Error) as e:
        gpu_ctx.stark_prove(s.desc, t, s.pis, sc.lib_challenger().state, perm=s.sperm)
    assert e.value.status == -5 and (e.value.violation.kind, e.value.violation.constraint, e.value.violation.row) == (3, 0, (1 << 11) - 1)
