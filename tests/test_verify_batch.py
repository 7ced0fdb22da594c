"""lcp2_verify_batch on the GPU: data.verify for a batch of proofs of one circuit, check 1 by k_verify_canon, checks 4 to 7 by
k_verify_paths and k_verify_fri.  Proofs come from the oracle prover on the CPU and the expected code of every case is orc_verify's
(verify_batch_cases.py), which lcp2_verify names too.  The sweeps change one word per proof across whole sections of the layout -
k_verify_paths is GPU-only code, the emulation walks a path with one lane - and are large enough to take the chunk loop of
verify_batch.hip past its first chunk, from device memory and from host memory."""
import ctypes
import re

import numpy as np
import pytest

import verify_batch_cases as vc

pytestmark = pytest.mark.gpu
OK, E_INVALID, E_VERIFY = 0, -1, -7


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def raw_call(m, ctx, data, proofs, proof_words, count, mem, pis, npi, checks):
    return m.load_library().lcp2_verify_batch(ctx.handle, data.handle, proofs, proof_words, count, mem, vp(pis), npi, vp(checks) if checks is not None else None)


@pytest.mark.parametrize("name", vc.circuit_names())
def test_one_call_holds_every_case_of_a_circuit(gpu_ctx, name):
    """the clean proof and every tampered copy in ONE call: the verdict array equals the oracle's codes element for element and the
    return value is LCP2_E_VERIFY; the same batch copied to a device buffer gives the same verdicts"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.batch(name)
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    got = gpu_ctx.verify_batch(vd, proofs, pis)
    assert got.dtype == np.int32 and list(got) == list(want), [(l, int(g), int(w)) for l, g, w in zip(labels, got, want) if g != w]
    checks = np.full(len(want), -9, dtype=np.int32)
    assert raw_call(m, gpu_ctx, vd, vp(proofs), proofs.shape[1], proofs.shape[0], m.binding.MEM_HOST, pis, pis.shape[1], checks) == E_VERIFY
    assert list(checks) == list(want)
    dev = gpu_ctx.buffer_alloc(proofs.size)
    try:
        gpu_ctx.buffer_write(dev, proofs)
        on_device = gpu_ctx.verify_batch(vd, dev, pis, mem=m.binding.MEM_DEVICE, count=proofs.shape[0])
        assert list(on_device) == list(want)
        one = gpu_ctx.verify_batch(vd, dev, pis[:1], mem=m.binding.MEM_DEVICE, count=1)  # count 1: the clean proof
        assert list(one) == [0]
    finally:
        gpu_ctx.buffer_free(dev)
    clean = np.full(1, -9, dtype=np.int32)
    assert raw_call(m, gpu_ctx, vd, vp(proofs), proofs.shape[1], 1, m.binding.MEM_HOST, pis, pis.shape[1], clean) == OK and clean[0] == 0
    vd.close()


SWEEPS = ([("synthetic_5", s) for s in vc.STRATA] + [("synthetic_6", s) for s in vc.STRATA]
          + [("synthetic_9", "queries"), (vc.HIGH_RATE, "queries")])


def wrong(labels, got, want):
    """(how many verdicts differ, the first few as (label, got, want))"""
    at = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return len(at), [(labels[i], int(got[i]), int(want[i])) for i in at[:8]]


def from_device(m, ctx, vd, proofs, pis):
    dev = ctx.buffer_alloc(proofs.size)
    try:
        ctx.buffer_write(dev, proofs)
        return ctx.verify_batch(vd, dev, pis, mem=m.binding.MEM_DEVICE, count=proofs.shape[0])
    finally:
        ctx.buffer_free(dev)


def report(what, count, L, mem, want):
    bound = vc.HOST_CHUNK if mem == "host" else min(vc.HOST_CHUNK, vc.device_chunk_bound(L))
    print("%s: %d proofs from %s memory, at least %d chunks, codes %s" % (what, count, mem, -(-count // bound), sorted(set(int(w) for w in want))))


@pytest.mark.parametrize("name,stratum", SWEEPS)
def test_one_word_sweep_from_host_and_device_memory(gpu_ctx, name, stratum):
    """a stratum of one-word changes (verify_batch_cases.sweep) in one call from host memory and one from a device buffer: every word
    outside the queries, every word offset of a query with every word of the last query, or words >= p across the proof.  Both verdict
    arrays equal orc_verify's codes element for element and the call returns LCP2_E_VERIFY.  The head and queries strata of
    synthetic_6 are more device proofs than one chunk of verify_batch.hip stages."""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.sweep(name, stratum)
    L = m.proof_layout(circ.params)
    count = proofs.shape[0]
    if name == "synthetic_6" and stratum != "noncanonical":
        assert count > vc.device_chunk_bound(L)
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    checks = np.full(count, -9, dtype=np.int32)
    assert raw_call(m, gpu_ctx, vd, vp(proofs), proofs.shape[1], count, m.binding.MEM_HOST, pis, pis.shape[1], checks) == E_VERIFY
    assert not wrong(labels, checks, want)[0], wrong(labels, checks, want)
    on_device = from_device(m, gpu_ctx, vd, proofs, pis)
    assert not wrong(labels, on_device, want)[0], wrong(labels, on_device, want)
    report("%s %s" % (name, stratum), count, L, "host", want)
    report("%s %s" % (name, stratum), count, L, "device", want)
    vd.close()


def test_device_chunks_that_fail_at_their_head_precede_live_ones(gpu_ctx):
    """head + queries of synthetic_6 in one device buffer: the head stratum is more proofs than a chunk, so the first chunk holds
    only proofs the host stops at checks 2 and 3 and no kernel of checks 4 to 7 runs for it; the chunks behind it are live"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, hl, hp, hpis, hwant = vc.sweep("synthetic_6", "head")
    _, _, _, ql, qp, qpis, qwant = vc.sweep("synthetic_6", "queries")
    L = m.proof_layout(circ.params)
    bound = vc.device_chunk_bound(L)
    assert len(hwant) >= bound and ((hwant[:bound] == 2) | (hwant[:bound] == 3)).all() and (qwant >= 4).all()
    labels, want = hl + ql, np.concatenate([hwant, qwant])
    proofs, pis = np.concatenate([hp, qp]), np.concatenate([hpis, qpis])
    del hp, qp
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    got = from_device(m, gpu_ctx, vd, proofs, pis)
    assert not wrong(labels, got, want)[0], wrong(labels, got, want)
    report("synthetic_6 head + queries", len(want), L, "device", want)
    vd.close()


TILED = 2 * vc.HOST_CHUNK + 37
CLEAN_AT = (0, vc.HOST_CHUNK - 1, vc.HOST_CHUNK, TILED - 1)
CHANGED_PI_AT = vc.HOST_CHUNK + 1234   # in the second chunk


@pytest.fixture(scope="module")
def tiled(gpu_ctx):
    """(labels, verdicts, want) of ONE call from host memory over three chunks: the queries stratum of synthetic_5 repeated to
    2 * 4096 + 37 proofs, the clean proof at both ends and on both sides of the first chunk boundary, and one clean proof in the second
    chunk under public inputs of its own"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.sweep("synthetic_5", "queries")
    proof, pi = vc.clean("synthetic_5")
    bad_pi, bad_pi_code = vc.changed_public_input("synthetic_5")
    pick = np.arange(TILED) % len(want)
    labels, proofs, pis, want = [labels[i] for i in pick], proofs[pick], pis[pick], want[pick]
    for i in CLEAN_AT + (CHANGED_PI_AT,):
        labels[i], proofs[i], pis[i], want[i] = "clean", proof, pi, 0
    labels[CHANGED_PI_AT], pis[CHANGED_PI_AT], want[CHANGED_PI_AT] = "public_input", bad_pi, bad_pi_code
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    got = gpu_ctx.verify_batch(vd, proofs, pis)
    report("synthetic_5 queries, tiled", TILED, m.proof_layout(circ.params), "host", want)
    vd.close()
    return labels, got, want


def test_host_batch_of_three_chunks(tiled):
    """more host proofs than two chunks of 4096, the last chunk partial: every verdict is the oracle's, and exactly the four clean
    proofs - first, last, and the two at the first chunk boundary - are accepted"""
    labels, got, want = tiled
    assert len(got) == TILED > 2 * vc.HOST_CHUNK
    assert not wrong(labels, got, want)[0], wrong(labels, got, want)
    assert all(got[i] == 0 for i in CLEAN_AT) and list(np.nonzero(got == 0)[0]) == list(CLEAN_AT)


def test_public_inputs_of_a_proof_in_a_later_chunk(tiled):
    """the one proof of the second chunk whose public inputs differ gets the oracle's code for that pair (its words are the clean
    proof's), and the proofs beside it, under the circuit's public inputs, keep theirs"""
    labels, got, want = tiled
    i = CHANGED_PI_AT
    assert vc.HOST_CHUNK < i < 2 * vc.HOST_CHUNK and labels[i] == "public_input" and got[i] == want[i] != 0
    assert got[i - 1] == want[i - 1] >= 4 and got[i + 1] == want[i + 1] >= 4


def test_prover_handle_and_verifier_only_handle_agree(gpu_ctx):
    """the prover's handle and a verifier-only handle (which has no context: the call names one) give the same verdicts; a proof made
    by CircuitData.prove on the GPU is accepted from a device buffer and rejected after a one-word change written with buffer_write"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.batch("synthetic_6")
    data = m.CircuitData.build(gpu_ctx, circ)
    vd = m.CircuitData.verifier_only(circ, *data.digest())
    assert list(gpu_ctx.verify_batch(data, proofs, pis)) == list(gpu_ctx.verify_batch(vd, proofs, pis)) == list(want)
    _, wires, pi = vc.make_circuit(m, "synthetic_6")
    proof = data.prove(wires, pi)
    dev = gpu_ctx.buffer_alloc(proof.size)
    try:
        gpu_ctx.buffer_write(dev, proof)
        assert list(gpu_ctx.verify_batch(data, dev, pi, mem=m.binding.MEM_DEVICE, count=1)) == [0]
        L = m.proof_layout(circ.params)
        pos = L.queries + 2 * L.query_words + L.q_init_off[1] + 9
        word = np.array([(int(proof[pos]) + 1) % m.GOLDILOCKS_P], dtype=np.uint64)
        gpu_ctx.buffer_write(dev + 8 * pos, word)
        bad = proof.copy()
        bad[pos] = word[0]
        with pytest.raises(m.ProofRejected) as e:
            data.verify(bad, pi)
        assert list(gpu_ctx.verify_batch(vd, dev, pi, mem=m.binding.MEM_DEVICE, count=1)) == [e.value.check] == [4]
    finally:
        gpu_ctx.buffer_free(dev)
    data.close()
    vd.close()


def test_batch_of_64_with_one_tampered_copy(gpu_ctx):
    """64 copies of the 2^9-row proof, copy 37 tampered in a FRI layer: only failed_checks[37] is non-zero; count 0 returns OK and writes nothing"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.batch("synthetic_9")
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    tampered = labels.index("fri_eval_layer_0")
    many = np.ascontiguousarray(np.repeat(proofs[:1], 64, axis=0))
    many[37] = proofs[tampered]
    many_pis = np.ascontiguousarray(np.repeat(pis[:1], 64, axis=0))
    got = gpu_ctx.verify_batch(vd, many, many_pis)
    expect = np.zeros(64, dtype=np.int32)
    expect[37] = want[tampered]
    assert want[tampered] != 0 and list(got) == list(expect)
    checks = np.full(4, -9, dtype=np.int32)
    assert raw_call(m, gpu_ctx, vd, vp(many), many.shape[1], 0, m.binding.MEM_HOST, many_pis, many_pis.shape[1], checks) == OK
    assert (checks == -9).all()
    assert gpu_ctx.verify_batch(vd, many[:0], many_pis[:0]).size == 0
    vd.close()


def test_refusals_leave_the_verdicts_untouched(gpu_ctx):
    """a proof length or a public-input count that is not the circuit's, and a null failed_checks, are LCP2_E_INVALID before anything is read"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.batch("synthetic_5")
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    words, npi, host = proofs.shape[1], pis.shape[1], m.binding.MEM_HOST
    checks = np.full(2, -9, dtype=np.int32)
    for w, n in ((words - 1, npi), (words + 1, npi), (words, npi - 1), (words, npi + 1)):
        assert raw_call(m, gpu_ctx, vd, vp(proofs), w, 2, host, pis, n, checks) == E_INVALID
        assert (checks == -9).all()
    assert raw_call(m, gpu_ctx, vd, vp(proofs), words, 2, host, pis, npi, None) == E_INVALID
    assert raw_call(m, gpu_ctx, vd, None, words, 2, host, pis, npi, checks) == E_INVALID and (checks == -9).all()
    assert raw_call(m, gpu_ctx, vd, vp(proofs), words, 2, host, pis, npi, checks) == E_VERIFY and list(checks) == list(want[:2])
    vd.close()


def test_lch_verify_batch_on_a_light_client_session(gpu_ctx):
    """lch_verify_batch on the session's context: two good proofs and one altered give [0, 0, k], k the check lch_verify's rejection names"""
    import eth_lc_plonky2_amd as m
    prev, cur = m.light_client.reference_updates()
    step = m.light_client.LightClientStep(gpu_ctx, prev, cur)
    proof, pis = step.prove()
    bad = proof.copy()
    bad[len(bad) // 2] ^= np.uint64(1)
    with pytest.raises(m.ProofRejected) as e:
        step.verify(bad, pis)
    k = int(re.search(r"check (\d)", str(e.value.check)).group(1))
    got = step.verify_batch(np.stack([proof, proof, bad]), np.stack([pis, pis, pis]))
    assert k != 0 and list(got) == [0, 0, k]
    assert list(step.verify_batch(np.stack([proof, proof]), np.stack([pis, pis]))) == [0, 0]
    step.close()
