"""lcp2_verify_batch_ex with LCP2_VERIFY_HEAD_DEVICE on the GPU: checks 2 and 3 by k_verify_transcript, k_verify_identity and
k_verify_head_finish, whose challenge blocks the query kernels then read.  Every expected verdict is orc_verify's code
(verify_batch_cases.py, verify_head_cases.py), and every batch also goes through the host head, which must give the same array."""
import ctypes

import numpy as np
import pytest

import verify_batch_cases as vc
import verify_head_cases as hc

pytestmark = pytest.mark.gpu
OK, E_INVALID, E_VERIFY = 0, -1, -7
HEAD_HOST, HEAD_DEVICE = 0, 1


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def raw_call(m, ctx, data, proofs, proof_words, count, mem, pis, npi, checks, flags):
    return m.load_library().lcp2_verify_batch_ex(ctx.handle, data.handle, proofs, proof_words, count, mem, vp(pis), npi,
                                                 vp(checks) if checks is not None else None, flags)


def wrong(labels, got, want):
    at = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return len(at), [(labels[i], int(got[i]), int(want[i])) for i in at[:8]]


def device_head_chunk(m, circ):
    """verify_batch.hip, device head: proofs per chunk"""
    per_proof = 8 * circ.num_public_inputs + 8 + 4 * circ.params.num_query_rounds
    return min(vc.HOST_CHUNK, (vc.PIN_BYTES - 256) // per_proof)


def both_heads_both_memories(m, ctx, data, labels, proofs, pis, want):
    """head="device" from host and from device memory gives `want`, and head="host" gives the identical arrays"""
    count = proofs.shape[0]
    checks = np.full(count, -9, dtype=np.int32)
    rc = raw_call(m, ctx, data, vp(proofs), proofs.shape[1], count, m.binding.MEM_HOST, pis, pis.shape[1], checks, HEAD_DEVICE)
    assert rc == (E_VERIFY if (want != 0).any() else OK)
    assert not wrong(labels, checks, want)[0], wrong(labels, checks, want)
    dev = ctx.buffer_alloc(proofs.size)
    try:
        ctx.buffer_write(dev, proofs)
        on_device = ctx.verify_batch(data, dev, pis, mem=m.binding.MEM_DEVICE, count=count, head="device")
        host_head = ctx.verify_batch(data, dev, pis, mem=m.binding.MEM_DEVICE, count=count, head="host")
    finally:
        ctx.buffer_free(dev)
    assert on_device.dtype == np.int32 and not wrong(labels, on_device, want)[0], wrong(labels, on_device, want)
    assert (host_head == on_device).all() and (ctx.verify_batch(data, proofs, pis, head="host") == checks).all()


def run(m, ctx, cases):
    circ, digest, cap, labels, proofs, pis, want = cases
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    try:
        both_heads_both_memories(m, ctx, vd, labels, proofs, pis, want)
    finally:
        vd.close()
    print("%d proofs, %d chunk(s), codes %s" % (len(want), -(-len(want) // device_head_chunk(m, circ)), sorted(set(int(w) for w in want))))


@pytest.mark.parametrize("name", hc.circuit_names())
def test_device_head_holds_every_case_of_a_circuit(gpu_ctx, name):
    """the clean proof and every tampered copy of the circuit in one call: ragged public-input counts and the mixed gate set included"""
    import eth_lc_plonky2_amd as m
    run(m, gpu_ctx, hc.batch(name))


@pytest.mark.parametrize("name,stratum", [("synthetic_5", "head"), (vc.HIGH_RATE, "head"), ("synthetic_5", "noncanonical"), ("synthetic_6", "queries")])
def test_device_head_over_a_one_word_sweep(gpu_ctx, name, stratum):
    """head: every word outside the queries moves the transcript; noncanonical: check 1 wins over whatever the head kernels compute;
    queries: the query kernels eat blocks the head kernels made"""
    import eth_lc_plonky2_amd as m
    run(m, gpu_ctx, vc.sweep(name, stratum))


@pytest.mark.parametrize("name", hc.IDENTITY_CIRCUITS)
def test_device_head_over_the_identity_stratum(gpu_ctx, name):
    """honest proofs of work over unsatisfied witnesses: one per gate, a broken copy, alpha = 0 - check 3 from k_verify_head_finish"""
    import eth_lc_plonky2_amd as m
    cases = hc.identity_stratum(name)
    assert (cases[6][1:] == 3).all()
    run(m, gpu_ctx, cases)


def test_interleaved_verdicts_over_three_chunks(gpu_ctx):
    """ONE call over 4096 + 4096 + 64 proofs of synthetic_6, from host and from device memory: the first chunk holds only proofs that
    die in the head (checks 1, 2 and 3), the second interleaves clean / 1 / 2 / 3 / 4-7 proofs with a clean proof at both ends and a
    clean proof under a changed public input inside, the third is short with a clean proof at both ends"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, hl, hp, hpis, hwant = vc.sweep("synthetic_6", "head")
    _, _, _, ql, qp, _, qwant = vc.sweep("synthetic_6", "queries")
    _, _, _, nl, npf, _, nwant = vc.sweep("synthetic_6", "noncanonical")
    _, _, _, il, ip, _, iwant = hc.identity_stratum("synthetic_6")
    proof, pi = vc.clean("synthetic_6")
    bad_pi, bad_pi_code = vc.changed_public_input("synthetic_6")
    C = device_head_chunk(m, circ)
    assert C == vc.HOST_CHUNK and (hwant != 0).all() and (hwant < 4).all() and (qwant >= 4).all()
    dead = [(hl[i % len(hl)], hp[i % len(hl)], hwant[i % len(hl)]) for i in range(C - 64)] + [(nl[i], npf[i], nwant[i]) for i in range(32)]
    dead += [(il[1 + i % (len(il) - 1)], ip[1 + i % (len(il) - 1)], 3) for i in range(32)]
    kinds = [("clean", proof, 0)], list(zip(nl, npf, nwant)), list(zip(hl, hp, hwant)), list(zip(il[1:], ip[1:], iwant[1:])), list(zip(ql, qp, qwant))
    mixed = [kinds[i % 5][(i // 5) % len(kinds[i % 5])] for i in range(C)]
    tail = [kinds[(i + 2) % 5][(i // 5) % len(kinds[(i + 2) % 5])] for i in range(64)]
    for chunk in (mixed, tail):
        chunk[0] = chunk[-1] = ("clean", proof, 0)
    everything = dead + mixed + tail
    labels = [c[0] for c in everything]
    proofs = np.ascontiguousarray(np.stack([c[1] for c in everything]))
    want = np.array([c[2] for c in everything], dtype=np.int32)
    pis = np.repeat(np.ascontiguousarray(pi)[None, :], len(want), axis=0)
    at = C + 1235  # a clean proof (1235 % 5 == 0) in the second chunk
    assert want[at] == 0
    labels[at], pis[at], want[at] = "public_input", bad_pi, bad_pi_code
    assert len(want) == 2 * C + 64 and (want[:C] != 0).all() and set(want[C:]) >= {0, 1, 2, 3, 4}
    run(m, gpu_ctx, (circ, digest, cap, labels, proofs, pis, want))


def test_prover_handle_and_verifier_only_handle_agree(gpu_ctx):
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = hc.batch("synthetic_6")
    data = m.CircuitData.build(gpu_ctx, circ)
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    a = gpu_ctx.verify_batch(data, proofs, pis, head="device")
    b = gpu_ctx.verify_batch(vd, proofs, pis, head="device")
    assert list(a) == list(b) == list(want)
    data.close()
    vd.close()


def test_refusals_leave_the_verdicts_untouched(gpu_ctx):
    """unknown flags, a proof length or public-input count that is not the circuit's: LCP2_E_INVALID and nothing written;
    count = 0: LCP2_OK and nothing written"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = hc.batch("synthetic_5")
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    words, npi, H = proofs.shape[1], pis.shape[1], m.binding.MEM_HOST
    checks = np.full(len(want), -9, dtype=np.int32)
    for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
        assert raw_call(m, gpu_ctx, vd, vp(proofs), words, len(want), H, pis, npi, checks, flags) == E_INVALID
    for w, k in ((words - 1, npi), (words + 1, npi), (words, npi + 1)):
        assert raw_call(m, gpu_ctx, vd, vp(proofs), w, 1, H, pis, k, checks, HEAD_DEVICE) == E_INVALID
    for flags in (HEAD_HOST, HEAD_DEVICE):
        assert raw_call(m, gpu_ctx, vd, vp(proofs), words, 0, H, pis, npi, checks, flags) == OK
        assert raw_call(m, gpu_ctx, vd, None, words, 0, H, pis, npi, None, flags) == OK
    assert (checks == -9).all()
    with pytest.raises(m.Lcp2Error):
        gpu_ctx.verify_batch(vd, proofs, pis, head="auto")
    assert raw_call(m, gpu_ctx, vd, vp(proofs), words, 1, H, pis, npi, checks, HEAD_DEVICE) == OK and checks[0] == 0 and (checks[1:] == -9).all()
    vd.close()
