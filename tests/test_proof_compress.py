"""lcp2_verify_batch_compressed on the GPU: k_compress_scatter and k_decompress_paths in front of the kernels of lcp2_verify_batch.
Proofs come from the oracle prover on the CPU (compress_cases.py); the expected verdict of every compressed proof is lcp2_verify's
for lcp2_proof_decompress of it, and check 1 where decompression refuses.  Shapes: 2^3 rows at rate 3 / cap 1 (the smallest circuit
the case helpers make: 64 leaves for 28 queries, and the seed is chosen so that duplicates and level-0 siblings occur), 2^5 rows under
the standard config, 2^6 rows at rate 8 / cap 0 / 10 queries."""
import concurrent.futures
import ctypes

import numpy as np
import pytest

import compress_cases as cc

pytestmark = pytest.mark.gpu
OK, E_INVALID, E_VERIFY = 0, -1, -7
HEADS = ("host", "device")
WANT_CLASSES = {"tiny": {"a", "b", "c_mid", "c_last"}, "synthetic_5": {"a", "c_mid", "c_last", "d"}, "shrink_2": {"c_mid", "c_last"}}
SCRATCH_BYTES = 64 << 20   # LCP2_COMPRESSED_SCRATCH_BYTES (include/lcp2.h)


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def handles(m, shape):
    circ, digest, cap, proof, pis, x = cc.proved(shape)
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    return vd, proof, pis, x, vd.compress(proof, pis)


def expected(m, vd, comps, pis):
    """lcp2_verify of lcp2_proof_decompress of every compressed proof, 1 where decompression refuses (threads: ctypes drops the GIL)"""
    def one(comp):
        try:
            full = vd.decompress(comp, pis)
        except m.Lcp2Error as e:
            assert e.status == E_INVALID
            return 1
        try:
            vd.verify(full, pis)
        except m.ProofRejected as e:
            return e.check
        return 0
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        return np.array(list(pool.map(one, comps)), dtype=np.int32)


def test_the_shapes_hold_every_class_between_them():
    """asserted from the derived indices: which of the classes a to d the proofs of each shape contain; across the file all occur"""
    import eth_lc_plonky2_amd as m
    seen = set()
    for shape in cc.SHAPES:
        circ, digest, cap, proof, pis, x = cc.proved(shape)
        got = cc.classes(circ.params, x)
        assert got >= WANT_CLASSES[shape], (shape, sorted(got))
        seen |= got
    assert seen >= {"a", "b", "c_mid", "c_last", "d"}


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_round_trip_and_batches_of_1_and_5(gpu_ctx, shape):
    """compress -> decompress gives the proof back word for word; verify_batch_compressed accepts a batch of 1 and of 5 under both
    heads, from host memory and from a device buffer; count 0 returns OK and writes nothing"""
    import eth_lc_plonky2_amd as m
    vd, proof, pis, x, comp = handles(m, shape)
    assert cc.classes(vd.circ.params, x) >= WANT_CLASSES[shape]
    assert comp.size < proof.size and (vd.decompress(comp, pis) == proof).all()
    for head in HEADS:
        assert list(vd.verify_batch_compressed([comp], [pis], head=head, ctx=gpu_ctx)) == [0]
        assert list(vd.verify_batch_compressed([comp] * 5, [pis] * 5, head=head, ctx=gpu_ctx)) == [0] * 5
    five, offsets = np.concatenate([comp] * 5), np.arange(6, dtype=np.uint64) * np.uint64(comp.size)
    dev = gpu_ctx.buffer_alloc(five.size)
    try:
        gpu_ctx.buffer_write(dev, five)
        for head in HEADS:
            assert list(vd.verify_batch_compressed(dev, [pis] * 5, head=head, ctx=gpu_ctx, offsets=offsets, mem=m.binding.MEM_DEVICE)) == [0] * 5
    finally:
        gpu_ctx.buffer_free(dev)
    checks = np.full(2, -9, dtype=np.int32)
    lib = m.load_library()
    assert lib.lcp2_verify_batch_compressed(gpu_ctx.handle, vd.handle, vp(five), vp(offsets), 0, 0, vp(pis), pis.size, vp(checks), 0) == OK
    assert lib.lcp2_verify_batch_compressed(gpu_ctx.handle, vd.handle, vp(five), vp(offsets), 2, 0, vp(pis), pis.size + 1, vp(checks), 0) == E_INVALID
    assert lib.lcp2_verify_batch_compressed(gpu_ctx.handle, vd.handle, vp(five), vp(offsets), 2, 0, vp(pis), pis.size, vp(checks), 7) == E_INVALID
    down = np.ascontiguousarray(offsets[::-1])
    assert lib.lcp2_verify_batch_compressed(gpu_ctx.handle, vd.handle, vp(five), vp(down), 2, 0, vp(pis), pis.size, vp(checks), 0) == E_INVALID
    assert (checks == -9).all()
    vd.close()


def test_one_more_proof_than_a_chunk_holds(gpu_ctx):
    """the scratch proofs of a chunk take at most LCP2_COMPRESSED_SCRATCH_BYTES: one proof more than that, the last one and the one
    on the chunk boundary tampered, gets per-proof verdicts under both heads"""
    import eth_lc_plonky2_amd as m
    vd, proof, pis, x, comp = handles(m, "tiny")
    chunk = min(4096, SCRATCH_BYTES // (8 * proof.size))
    count = chunk + 1
    assert 1 < chunk < 4096
    bad = comp.copy()
    bad[comp.size - 3] ^= np.uint64(1)
    code = int(expected(m, vd, [bad], pis)[0])
    assert code >= 4
    comps = [comp] * count
    comps[chunk - 1] = comps[chunk] = bad
    want = np.zeros(count, dtype=np.int32)
    want[chunk - 1] = want[chunk] = code
    for head in HEADS:
        got = vd.verify_batch_compressed(comps, np.repeat(pis[None, :], count, axis=0), head=head, ctx=gpu_ctx)
        assert (got == want).all(), (head, np.nonzero(got != want)[0][:8])
    vd.close()


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_one_word_tamper_sweep_under_both_heads(gpu_ctx, shape):
    """every word of one compressed proof changed in a copy of its own: under both heads each verdict equals lcp2_verify of the
    lcp2_proof_decompress result (check 1 where that refuses), and no tampered proof is accepted"""
    import eth_lc_plonky2_amd as m
    vd, proof, pis, x, comp = handles(m, shape)
    n = comp.size
    values = comp + np.uint64(1)
    values[values == np.uint64(m.GOLDILOCKS_P)] = 0

    def tampered(i):
        c = comp.copy()
        c[i] = values[i]
        return c
    want = expected(m, vd, (tampered(i) for i in range(n)), pis)
    assert (want != 0).all() and set(want) >= {2, 4}, sorted(set(want))
    print("%s: %d words, verdicts %s" % (shape, n, {int(k): int((want == k).sum()) for k in sorted(set(want))}))
    piece = 2048
    for head in HEADS:
        for at in range(0, n, piece):
            k = min(piece, n - at)
            batch = np.repeat(comp[None, :], k, axis=0)
            batch[np.arange(k), at + np.arange(k)] = values[at:at + k]
            offsets = np.arange(k + 1, dtype=np.uint64) * np.uint64(n)
            got = vd.verify_batch_compressed(batch.ravel(), np.repeat(pis[None, :], k, axis=0), head=head, ctx=gpu_ctx, offsets=offsets)
            wrong = np.nonzero(got != want[at:at + k])[0]
            assert not wrong.size, (head, [(at + int(i), int(got[i]), int(want[at + i])) for i in wrong[:8]])
    vd.close()


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_mixed_batch_gets_per_proof_verdicts(gpu_ctx, shape):
    """good proofs between tampered, truncated, extended, empty and non-canonical ones, of different lengths in one call"""
    import eth_lc_plonky2_amd as m
    vd, proof, pis, x, comp = handles(m, shape)
    L = m.proof_layout(vd.circ.params)
    outside = L.queries + L.total - L.final_poly

    def changed(pos, value=None):
        c = comp.copy()
        c[pos] = np.uint64((int(c[pos]) + 1) % m.GOLDILOCKS_P) if value is None else np.uint64(value)
        return c
    cases = [comp, changed(0), comp, changed(outside + 1), changed(comp.size - 1), comp[:-1], np.concatenate([comp, comp[:1]]), comp[:outside],
             comp[:outside - 1], comp[:0], changed(outside + 2, m.GOLDILOCKS_P), changed(comp.size - 2, 2 ** 64 - 1), changed(L.queries + 1), comp]
    want = expected(m, vd, cases, pis)
    assert [int(w) for w in want[[0, 2, 13]]] == [0, 0, 0] and (np.delete(want, [0, 2, 13]) != 0).all()
    assert list(want[5:12]) == [1] * 7  # wrong lengths and words >= p: the encoding
    for head in HEADS:
        got = vd.verify_batch_compressed(cases, np.repeat(pis[None, :], len(cases), axis=0), head=head, ctx=gpu_ctx)
        assert list(got) == list(want), head
    vd.close()


def test_compress_refuses_a_flipped_duplicate_sibling():
    """(host only) one flipped duplicate sibling: LCP2_E_VERIFY, and out is untouched"""
    import eth_lc_plonky2_amd as m
    vd, proof, pis, x, comp = handles(m, "tiny")
    L = m.proof_layout(vd.circ.params)
    dup = next(q for q in range(len(x)) if x[q] in x[:q])
    bad = proof.copy()
    bad[L.queries + dup * L.query_words + L.q_init_off[1] + L.q_init_cols[1] + 5] ^= np.uint64(1)
    out, words = np.full(proof.size, 7, dtype=np.uint64), ctypes.c_size_t(99)
    rc = m.load_library().lcp2_proof_compress(vd.handle, vp(bad), bad.size, vp(pis), pis.size, vp(out), out.size, ctypes.byref(words))
    assert rc == E_VERIFY and (out == 7).all() and words.value == 99
    vd.close()
