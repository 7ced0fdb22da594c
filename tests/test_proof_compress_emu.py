"""Compressed proofs without a GPU: csrc/proof_compress.hpp compiled for the CPU (tests/emu/emu_compress.cpp) against the numpy model
(eth-lc-plonky2_amd/proof_compress.py), word for word, on forced index sets over real Merkle trees and on oracle proofs; the host entry
points lcp2_proof_compress / lcp2_proof_decompress against both."""
import ctypes

import numpy as np
import pytest

import compress_cases as cc
from rows_lib import vp

E_INVALID, E_VERIFY = -1, -7


@pytest.mark.parametrize("name", cc.FORCED)
def test_emulation_equals_the_model_on_forced_index_sets(name):
    """classes a to g of the format on index sets chosen by hand: the emulated compression equals the model's word for word, its
    length is compressed_words of both, and both reconstructions give the proof back"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import proof_compress as pc
    params, x = cc.forced_cases(m)[name]
    proof = cc.forced_proof(m, params, x, seed=len(name))
    comp, model = cc.emu_compress(params, x, proof), pc.compress_model(params, proof, x)
    assert comp.size == model.size == pc.compressed_words(params, x) and (comp == model).all()
    assert comp.size == cc.emu().emu_compressed_words(ctypes.byref(params), vp(cc.x64(x)))
    rc, back = cc.emu_decompress(params, x, comp)
    assert rc == 0 and (back[:proof.size] == proof).all()
    assert (pc.decompress_model(params, model, x) == proof).all()
    if name.startswith("d_") or name == "c_meet_in_the_cap":
        assert comp.size == proof.size  # no merge at all: nothing is dropped
    else:
        assert comp.size < proof.size


def test_forced_cases_hold_the_classes_their_names_say():
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import proof_compress as pc
    cases = cc.forced_cases(m)
    for name, cls in (("a_same_index", "a"), ("b_level0_siblings", "b"), ("c_middle_level", "c_mid"), ("c_last_level_below_cap", "c_last"), ("d_no_merge", "d")):
        assert cls in cc.classes(*cases[name]), name
    assert cc.classes(*cases["d_no_merge"]) == {"d"}
    assert all(nsib == 0 for _, _, nsib, _ in pc.layout(cases["e_no_siblings"][0]).trees)
    assert pc.layout(cases["e_layer_at_its_cap"][0]).trees[4][2] == 0
    assert cases["f_64_queries"][0].num_query_rounds == cases["f_64_distinct_wide"][0].num_query_rounds == 64
    assert [t[1] for t in pc.layout(cases["g_noop_leaves_arity_2"][0]).trees[4:]] == [4, 4, 4]


def test_plan_equals_the_two_predicates():
    """pc_plan derives both predicates from one pass over the indices; the model states them as the format does"""
    from eth_lc_plonky2_amd import proof_compress as pc
    rng = np.random.default_rng(5)
    out = np.zeros(2, dtype=np.uint32)
    for R, bits, nsib, shift in ((1, 3, 3, 0), (5, 2, 2, 0), (28, 4, 3, 0), (28, 7, 7, 2), (64, 5, 4, 1), (64, 12, 12, 0), (9, 32, 32, 0)):
        x = [int(v) for v in rng.integers(0, 1 << bits, size=R)]
        idx = [v >> shift for v in x]
        for q in range(R):
            cc.emu().emu_compress_plan(vp(cc.x64(x)), R, q, shift, nsib, vp(out))
            assert (out[0] > 0) == pc.leaf_stored(idx, q)
            assert [(int(out[1]) >> l) & 1 for l in range(nsib)] == [int(pc.sibling_stored(idx, q, l)) for l in range(nsib)], (R, bits, q)


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_oracle_proofs_round_trip_through_model_emulation_and_library(shape):
    """decompress_model(compress_model(P)) == P on the oracle's proofs, compressed_words equals the length produced, and
    lcp2_proof_compress / lcp2_proof_decompress give the same words as the model and the emulation"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import proof_compress as pc
    circ, digest, cap, proof, pis, x = cc.proved(shape)
    p = circ.params
    model = pc.compress_model(p, proof, x)
    assert model.size == pc.compressed_words(p, x) < proof.size
    assert (pc.decompress_model(p, model, x) == proof).all()
    assert (cc.emu_compress(p, x, proof) == model).all()
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    comp = vd.compress(proof, pis)
    assert comp.size == model.size and (comp == model).all()
    assert (vd.decompress(comp, pis) == proof).all()
    assert cc.indices_of(m, circ, digest, comp, pis, compressed=True) == x
    assert m.load_library().lcp2_proof_compressed_words_max(ctypes.byref(p)) == proof.size
    vd.close()


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_every_other_word_count_is_refused(shape):
    """every truncated word count and some extended ones: the emulation and lcp2_proof_decompress refuse with LCP2_E_INVALID, the
    output untouched, and the buffer handed over holds exactly that many words"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, proof, pis, x = cc.proved(shape)
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    lib = m.load_library()
    comp = vd.compress(proof, pis)
    L = m.proof_layout(circ.params)
    outside = L.queries + L.total - L.final_poly
    counts = list(range(0, outside + 2)) + list(range(outside + 2, comp.size, 37)) + [comp.size - 1, comp.size + 1, comp.size + 4, proof.size, 2 * comp.size]
    for words in counts:
        if words == comp.size:
            continue
        rc, back = cc.emu_decompress(circ.params, x, comp, words)
        assert rc == E_INVALID and (back == np.uint64(0xABABABABABABABAB)).all(), words
    out = np.full(proof.size, 7, dtype=np.uint64)
    for words in (0, 1, outside - 1, outside, comp.size - 1, comp.size + 1):
        exact = np.ascontiguousarray(np.concatenate([comp, np.zeros(1, dtype=np.uint64)])[:words]) if words else np.zeros(1, dtype=np.uint64)
        assert lib.lcp2_proof_decompress(vd.handle, vp(exact), words, vp(pis), pis.size, vp(out), out.size) == E_INVALID, words
        assert (out == 7).all()
    assert lib.lcp2_proof_decompress(vd.handle, vp(comp), comp.size, vp(pis), pis.size, vp(out), out.size - 1) == E_INVALID and (out == 7).all()
    vd.close()


def test_compress_refuses_what_it_could_not_give_back():
    """a flipped duplicate sibling, a flipped duplicate leaf word and a flipped sibling that the other paths recompute: LCP2_E_VERIFY,
    out and *out_words untouched; a stored sibling flipped in every query through its node comes back word for word where the change
    is consistent, and is refused where an ancestor of the node is another path's dropped sibling"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import proof_compress as pc
    circ, digest, cap, proof, pis, x = cc.proved("tiny")
    vd = m.CircuitData.verifier_only(circ, digest, cap)
    lib, L = m.load_library(), pc.layout(circ.params)
    off, leaf_len, nsib, shift = L.trees[1]
    dup = next(q for q in range(len(x)) if x[q] in x[:q])
    on_sibling = next((q, l) for q in range(len(x)) for l in range(nsib) if any((o >> l) == (x[q] >> l) ^ 1 for o in x))
    spots = {"duplicate sibling": L.queries + dup * L.query_words + off + leaf_len + 4 * (nsib - 1) + 2,
             "duplicate leaf": L.queries + dup * L.query_words + off + 3,
             "recomputed sibling": L.queries + on_sibling[0] * L.query_words + off + leaf_len + 4 * on_sibling[1]}
    for label, pos in spots.items():
        bad = proof.copy()
        bad[pos] ^= np.uint64(1)
        out, words = np.full(proof.size, 7, dtype=np.uint64), ctypes.c_size_t(99)
        assert lib.lcp2_proof_compress(vd.handle, vp(bad), bad.size, vp(pis), pis.size, vp(out), out.size, ctypes.byref(words)) == E_VERIFY, label
        assert (out == 7).all() and words.value == 99, label
    first = x.index(x[dup])
    stored = next(l for l in range(nsib) if pc.sibling_stored(x, first, l))
    bad = proof.copy()
    bad[L.queries + first * L.query_words + off + leaf_len + 4 * stored] ^= np.uint64(1)
    with pytest.raises(m.Lcp2Error) as e:  # the duplicate no longer equals its first occurrence
        vd.compress(bad, pis)
    assert e.value.status == E_VERIFY
    # The same change in EVERY query through that node.  The node's ancestors change with it; where one of them is the dropped sibling
    # of another path the proof still could not be given back (E_VERIFY), and where none is, the changed proof is consistent - a
    # wrong proof, but one that comes back word for word.  Both kinds are looked for over all trees of all three shapes.
    given_back = refused = 0
    for shape in cc.SHAPES:
        circ2, digest2, cap2, proof2, pis2, x2 = cc.proved(shape)
        vd2, L2 = m.CircuitData.verifier_only(circ2, digest2, cap2), pc.layout(circ2.params)
        for off2, leaf_len2, nsib2, shift2 in L2.trees:
            idx = [v >> shift2 for v in x2]
            done = set()
            for q in range(len(idx)):
                for l in range(nsib2):
                    if not pc.sibling_stored(idx, q, l) or (given_back and refused) or len(done) >= 2:
                        continue
                    feeds = any((o >> up) == (idx[q] >> up) ^ 1 for up in range(l + 1, nsib2) for o in idx)
                    if feeds in done:
                        continue
                    done.add(feeds)
                    bad = proof2.copy()
                    for o in range(len(idx)):
                        if idx[o] >> l == idx[q] >> l:
                            bad[L2.queries + o * L2.query_words + off2 + leaf_len2 + 4 * l] ^= np.uint64(1)
                    if feeds:
                        with pytest.raises(m.Lcp2Error) as e:
                            vd2.compress(bad, pis2)
                        assert e.value.status == E_VERIFY
                        refused += 1
                    else:
                        assert (vd2.decompress(vd2.compress(bad, pis2), pis2) == bad).all() and not (bad == proof2).all()
                        given_back += 1
        vd2.close()
    assert given_back and refused
    out, words = np.full(8, 7, dtype=np.uint64), ctypes.c_size_t(0)  # too small an output: the count, nothing written
    assert lib.lcp2_proof_compress(vd.handle, vp(proof), proof.size, vp(pis), pis.size, vp(out), out.size, ctypes.byref(words)) == E_INVALID
    assert (out == 7).all() and words.value == pc.compressed_words(circ.params, x)
    vd.close()
