"""lcp2_verify_batch without a GPU: csrc/verify_query.hpp (the layout, the status encoding, the one-lane Merkle path that is the
reference of k_verify_paths, the FRI query k_verify_fri runs) and csrc/verify_head.hpp compiled for the CPU (tests/emu/emu_verify.cpp)
and run over the jobs of the kernels.  Proofs come from the oracle prover, and the expected code of every case is orc_verify's."""
import ctypes

import numpy as np
import pytest

import oracle_lib
import verify_batch_cases as vc
from rows_lib import build_emu, vp

NONE = 0xFFFFFFFF   # VQ_STATUS_NONE: a query without a status


@pytest.fixture(scope="module")
def emuv():
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_verify", (("emu_verify_status", c.c_uint, [c.c_uint, c.c_uint]), ("emu_verify_status_none", c.c_uint, []),
                            ("emu_verify_ordinal", c.c_uint, [c.c_uint, c.c_uint]), ("emu_verify_reduce", c.c_uint, [V, c.c_uint]),
                            ("emu_verify_tree_status", c.c_uint, [V, c.c_uint]), ("emu_verify_num_trees", c.c_uint, [V]),
                            ("emu_merkle_path", c.c_int, [V, c.c_uint, U, V, c.c_uint, V]),
                            ("emu_verify_batch", c.c_int, [V, V, V, V, U, U, V, U, V, V])))


def run_emu(E, m, name, cases=None):
    circ, digest, cap, labels, proofs, pis, want = cases or vc.batch(name)
    desc, keep = m.binding._describe(circ, 0)
    dg, cp = np.ascontiguousarray(digest, dtype=np.uint64), np.ascontiguousarray(cap, dtype=np.uint64)
    k, Q = proofs.shape[0], circ.params.num_query_rounds
    checks = np.full(k, -9, dtype=np.int32)
    statuses = np.zeros((k, Q), dtype=np.uint32)
    rejected = E.emu_verify_batch(ctypes.byref(desc), vp(dg), vp(cp), vp(proofs), proofs.shape[1], k, vp(pis), pis.shape[1], vp(checks), vp(statuses))
    return labels, want, checks, statuses, rejected, circ.params


@pytest.mark.parametrize("name", vc.circuit_names())
def test_emulated_batch_names_the_oracles_check(emuv, name):
    """every case of the batch - the clean proof, one tampered copy per section, the last query's leaf and last sibling, an eval of
    each FRI layer, a word >= p in the head and inside a query, a changed public input, two defects at once - through the emulated
    kernels: the verdicts equal orc_verify's codes element for element, and each per-query status array reduces to its code"""
    import eth_lc_plonky2_amd as m
    labels, want, checks, statuses, rejected, p = run_emu(emuv, m, name)
    assert list(checks) == list(want), [(l, int(g), int(w)) for l, g, w in zip(labels, checks, want) if g != w]
    assert rejected == int((want != 0).sum()) == len(want) - 1
    for i, label in enumerate(labels):
        if want[i] >= 4:
            assert emuv.emu_verify_reduce(vp(np.ascontiguousarray(statuses[i])), p.num_query_rounds) == want[i], label
            first = [int(s) for s in statuses[i] if s != NONE][0]
            assert first & 0xFF == want[i], label
        else:
            assert (statuses[i] == NONE).all(), label  # accepted, or stopped before its queries: no job of it reports
    # the defects sit where the cases put them: the last query's cases leave every earlier query without a status
    for label in ("last_query_leaf", "last_query_last_sibling"):
        i = labels.index(label)
        assert (statuses[i][:-1] == NONE).all() and statuses[i][-1] != NONE and want[i] == 4
    if "two_query_defects" in labels:  # the host stops in query 0's first layer (check 5 or 6): not at the smaller check number of query 3
        two = labels.index("two_query_defects")
        assert want[two] in (5, 6) and statuses[two][0] & 0xFF == want[two] and statuses[two][3] & 0xFF == 4


@pytest.mark.parametrize("name,stratum", [("synthetic_6", "queries"), ("synthetic_5", "noncanonical")])
def test_emulated_batch_over_a_one_word_sweep(emuv, name, stratum):
    """the strata the GPU verifier is held to (verify_batch_cases.sweep), two of them here: every word offset of a query changed in
    one proof each, and words >= p across the whole proof; every verdict is orc_verify's, and a defect inside query q leaves every
    other query without a status"""
    import eth_lc_plonky2_amd as m
    cases = vc.sweep(name, stratum)
    labels, want, checks, statuses, rejected, p = run_emu(emuv, m, name, cases)
    wrong = [(l, int(g), int(w)) for l, g, w in zip(labels, checks, want) if g != w]
    assert not wrong, (len(wrong), wrong[:8])
    assert rejected == len(want) and (want != 0).all()
    if stratum == "noncanonical":
        assert (statuses == NONE).all()  # check 1 stops a proof before its queries
    else:
        for i, (j, q) in enumerate(labels):
            assert (np.delete(statuses[i], q) == NONE).all() and statuses[i][q] & 0xFF == want[i], (j, q)


def test_wrong_lengths_are_refused_before_anything_is_read(emuv):
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = vc.batch("synthetic_5")
    desc, keep = m.binding._describe(circ, 0)
    dg, cp = np.ascontiguousarray(digest, dtype=np.uint64), np.ascontiguousarray(cap, dtype=np.uint64)
    checks = np.full(1, -9, dtype=np.int32)
    for words, npi in ((proofs.shape[1] - 1, pis.shape[1]), (proofs.shape[1] + 1, pis.shape[1]), (proofs.shape[1], pis.shape[1] + 1)):
        assert emuv.emu_verify_batch(ctypes.byref(desc), vp(dg), vp(cp), vp(proofs), words, 1, vp(pis), npi, vp(checks), None) == -1
        assert checks[0] == -9


@pytest.mark.parametrize("leaf_len", [1, 4, 5, 8, 9, 135])
def test_one_lane_merkle_path_equals_the_oracles(oracle, emuv, leaf_len):
    """vq_merkle_path against orc_merkle_verify on both sides of the hash_or_noop boundary (4 | 5) and of the rate block (8 | 9), and
    on a wires-sized leaf: true paths at every index of a 32-leaf tree with a 4-entry cap, and a changed leaf word, sibling word,
    cap word and index are refused by both"""
    rng = np.random.default_rng(leaf_len)
    n, cap_height = 32, 2
    nsib = 5 - cap_height
    leaves = rng.integers(0, vc_p(), size=(n, leaf_len), dtype=np.uint64)
    V = ctypes.c_void_p  # oracle_lib declares no prototypes for the tree object's functions
    oracle.orc_merkle_build.restype, oracle.orc_merkle_build.argtypes = V, [V, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint]
    oracle.orc_merkle_prove.restype, oracle.orc_merkle_prove.argtypes = None, [V, ctypes.c_size_t, V]
    oracle.orc_merkle_free.restype, oracle.orc_merkle_free.argtypes = None, [V]
    tree = oracle.orc_merkle_build(oracle_lib.vp(leaves), n, leaf_len, cap_height)
    cap = np.zeros(4 << cap_height, dtype=np.uint64)
    assert oracle.orc_merkle_cap(oracle_lib.vp(leaves), n, leaf_len, cap_height, oracle_lib.vp(cap)) == 0
    try:
        for index in range(n):
            sib = np.zeros(4 * nsib, dtype=np.uint64)
            oracle.orc_merkle_prove(tree, index, oracle_lib.vp(sib))
            leaf = np.ascontiguousarray(leaves[index])

            def both(lf, ix, sb, cp):
                a = emuv.emu_merkle_path(vp(lf), leaf_len, ix, vp(sb), nsib, vp(cp))
                b = oracle.orc_merkle_verify(oracle_lib.vp(lf), leaf_len, ix, oracle_lib.vp(sb), nsib, oracle_lib.vp(cp))
                assert a == (1 if b else 0)
                return a
            assert both(leaf, index, sib, cap) == 1
            bad = leaf.copy(); bad[leaf_len - 1] ^= np.uint64(1)
            assert both(bad, index, sib, cap) == 0
            bad = sib.copy(); bad[4 * (index % nsib) + index % 4] ^= np.uint64(1)
            assert both(leaf, index, bad, cap) == 0
            bad = cap.copy(); bad[4 * (index >> nsib) + 3] ^= np.uint64(1)
            assert both(leaf, index, sib, bad) == 0
            assert both(leaf, index ^ 1, sib, cap) == 0
    finally:
        oracle.orc_merkle_free(tree)


def vc_p():
    return 0xFFFFFFFF00000001


def test_status_words_order_the_checks_as_the_host_meets_them(emuv):
    """ordinal << 8 | check: inside a query the host meets initial tree 0..3, then per layer the consistency check and the layer's
    Merkle path, then the final polynomial; a minimum over status words must pick the first of them whatever the check numbers are"""
    import eth_lc_plonky2_amd as m
    E = emuv
    layers = 8
    order = [(E.emu_verify_ordinal(0, o), 4) for o in range(4)]
    for l in range(layers):
        order += [(E.emu_verify_ordinal(1, l), 5), (E.emu_verify_ordinal(2, l), 6)]
    order.append((E.emu_verify_ordinal(3, layers), 7))
    assert [o for o, _ in order] == list(range(4 + 2 * layers + 1))
    words = [E.emu_verify_status(o, c) for o, c in order]
    assert words == sorted(words) and len(set(words)) == len(words) and words[-1] < E.emu_verify_status_none() == NONE
    assert all(w & 0xFF == c and w >> 8 == o for w, (o, c) in zip(words, order))
    assert E.emu_verify_ordinal(3, 0) == 4  # no layers: the final polynomial follows the initial trees
    # a layer's Merkle failure (check 6) before a later layer's consistency failure (check 5): the minimum is the 6
    assert min(E.emu_verify_status(E.emu_verify_ordinal(2, 0), 6), E.emu_verify_status(E.emu_verify_ordinal(1, 1), 5)) & 0xFF == 6
    # what the trees of a layout report
    p = m.standard_params(9, 4)
    assert E.emu_verify_num_trees(ctypes.byref(p)) == 4 + p.num_fri_layers
    assert [E.emu_verify_tree_status(ctypes.byref(p), t) for t in range(4)] == words[:4]
    assert [E.emu_verify_tree_status(ctypes.byref(p), 4 + l) for l in range(p.num_fri_layers)] == [words[5 + 2 * l] for l in range(p.num_fri_layers)]
    # the reduction: the FIRST query with a status, not the smallest word
    st = np.array([NONE, words[5], words[0], NONE], dtype=np.uint32)
    assert E.emu_verify_reduce(vp(st), 4) == words[5] & 0xFF == 6
    assert E.emu_verify_reduce(vp(np.full(4, NONE, dtype=np.uint32)), 4) == 0
