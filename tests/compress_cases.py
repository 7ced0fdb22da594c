"""Shared by test_proof_compress_emu.py (CPU) and test_proof_compress.py (GPU): the emulation of csrc/proof_compress.hpp, forced index
sets over real Merkle trees (built by the oracle), the three circuit shapes of the GPU tests with proofs from the ORACLE prover, and
the classes of index sets a test asserts its proofs contain:
  a  two queries with the same index            b  two queries that are level-0 siblings (x, x ^ 1)
  c  paths that first merge at a middle level (c_mid) and at the last level below the cap (c_last)
  d  a query whose path meets no other path below the cap"""
import ctypes
import functools

import numpy as np

import oracle_lib
import verify_batch_cases as vc
from rows_lib import build_emu, vp

P = 0xFFFFFFFF00000001
SHAPES = ("tiny", "synthetic_5", "shrink_2")   # 2^3 rows at rate 3 / cap 1 (the smallest circuit the helpers make); 2^5 rows, standard; 2^6 rows at rate 8 / cap 0 / 10 queries
TINY_SEED = 7
FORCED = ("a_same_index", "a_all_the_same", "b_level0_siblings", "b_siblings_later_first", "c_middle_level", "c_last_level_below_cap", "c_top_level_siblings",
          "c_meet_in_the_cap", "d_no_merge", "d_single_query", "mixed", "e_no_siblings", "e_layer_at_its_cap", "f_64_queries", "f_64_distinct_wide",
          "g_noop_leaves_arity_2")   # the keys of forced_cases(), known without loading the library


@functools.lru_cache(maxsize=None)
def emu():
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_compress", (("emu_compress_plan", None, [V, c.c_uint, c.c_uint, c.c_uint, c.c_uint, V]),
                                      ("emu_compressed_words", U, [V, V]), ("emu_compressed_words_max", U, [V]),
                                      ("emu_compress", U, [V, V, V, V]), ("emu_decompress", c.c_int, [V, V, V, U, V]),
                                      ("emu_compress_indices", c.c_int, [V, V, V, V, V])))


def x64(indices):
    x = np.zeros(64, dtype=np.uint32)
    x[:len(indices)] = indices
    return x


def emu_compress(params, indices, proof):
    E, x = emu(), x64(indices)
    out = np.zeros(E.emu_compressed_words_max(ctypes.byref(params)), dtype=np.uint64)
    words = E.emu_compress(ctypes.byref(params), vp(x), vp(np.ascontiguousarray(proof)), vp(out))
    assert words == E.emu_compressed_words(ctypes.byref(params), vp(x)) <= out.size
    return out[:words].copy()


def emu_decompress(params, indices, comp, words=None):
    """(status, proof): the buffer handed over holds exactly `words` words, so a read past them leaves it"""
    E, x = emu(), x64(indices)
    words = comp.size if words is None else words
    exact = np.ascontiguousarray(comp[:words]) if words <= comp.size else np.concatenate([comp, np.zeros(words - comp.size, dtype=np.uint64)])
    proof = np.full(E.emu_compressed_words_max(ctypes.byref(params)), 0xABABABABABABABAB, dtype=np.uint64)
    return E.emu_decompress(ctypes.byref(params), vp(x), vp(exact) if exact.size else None, words, vp(proof)), proof


def classes(params, indices):
    """the classes of the index set, over the initial trees (leaf index x, depth lgN - cap_height)"""
    x = [int(i) for i in indices]
    nsib = params.degree_bits + params.rate_bits - params.cap_height
    found = set()
    for q, a in enumerate(x):
        merges = [(a ^ b).bit_length() for o, b in enumerate(x) if o != q]
        if all(m > nsib for m in merges):
            found.add("d")
        for m in merges:
            if m == 0:
                found.add("a")
            if m == 1 and nsib >= 1:
                found.add("b")
            if 1 < m < nsib - 1:
                found.add("c_mid")
            if m == nsib - 1 and m > 1:
                found.add("c_last")
    return found


def forced_proof(m, params, indices, seed=0):
    """a full-layout proof whose query section holds real Merkle paths (trees over random leaves, built by the oracle) for the given
    query indices; the words outside the queries are random field elements.  Nothing else of it is a proof."""
    from eth_lc_plonky2_amd import proof_compress as pc
    oracle = oracle_lib.load()
    V = ctypes.c_void_p
    oracle.orc_merkle_build.restype, oracle.orc_merkle_build.argtypes = V, [V, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint]
    oracle.orc_merkle_prove.restype, oracle.orc_merkle_prove.argtypes = None, [V, ctypes.c_size_t, V]
    oracle.orc_merkle_free.restype, oracle.orc_merkle_free.argtypes = None, [V]
    L = pc.layout(params)
    rng = np.random.default_rng(seed)
    proof = rng.integers(0, P, size=L.total, dtype=np.uint64)
    lgN = params.degree_bits + params.rate_bits
    for off, leaf_len, nsib, shift in L.trees:
        n = 1 << (lgN - shift)
        leaves = rng.integers(0, P, size=(n, leaf_len), dtype=np.uint64)
        tree = oracle.orc_merkle_build(oracle_lib.vp(leaves), n, leaf_len, params.cap_height)
        try:
            for q, x in enumerate(indices):
                at = L.queries + q * L.query_words + off
                proof[at:at + leaf_len] = leaves[int(x) >> shift]
                sib = np.zeros(max(4 * nsib, 1), dtype=np.uint64)
                oracle.orc_merkle_prove(tree, int(x) >> shift, oracle_lib.vp(sib))
                proof[at + leaf_len:at + leaf_len + 4 * nsib] = sib[:4 * nsib]
        finally:
            oracle.orc_merkle_free(tree)
    return proof


def with_fields(params, **kw):
    import copy
    p = copy.copy(params)
    for k, v in kw.items():
        if k == "fri_arity_bits":
            p.num_fri_layers = len(v)
            for i in range(8):
                p.fri_arity_bits[i] = v[i] if i < len(v) else 0
        else:
            setattr(p, k, v)
    return p


def forced_cases(m):
    """name -> (params, indices): the classes of the issue on index sets chosen by hand.  Base shape: 2^3 rows at rate 2, cap 1 (32
    leaves, 4 siblings in the initial trees), two layers of arity 2 (leaves of 4 words: the no-op hash) - except where a case says."""
    base = with_fields(m.params_config(3, 4, 2, 1, 16, 4, 1, 1), fri_arity_bits=[1, 1])
    Q = lambda n: with_fields(base, num_query_rounds=n)  # noqa: E731
    cases = {
        "a_same_index": (Q(3), [5, 5, 20]),
        "a_all_the_same": (Q(4), [9, 9, 9, 9]),
        "b_level0_siblings": (Q(3), [6, 7, 25]),
        "b_siblings_later_first": (Q(3), [7, 25, 6]),
        "c_middle_level": (Q(3), [0b00001, 0b00010, 0b10000]),   # the first two meet at level 2 of 4
        "c_last_level_below_cap": (Q(2), [0b00001, 0b00110]),    # meet at level 3, the last node below the cap entry
        "c_top_level_siblings": (Q(2), [0b00000, 0b01000]),      # each is the other's last sibling: they meet in the cap entry
        "c_meet_in_the_cap": (Q(2), [0b00000, 0b10000]),         # different cap entries
        "d_no_merge": (Q(2), [3, 19]),
        "d_single_query": (Q(1), [11]),
        "mixed": (Q(7), [1, 0, 1, 14, 30, 31, 8]),
        "e_no_siblings": (with_fields(m.params_config(1, 4, 1, 2, 16, 5, 1, 0), fri_arity_bits=[]), [0, 3, 3, 1, 2]),
        "e_layer_at_its_cap": (with_fields(m.params_config(2, 4, 1, 2, 16, 4, 1, 1), fri_arity_bits=[1]), [7, 6, 1, 7]),
        "f_64_queries": (Q(64), [(37 * i + 3) % 32 for i in range(64)]),
        "f_64_distinct_wide": (with_fields(m.params_config(6, 4, 2, 2, 16, 64, 2, 2), fri_arity_bits=[2, 2]), [(5 * i + 1) % 256 for i in range(64)]),
        "g_noop_leaves_arity_2": (with_fields(base, fri_arity_bits=[1, 1, 1]), [4, 5, 12, 29]),
    }
    assert tuple(cases) == FORCED
    return cases


@functools.lru_cache(maxsize=None)
def proved(shape):
    """(circ, digest, cap, the oracle's proof, public inputs, query indices) of a shape; the indices as the emulated head derives them"""
    import eth_lc_plonky2_amd as m
    if shape == "tiny":
        circ, wires, pis = m.circuit.synthetic_circuit(m.params_config(3, 4, 3, 1, 16, 28, 4, 5), seed=TINY_SEED, npi=0)
        oc = oracle_lib.OracleCircuit(oracle_lib.load(), circ)
        proof = oc.prove(wires, pis)
        assert oc.verify(proof, pis) == 0
        digest, cap = oc.digest()
        oc.close()
        proof.setflags(write=False)
        pis = np.ascontiguousarray(pis, dtype=np.uint64)
    else:
        circ, digest, cap, proof, pis = vc._proved(shape)
    x = indices_of(m, circ, digest, proof, pis)
    assert x is not None
    return circ, digest, cap, proof, pis, x


def indices_of(m, circ, digest, proof_or_comp, pis, compressed=False):
    """the query indices from the words outside the query section - a full proof or a compressed one -, None when the proof of work fails"""
    from eth_lc_plonky2_amd import proof_compress as pc
    L = pc.layout(circ.params)
    w = np.ascontiguousarray(proof_or_comp, dtype=np.uint64)
    outside = np.concatenate([w[:L.queries], w[L.final_poly:]]) if not compressed else np.ascontiguousarray(w[:L.outside])
    desc, keep = m.binding._describe(circ, 0)
    x = np.zeros(64, dtype=np.uint32)
    dg, pi = np.ascontiguousarray(digest, dtype=np.uint64), np.ascontiguousarray(pis, dtype=np.uint64)
    rc = emu().emu_compress_indices(ctypes.byref(desc), vp(dg), vp(outside), vp(pi), vp(x))
    return None if rc else [int(i) for i in x[:circ.params.num_query_rounds]]
