"""Compressed proofs (pruned Merkle multiproofs): the numpy model of csrc/proof_compress.hpp, written from the format's two
predicates as include/lcp2.h states them - no shared arithmetic with the portable text, which derives both from one pass over the
indices.  The query indices are an argument, so the model runs without a proof system: compress_model / decompress_model move
words between the two layouts and hash with poseidon_py, compressed_words is the word count alone (parameters and indices).
The layout is plonky2-shaped but parity unpinned; the evaluation at the queried position of every FRI step is kept."""
from types import SimpleNamespace

import numpy as np

from . import poseidon_py

P = poseidon_py.P


def layout(params):
    """the flat proof layout of `params` (csrc/host_protocol.hpp ProofLayout) as far as the format needs it: queries, query_words,
    final_poly, total, and per tree (leaf offset inside a query, leaf words, siblings, index shift)"""
    p = params
    ch, nr, nc, w, qd = p.num_challenges, p.num_routed_wires, p.num_constants, p.num_wires, p.quotient_degree_factor
    npp = (nr + qd - 1) // qd - 1
    capw, lg = 4 << p.cap_height, p.degree_bits + p.rate_bits
    head = 3 * capw + 2 * (nc + nr + w) + 2 * ch * (2 + npp + qd) + p.num_fri_layers * capw
    trees, at = [], 0
    for cols in (nc + nr, w, ch * (1 + npp), ch * qd):
        trees.append((at, cols, lg - p.cap_height, 0))
        at += cols + 4 * (lg - p.cap_height)
    shift, final_bits = 0, p.degree_bits
    for l in range(p.num_fri_layers):
        a = p.fri_arity_bits[l]
        lg, shift, final_bits = lg - a, shift + a, final_bits - a
        trees.append((at, 2 << a, lg - p.cap_height, shift))
        at += (2 << a) + 4 * (lg - p.cap_height)
    final_poly = head + at * p.num_query_rounds
    return SimpleNamespace(queries=head, query_words=at, final_poly=final_poly, total=final_poly + 2 * (1 << final_bits) + 1, trees=trees,
                           outside=head + 2 * (1 << final_bits) + 1)


def leaf_stored(idx, q):
    """the leaf of query q is stored iff no earlier query has the same leaf index"""
    return all(idx[o] != idx[q] for o in range(q))


def sibling_stored(idx, q, level):
    """the sibling of level `level` is stored iff no earlier query passes through the same node and no query at all through the sibling"""
    y = idx[q] >> level
    return all(idx[o] >> level != y for o in range(q)) and all(i >> level != y ^ 1 for i in idx)


def tree_items(idx, leaf_len, nsib):
    """the stored items of one tree in format order: (query, -1 | level, words)"""
    for q in range(len(idx)):
        if leaf_stored(idx, q):
            yield q, -1, leaf_len
        for level in range(nsib):
            if sibling_stored(idx, q, level):
                yield q, level, 4


def compressed_words(params, indices, L=None):
    """the word count of a compressed proof: a function of the parameters and the query indices"""
    L = L or layout(params)
    x = [int(i) for i in indices]
    assert len(x) == params.num_query_rounds
    return L.outside + sum(words for _, leaf_len, nsib, shift in L.trees for _, _, words in tree_items([i >> shift for i in x], leaf_len, nsib))


def compress_model(params, proof, indices):
    """the compressed proof of `proof` (flat words) under the query indices `indices`; nothing is checked"""
    L = layout(params)
    proof = np.ascontiguousarray(proof, dtype=np.uint64).ravel()
    assert proof.size == L.total
    x = [int(i) for i in indices]
    out = [proof[:L.queries], proof[L.final_poly:]]
    for off, leaf_len, nsib, shift in L.trees:
        for q, level, words in tree_items([i >> shift for i in x], leaf_len, nsib):
            at = L.queries + q * L.query_words + off + (0 if level < 0 else leaf_len + 4 * level)
            out.append(proof[at:at + words])
    return np.concatenate(out)


def hash_or_noop(words):
    vals = [int(v) % P for v in words]
    return vals + [0] * (4 - len(vals)) if len(vals) <= 4 else poseidon_py.hash_no_pad(vals)


def two_to_one(left, right):
    return poseidon_py.permute(list(left) + list(right) + [0] * 4)[:4]


def decompress_model(params, comp, indices):
    """the full proof of a compressed one, level by level: every node on a path has both children on a path or stored by the first
    query through the other child.  ValueError for a word count that is not compressed_words(params, indices)"""
    L = layout(params)
    comp = np.ascontiguousarray(comp, dtype=np.uint64).ravel()
    x = [int(i) for i in indices]
    if comp.size != compressed_words(params, x, L):
        raise ValueError("not the word count the indices imply")
    proof = np.zeros(L.total, dtype=np.uint64)
    proof[:L.queries] = comp[:L.queries]
    proof[L.final_poly:] = comp[L.queries:L.outside]
    at = L.outside
    R = len(x)
    for off, leaf_len, nsib, shift in L.trees:
        idx = [i >> shift for i in x]
        stored = {}
        for q, level, words in tree_items(idx, leaf_len, nsib):
            stored[(q, level)] = comp[at:at + words]
            at += words
        nodes = {}  # (level, node index) -> digest
        for q in range(R):
            first = idx.index(idx[q])
            leaf = stored[(first, -1)]
            base = L.queries + q * L.query_words + off
            proof[base:base + leaf_len] = leaf
            if first == q:
                nodes[(0, idx[q])] = hash_or_noop(leaf)
        for level in range(nsib):
            ys = [i >> level for i in idx]
            for q in range(R):
                y = ys[q]
                first = ys.index(y)
                sib = nodes[(level, y ^ 1)] if (y ^ 1) in ys else stored[(first, level)]
                base = L.queries + q * L.query_words + off + leaf_len + 4 * level
                proof[base:base + 4] = np.array([int(v) for v in sib], dtype=np.uint64)
                if first == q:
                    mine, theirs = nodes[(level, y)], [int(v) % P for v in sib]
                    nodes[(level + 1, y >> 1)] = two_to_one(theirs, mine) if y & 1 else two_to_one(mine, theirs)
    assert at == comp.size
    return proof
