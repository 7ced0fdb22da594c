"""The model of the STARK permutation argument (eth_lc_plonky2_amd.stark with perm=) against itself: its prover and verifier agree
on the three sample AIRs, every one-word change of a small proof is rejected, a changed cell of an rhs column is located as kind 3,
and the Z columns are what their definition says.  No GPU (the library only makes the FRI configs)."""
import numpy as np
import pytest

import stark_cases as sc
import stark_perm_cases as pc

P = sc.P
SMALL = ["shuffle_n2", "range_n8", "tuples_n32"]


@pytest.mark.parametrize("name", SMALL)
def test_model_accepts_its_own_proofs(name):
    from eth_lc_plonky2_amd import stark
    s = pc.case(name)
    proof, after = pc.model_proof(name)
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges, perm=s.perm)
    assert proof.size == L.total and all(int(w) < P for w in proof)
    assert L.num_z == s.perm.num_z(s.challenges) == -(-len(s.perm.pairs) * s.challenges // s.batch)
    at = 0
    for _, first, words in stark.sections(L):   # the sections tile the proof, the Z cap between the other two
        assert first == at
        at += words
    assert at == L.total and [n for n, _, _ in stark.sections(L)][:3] == ["trace_cap", "z_cap", "quotient_cap"]
    verdict, transcript = pc.model_verdict(s, proof)
    assert verdict == 0 and transcript == after
    # without the permutation the same words are not even a proof of the right length
    assert stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges).total < L.total


def test_every_one_word_change_is_rejected():
    s = pc.case("shuffle_n2")
    proof, _ = pc.model_proof("shuffle_n2")
    seen = set()
    for w in range(proof.size):
        bad = proof.copy()
        bad[w] = (int(bad[w]) + 1) % P
        verdict = pc.model_verdict(s, bad)[0]
        assert verdict != 0, w
        seen.add(verdict)
    assert 9 in seen   # no proof of work here: a changed opening reaches the identity
    for w in (0, 4, 11):   # one word of each of the three caps (4 words each), made non-canonical
        bad = proof.copy()
        bad[w] = int(bad[w]) + P if int(bad[w]) < (1 << 64) - P else P
        assert pc.model_verdict(s, bad)[0] == 8


@pytest.mark.parametrize("name", SMALL)
def test_changed_rhs_cell_is_located_as_kind_3(name):
    from eth_lc_plonky2_amd import fri_openings as fo
    from eth_lc_plonky2_amd import stark
    s = pc.case(name)
    n = 1 << s.log_n
    ch = fo.Challenger()
    ch.observe([1, 2, 3])
    sets = stark.draw_challenge_sets(s.perm, s.challenges, ch)
    assert len(sets) == s.batch and all(len(st) == s.challenges for st in sets)
    assert stark.check_trace(s.air, s.trace, s.pis, perm=s.perm, challenge_sets=sets) is None
    # the last column pair of the last pair: its Z column is the last one, whatever the batching
    l, r = s.perm.pairs[-1][-1]
    t = s.trace.copy()
    t[r, n // 2] = (int(t[r, n // 2]) + (1 << 40)) % P
    if name == "range_n8":   # (there the changed cell also breaks the AIR's own transition, which is found first)
        assert stark.check_trace(s.air, t, s.pis, perm=s.perm, challenge_sets=sets)[0] == 1
        return
    assert stark.check_trace(s.air, t, s.pis, perm=s.perm, challenge_sets=sets) == (3, s.perm.num_z(s.challenges) - 1, n - 1)
    ch = sc.model_challenger()
    before = ch.words()
    with pytest.raises(ValueError) as e:
        stark.prove(s.air, s.cfg, s.log_n, s.q, s.challenges, t, s.pis, ch, perm=s.perm)
    assert e.value.args[0] == (3, s.perm.num_z(s.challenges) - 1, n - 1) and ch.words() == before
    # the first pair instead: Z column 0
    t = s.trace.copy()
    r = s.perm.pairs[0][0][1]
    t[r, 0] ^= np.uint64(1)
    assert stark.check_trace(s.air, t, s.pis, perm=s.perm, challenge_sets=sets) == (3, 0, n - 1)


def test_z_columns_follow_their_definition():
    """perm_z_columns (whole columns at a time) against the row-by-row products, and the all-rows constraint on every row"""
    from eth_lc_plonky2_amd import stark
    s = pc.case("tuples_n32")
    n = 1 << s.log_n
    rng = np.random.default_rng(5)
    sets = [[(int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64))) for _ in range(s.challenges)] for _ in range(s.batch)]
    zs = stark.perm_z_columns(s.trace, s.perm, sets)
    assert zs.shape == (2, n) and stark.perm_open_z(s.trace, s.perm, sets) is None
    rows = [[int(s.trace[c][i]) for c in range(s.air.width)] for i in range(n)]
    for z, batch in enumerate(s.perm.batches(s.challenges)):
        assert len(batch) == (4, 2)[z] and int(zs[z, 0]) == 1
        for i in range(n):
            num, den = stark.perm_products(s.perm, batch, sets, rows[i], stark.BASE)
            assert (int(zs[z, (i + 1) % n]) * den - int(zs[z, i]) * num) % P == 0
