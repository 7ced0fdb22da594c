"""The STARK model (eth_lc_plonky2_amd.stark) against itself: its prover and its verifier agree on the three sample AIRs, its witness
check names a planted violation, and a one-word change in any section of a proof is rejected.  No GPU (the library only makes the
FRI configs)."""
import numpy as np
import pytest

import stark_cases as sc

P = sc.P
SMALL = ["fib_n2", "fib_n8", "cubic_n2", "cubic_n8", "poseidon_n2", "poseidon_n8"]


@pytest.mark.parametrize("name", SMALL)
def test_model_prover_and_verifier_agree(name):
    from eth_lc_plonky2_amd import stark
    s = sc.case(name)
    proof, after = sc.model_proof(name)
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges)
    assert proof.size == L.total and all(int(w) < P for w in proof)
    at = 0
    for _, first, words in stark.sections(L):   # the sections tile the proof
        assert first == at
        at += words
    assert at == L.total
    verdict, transcript = sc.model_verdict(s, proof)
    assert verdict == 0 and transcript == after
    # another public input is another statement
    pis = s.pis.copy()
    pis[-1] = (int(pis[-1]) + 1) % P
    assert sc.model_verdict(s, proof, pis=pis)[0] != 0


def test_degrees_of_the_sample_airs():
    from eth_lc_plonky2_amd import stark
    want = {"fibonacci": [1, 1, 1], "cubic": [1, 3, 2], "poseidon_round": [1, 7, 1]}
    for name, (make_air, _) in stark.AIRS.items():
        air = make_air()
        assert [stark.program_degree(air, k) for k in range(3)] == want[name]
    ops = {w & 0xF for w in stark.cubic_air().code[0::2]}
    assert {stark.OP_ADD, stark.OP_SUB, stark.OP_MUL, stark.OP_MULADD, stark.OP_XOR, stark.OP_DBLADD, stark.OP_EMIT, stark.OP_EMITBOOL} <= ops


@pytest.mark.parametrize("air_name", ["fibonacci", "cubic", "poseidon_round"])
def test_check_trace_names_the_planted_violation(air_name):
    from eth_lc_plonky2_amd import stark
    s = sc.shape(air_name, 3, 3, 3, 1)
    n = 1 << s.log_n
    assert stark.check_trace(s.air, s.trace, s.pis) is None
    # a cell of row 4 breaks the transition INTO it (row 3) first, then the one out of it
    t = s.trace.copy()
    t[0, 4] = (int(t[0, 4]) + 1) % P
    kind, constraint, row = stark.check_trace(s.air, t, s.pis)
    assert (kind, row) == (1, 3)
    # row 0 alone: the first-row constraint on that column (the transition out of row 0 comes later in the list)
    t = s.trace.copy()
    t[1, 0] = (int(t[1, 0]) + 1) % P
    assert stark.check_trace(s.air, t, s.pis) == (0, 1, 0)
    # the last row alone: the transition into it (row n - 2) comes first; with the public input changed instead, kind 2 on row n - 1
    pis = s.pis.copy()
    pis[-1] = (int(pis[-1]) + 1) % P
    kind, constraint, row = stark.check_trace(s.air, s.trace, pis)
    assert (kind, row) == (2, n - 1)
    # the prover refuses what the check refuses
    with pytest.raises(ValueError) as e:
        stark.prove(s.air, s.cfg, s.log_n, s.q, s.challenges, t, s.pis, sc.model_challenger())
    assert e.value.args[0] == (0, 1, 0)


@pytest.mark.parametrize("name", ["fib_n8", "cubic_n2"])
def test_one_word_tampering_is_rejected_in_every_section(name):
    from eth_lc_plonky2_amd import stark
    s = sc.case(name)
    proof, _ = sc.model_proof(name)
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges)
    seen = set()
    for section, first, words in stark.sections(L):
        if not words:
            continue
        for w in sorted({first, first + words // 2, first + words - 1}):
            bad = proof.copy()
            bad[w] = (int(bad[w]) + 1) % P
            verdict = sc.model_verdict(s, bad)[0]
            assert verdict != 0, (section, w)
            seen.add(verdict)
    if s.cfg.proof_of_work_bits == 0:   # (with a proof of work, a changed opening moves the transcript and mostly fails check 2 first)
        assert 9 in seen   # a changed opening breaks the identity before any query is looked at
    bad = proof.copy()
    bad[1] = int(bad[1]) + P if int(bad[1]) < (1 << 64) - P else P
    assert sc.model_verdict(s, bad)[0] == 8
