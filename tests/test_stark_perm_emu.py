"""The portable text of the STARK permutation argument (csrc/stark.hpp) on the CPU, through tests/emu/emu_stark_perm.cpp, against the
model (eth_lc_plonky2_amd.stark with perm=): word counts, per-row ratios, Z columns, the closing verdict, the per-point quotient
values, and lcp2_stark_verify_perm - host only, so tested from the library itself and from the harness - on the model's proofs, on
one-word changes, without a permutation and on refused descriptions.  No GPU."""
import ctypes

import numpy as np
import pytest

import stark_cases as sc
import stark_perm_cases as pc
from rows_lib import vp

P = sc.P
AIR_Q = {"shuffle": 0, "range_check": 1, "tuples": 0}   # the smallest q the AIR's own degree admits


def batch_sizes(num_instances, Q):
    """1, Q and - where there is one - the smallest B <= Q that leaves a partial last batch"""
    partial = [B for B in range(2, Q + 1) if num_instances % B]
    return sorted({1, Q} | set(partial[:1]))


def emu_columns(s, draws, trace, threads=128):
    n, num_z = 1 << s.log_n, s.perm.num_z(s.challenges)
    ratio, zs = np.zeros((num_z, n), dtype=np.uint64), np.zeros((num_z, n), dtype=np.uint64)
    t = np.ascontiguousarray(trace, dtype=np.uint64)
    rc = pc.emu().emu_stark_perm_columns(ctypes.byref(s.desc), ctypes.byref(s.sperm), vp(draws), vp(t), threads, vp(ratio), vp(zs))
    assert rc >= -1
    return ratio, zs, None if rc < 0 else rc


@pytest.mark.parametrize("log_n", range(1, 7))
@pytest.mark.parametrize("air_name", list(AIR_Q))
def test_ratios_z_columns_and_quotient_values_equal_the_model(air_name, log_n):
    """log_n 1 .. 6, rate_bits 1 .. 3, every q from the AIR's smallest up to rate_bits, 1, 2 and 4 challenges, B = 1, B = Q and a B
    with a partial last batch; the ratio text with lanes 128, 4 and 1 rows apart (n below, at and above four rows per lane)"""
    from eth_lc_plonky2_amd import stark
    import eth_lc_plonky2_amd as m
    rng = np.random.default_rng(4)
    shapes, partial = 0, 0
    for log_n in (log_n,):
        n = 1 << log_n
        for rate_bits in range(1, 4):
            lde = leaves = None
            for q in range(AIR_Q[air_name], rate_bits + 1):
                for challenges in (1, 2, 4):
                    num_inst = len(stark.PERM_AIRS[air_name][2]().pairs) * challenges
                    for batch in batch_sizes(num_inst, 1 << q):
                        s = pc.shape(air_name, log_n, rate_bits, q, challenges, batch)
                        L = stark.layout(s.air, s.cfg, log_n, q, challenges, perm=s.perm)
                        assert pc.emu().emu_stark_perm_words(ctypes.byref(s.desc), ctypes.byref(s.sperm)) == L.total == m.stark_proof_words(s.desc, s.sperm)
                        if lde is None:
                            cols = [stark.coset_values(stark.interpolate(s.trace[c]), log_n + rate_bits) for c in range(s.air.width)]
                            lde = np.array(cols, dtype=np.uint64)
                            leaves = [[col[i] for col in cols] for i in range(1 << (log_n + rate_bits))]
                        sets = [[(int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64))) for _ in range(challenges)] for _ in range(batch)]
                        draws = pc.flat_draws(sets)
                        want_ratio = np.array(stark.perm_ratios(s.trace, s.perm, sets), dtype=np.uint64)
                        want_zs = stark.perm_z_columns(s.trace, s.perm, sets)
                        for threads in (128, 4, 1):
                            ratio, zs, open_z = emu_columns(s, draws, s.trace, threads)
                            assert (ratio == want_ratio).all() and (zs == want_zs).all() and open_z is None, (log_n, q, challenges, batch, threads)
                        z_cols = [stark.coset_values(stark.interpolate(col), log_n + rate_bits) for col in want_zs]
                        z_leaves = [[col[i] for col in z_cols] for i in range(1 << (log_n + rate_bits))]
                        alphas = [int(a) for a in rng.integers(1, P, challenges, dtype=np.uint64)]
                        want = stark.quotient_values(s.air, log_n, rate_bits, q, leaves, [int(v) for v in s.pis], alphas, s.perm, sets, z_leaves)
                        out = np.zeros((challenges, n << q), dtype=np.uint64)
                        assert pc.emu().emu_stark_perm_quotient(ctypes.byref(s.desc), ctypes.byref(s.sperm), vp(draws), vp(s.pis), vp(lde),
                                                                vp(np.array(z_cols, dtype=np.uint64)), vp(np.array(alphas, dtype=np.uint64)), vp(out)) == 0
                        assert [[int(v) for v in row] for row in out] == want, (log_n, rate_bits, q, challenges, batch)
                        # the quotient is a polynomial of degree < 2^q n: B <= Q is exactly what makes the top coefficient vanish
                        assert stark.coset_interpolate(want[0], log_n + q)[-1] == 0
                        shapes += 1
                        partial += num_inst % batch != 0
    assert shapes >= 18 and (partial or air_name != "tuples")   # (per log_n: 3 rates, their q, 3 challenge counts, 1 to 3 batch sizes)


def test_closing_verdict_and_zero_denominators():
    from eth_lc_plonky2_amd import stark
    s = pc.shape("tuples", 4, 2, 2, 2, 4)
    n = 1 << s.log_n
    rng = np.random.default_rng(6)
    sets = [[(int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64))) for _ in range(2)] for _ in range(4)]
    draws = pc.flat_draws(sets)
    # a changed rhs cell of the last pair: Z 1 stays open, Z 0 closes; of the first pair: Z 0
    t = s.trace.copy()
    t[11, 5] ^= np.uint64(1)
    ratio, zs, open_z = emu_columns(s, draws, t)
    assert open_z == 1 == stark.perm_open_z(t, s.perm, sets) and (zs == stark.perm_z_columns(t, s.perm, sets)).all()
    t[6, n - 1] ^= np.uint64(1)
    assert emu_columns(s, draws, t)[2] == 0 == stark.perm_open_z(t, s.perm, sets)
    # non-canonical trace words are reduced (the range-check trace holds small values, which have a second representation)
    s = pc.shape("range_check", 4, 2, 1, 2, 2)
    t = s.trace.copy()
    small = np.argwhere(t < np.uint64((1 << 64) - P))
    for c, r in small[::2]:
        t[c, r] += np.uint64(P)
    assert len(small) and (emu_columns(s, draws[:8], t)[0] == emu_columns(s, draws[:8], s.trace)[0]).all()
    # a zero denominator: gamma = -rhs on one row of the one-column pair.  The ratio of that row is 0 (the inverse of 0 is 0), as is
    # that of the row whose lhs holds the same value (a zero numerator); the rows that share their inversions keep their ratios, and
    # the product does not close
    s = pc.shape("shuffle", 4, 1, 0, 1, 1)
    row = 6
    sets = [[(12345, (P - int(s.trace[1, row])) % P)]]
    want = np.array(stark.perm_ratios(s.trace, s.perm, sets), dtype=np.uint64)
    for threads in (128, 2, 1):
        ratio, zs, open_z = emu_columns(s, pc.flat_draws(sets), s.trace, threads)
        assert (ratio == want).all() and int(ratio[0, row]) == 0 and np.count_nonzero(ratio) == n - 2 and open_z == 0


VERIFY_CASES = ["shuffle_n2", "range_n8", "tuples_n32"]


def verdicts(s, proof, pis=None):
    """(library, harness, model): the failed check, 0 if accepted"""
    lib, lib_after = pc.lib_verdict(s, proof, pis)
    rc, failed, emu_after = pc.emu_verdict(s, proof, pis)
    assert rc in (0, -7) and (rc == 0) == (failed == 0)
    model, model_after = pc.model_verdict(s, proof, pis)
    if lib == 0:
        assert lib_after == emu_after == model_after
    return lib, failed, model


@pytest.mark.parametrize("name", VERIFY_CASES)
def test_verifier_accepts_the_models_proofs(name):
    s = pc.case(name)
    proof, after = pc.model_proof(name)
    assert verdicts(s, proof) == (0, 0, 0)
    assert pc.lib_verdict(s, proof)[1] == after
    if len(s.pis):
        pis = s.pis.copy()
        pis[0] = (int(pis[0]) + 1) % P
        v = verdicts(s, proof, pis)
        assert v[0] == v[1] == v[2] != 0


@pytest.mark.parametrize("name", ["shuffle_n2", "tuples_n32"])
def test_changed_words_fail_the_check_the_model_names(name):
    from eth_lc_plonky2_amd import stark
    s = pc.case(name)
    proof, _ = pc.model_proof(name)
    L = stark.layout(s.air, s.cfg, s.log_n, s.q, s.challenges, perm=s.perm)
    assert (L.trace_cap, L.z_cap, L.quot_cap, L.openings) == (0, L.capw, 2 * L.capw, 3 * L.capw)
    # each cap: a canonical change moves the transcript, a non-canonical word is check 8 before anything else
    for cap in (L.trace_cap, L.z_cap, L.quot_cap):
        bad = proof.copy()
        bad[cap + 1] = (int(bad[cap + 1]) + 1) % P
        v = verdicts(s, bad)
        assert v[0] == v[1] == v[2] != 0, cap
        bad = proof.copy()
        bad[cap + L.capw - 1] = int(bad[cap + L.capw - 1]) + P if int(bad[cap + L.capw - 1]) < (1 << 64) - P else P
        assert verdicts(s, bad) == (8, 8, 8)
    # each opening section - the trace, Z and the chunks at zeta, Z at g zeta - enters the identity.  The trace at g zeta enters it
    # through the AIR's transition constraints only: these two AIRs have none, and the change is left to the queries
    assert s.air.programs[1][1] == 0
    ends = {"local": (L.op_local, L.op_z), "z": (L.op_z, L.op_quotient), "quotient": (L.op_quotient, L.op_next), "next": (L.op_next, L.op_z_next),
            "z_next": (L.op_z_next, L.openings + L.fo.fri_caps)}
    assert ends["z"][1] - ends["z"][0] == ends["z_next"][1] - ends["z_next"][0] == 2 * L.num_z
    for section, (first, end) in ends.items():
        for w in sorted({first, end - 1}):
            bad = proof.copy()
            bad[w] = (int(bad[w]) + 1) % P
            v = verdicts(s, bad)
            want = (3, 4, 5, 6, 7) if section == "next" else (9,)
            assert v[0] == v[1] == v[2] and v[0] in (want if s.cfg.proof_of_work_bits == 0 else want + (2,)), (section, w, v)
    # a query word, the final polynomial, the proof-of-work witness: the opening layer's numbers come through
    for w in (L.openings + L.fo.queries, L.openings + L.fo.queries + L.fo.init_off[1], L.openings + L.fo.final_poly, L.openings + L.fo.pow_witness):
        bad = proof.copy()
        bad[w] = (int(bad[w]) + 1) % P
        v = verdicts(s, bad)
        assert v[0] == v[1] == v[2] and v[0] in (2, 3, 4, 5, 6, 7), (w, v)


def test_without_a_permutation_the_calls_are_the_existing_ones():
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    empty = stark.pack_stark_perm(stark.Permutation([], 1))
    for name in ("fib_n2", "cubic_n2"):
        s = sc.case(name)
        proof, after = sc.model_proof(name)
        words = m.stark_proof_words(s.desc)
        assert words == proof.size == m.stark_proof_words(s.desc, empty) == pc.emu().emu_stark_perm_words(ctypes.byref(s.desc), None)
        assert words == pc.emu().emu_stark_perm_words(ctypes.byref(s.desc), ctypes.byref(empty))
        for w in (None, 0, proof.size // 2, proof.size - 1):
            pr = proof.copy()
            if w is not None:
                pr[w] = (int(pr[w]) + 1) % P
            want = sc.lib_verdict(s, pr)
            assert (want[0] == 0) == (w is None)
            for sperm in (None, empty):
                ch = sc.lib_challenger()
                from eth_lc_plonky2_amd import fri_openings as fo
                assert (m.stark_verify(s.desc, s.pis, ch.state, pr, perm=sperm), fo.state_words(ch.state)) == want
                rc, failed, transcript = pc.emu_verdict(s, pr, sperm=sperm, no_perm=sperm is None)
                assert (failed, transcript) == want and rc == (0 if w is None else -7)


def test_refusals_name_their_reason():
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    s = pc.case("tuples_n32")   # width 12, q = 2, 2 challenges
    proof, _ = pc.model_proof("tuples_n32")

    def refused(reason, perm=None, desc=None, sperm=None):
        sperm = sperm if sperm is not None else stark.pack_stark_perm(perm)
        desc = desc or s.desc
        assert reason in pc.emu_problem(desc, sperm)
        assert m.stark_proof_words(desc, sperm) == 0 == pc.emu().emu_stark_perm_words(ctypes.byref(desc), ctypes.byref(sperm))
        ch = sc.lib_challenger()
        before = bytes(ch.state)
        with pytest.raises(m.Lcp2Error) as e:
            m.stark_verify(desc, s.pis, ch.state, proof, perm=sperm)
        assert e.value.status == -1 and bytes(ch.state) == before   # the transcript was not touched
        assert pc.emu_verdict(s, proof, desc=desc, sperm=sperm)[0] == -1
        return True

    assert pc.emu_problem(s.desc, s.sperm) is None
    Pm = stark.Permutation
    one = [(0, 6)]
    # num_pairs above 64 (64 pairs of one challenge each in batches of 1 are 64 Z columns: taken)
    d1 = stark.pack_stark_desc(s.air, s.cfg, s.log_n, s.q, 1)
    assert pc.emu_problem(d1, stark.pack_stark_perm(Pm([one] * 64, 1))) is None
    assert refused("num_pairs above 64", Pm([one] * 65, 1), desc=d1)
    # a pair without columns; a run outside `columns`
    assert refused("pair 1 has no columns", Pm([one, []], 1))
    sp = stark.pack_stark_perm(Pm([one, [(1, 7), (2, 8)]], 1))
    sp.num_column_pairs = 2
    assert refused("pair 1 lies outside columns", sperm=sp)
    sp = stark.pack_stark_perm(Pm([one], 1))
    sp._pairs[0] = 0xFFFFFFFF   # first + count must not wrap
    assert refused("pair 0 lies outside columns", sperm=sp)
    # num_column_pairs above 4096 (4096 are taken)
    assert pc.emu_problem(s.desc, stark.pack_stark_perm(Pm([one * 4096], 1))) is None
    assert refused("num_column_pairs above 4096", Pm([one * 4097], 1))
    # a column >= width, on either side
    assert refused("column pair 1: column not below width", Pm([[(0, 6), (12, 7)]], 1))
    assert refused("column pair 0: column not below width", Pm([[(0, 12)]], 1))
    # batch_size outside [1, Q]
    assert refused("batch_size outside", Pm([one], 0)) and refused("batch_size outside", Pm([one], 5))
    assert pc.emu_problem(s.desc, stark.pack_stark_perm(Pm([one], 4))) is None
    # numZ above 64: 33 pairs of 2 challenges in batches of 1
    assert refused("more than 64 Z columns", Pm([one] * 33, 1))
    assert pc.emu_problem(s.desc, stark.pack_stark_perm(Pm([one] * 33, 2))) is None
    # null tables
    sp = stark.pack_stark_perm(Pm([one], 1))
    sp.columns = None
    assert refused("null pairs or columns", sperm=sp)
    # what lcp2_stark_prove refuses of the description, and what the opening layer refuses of the config, come through
    assert refused("quotient_degree_bits exceeds rate_bits", s.perm, desc=stark.pack_stark_desc(s.air, s.cfg, s.log_n, 4, 2))
    assert refused("num_challenges outside", s.perm, desc=stark.pack_stark_desc(s.air, s.cfg, s.log_n, s.q, 5))
    air = stark.range_check_air()
    assert refused("constraint degree above", stark.range_check_perm(1), desc=stark.pack_stark_desc(air, s.cfg, s.log_n, 0, 1))
    assert refused("too many queries", s.perm, desc=stark.pack_stark_desc(s.air, m.fri_config(5, 3, 2, 0, 65, 1, 5, schedule=[1]), s.log_n, s.q, 2))
    # a wrong proof_words with a good description
    ch = sc.lib_challenger()
    with pytest.raises(m.Lcp2Error) as e:
        m.stark_verify(s.desc, s.pis, ch.state, proof[:-1], perm=s.sperm)
    assert e.value.status == -1
    # lcp2_stark_prove_perm without a context
    lib = m.load_library()
    assert lib.lcp2_stark_prove_perm(None, ctypes.byref(s.desc), ctypes.byref(s.sperm), vp(s.trace), 0, vp(s.pis), ctypes.byref(ch.state),
                                     vp(np.zeros(proof.size, dtype=np.uint64)), proof.size, None) == -1
