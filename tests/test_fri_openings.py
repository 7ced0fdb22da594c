"""lcp2_fri_prove_openings / lcp2_oracle_eval on the device, at the smallest shapes where the code can still go wrong
(openings_cases.CASES).  Per case and per kind of point: the openings against Horner by the oracle's field functions, the proof
against lcp2_fri_verify_openings and against the independent verifier of eth_lc_plonky2_amd.fri_openings, the outgoing transcripts,
determinism, host-listed against device-resident inputs; for the random points also the model prover's proof word for word (small
cases), one-word sweeps, and changed caps, points and transcripts."""
import numpy as np
import pytest

import openings_cases as oc

pytestmark = pytest.mark.gpu
P = oc.P


def challenger(m, c, extra=0):
    ch = m.binding.Challenger()
    seed = oc.transcript_seed(c)
    seed[0] += extra
    ch.observe(seed)
    return ch


def model_challenger(c, extra=0):
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = fo.Challenger()
    seed = oc.transcript_seed(c)
    seed[0] += extra
    ch.observe(seed)
    return ch


def library_verdict(m, c, caps, pts, proof, extra=0):
    ch = challenger(m, c, extra)
    return m.fri_verify_openings(caps, c.cols, c.log_n, c.inst, pts, c.cfg, ch.state, proof), ch


@pytest.mark.parametrize("name", list(oc.CASES))
def test_openings_of_bare_oracles(gpu_ctx, oracle, name):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import fri_openings as fo
    c = oc.case(name)
    n = 1 << c.log_n
    coeffs = oc.coefficients(c)
    values = [oc.values_of(k, c.log_n) for k in coeffs]
    oracles = [gpu_ctx.commit_values(v, c.rate_bits, c.cap_height) for v in values]
    dev_ptrs, dev_oracles = [], []
    for v in values:
        p = gpu_ctx.buffer_alloc(v.size)
        gpu_ctx.buffer_write(p, v)
        dev_ptrs.append(p)
        dev_oracles.append(gpu_ctx.commit_values(p, c.rate_bits, c.cap_height, mem=m.MEM_DEVICE, shape=v.shape))
    caps = [o.cap.ravel() for o in oracles]
    for o, d, k in zip(oracles, dev_oracles, coeffs):
        assert np.array_equal(o.cap, d.cap)
        assert np.array_equal(o.read(lde=False)[0], k)   # the device's coefficients are the ones the values were made from
    L = fo.layout(c.cfg, c.log_n, c.cols, c.points_ranges)
    assert m.fri_openings_words(c.cfg, c.log_n, c.cols, c.inst) == L.total
    try:
        for kind in oc.POINT_KINDS:
            pts = oc.points(c, kind)
            # ---- Oracle.eval against Horner, word for word and canonical (every column, for every kind of point)
            for o, k in zip(oracles, coeffs):
                got = o.eval(pts)
                assert got.shape == (len(pts), o.ncols, 2) and int(got.max()) < P
                for b, z in enumerate(pts):
                    if b and kind != "random":
                        continue   # only the first point differs between the kinds
                    for j in range(o.ncols):
                        assert (int(got[b, j, 0]), int(got[b, j, 1])) == oc.horner(oracle, k[j], z), (kind, b, j)
            want = oc.expected_openings(oracle, c, coeffs, pts)
            # ---- the proof: openings, both verifiers, the transcripts, determinism, device-resident inputs
            ch = challenger(m, c)
            proof = gpu_ctx.fri_prove_openings(oracles, c.inst, pts, c.cfg, ch.state)
            assert proof.size == L.total and int(proof.max()) < P
            assert np.array_equal(proof[:L.fri_caps], want), kind
            verdict, vch = library_verdict(m, c, caps, pts, proof)
            assert verdict == 0, (kind, verdict)
            assert fo.state_words(vch.state) == fo.state_words(ch.state)
            mch = model_challenger(c)
            indices = fo.query_indices(c.cfg, c.log_n, c.cols, c.points_ranges, model_challenger(c), proof)
            assert fo.verify(caps, c.cfg, c.log_n, c.cols, c.points_ranges, pts, mch, proof) == 0, kind
            assert mch.words() == fo.state_words(ch.state)
            ch2 = challenger(m, c)
            assert np.array_equal(gpu_ctx.fri_prove_openings(oracles, c.inst, pts, c.cfg, ch2.state), proof)
            ch3 = challenger(m, c)
            assert np.array_equal(gpu_ctx.fri_prove_openings(dev_oracles, c.inst, pts, c.cfg, ch3.state), proof)
            assert fo.state_words(ch2.state) == fo.state_words(ch3.state) == fo.state_words(ch.state)
            # no query lands on an opened point (a point of H never can: the queries are on the coset 7 H_N), so check 7 is not due
            xs = [fo.query_points(L, i) for i in indices]
            assert not any((x, 0) == (z[0] % P, z[1] % P) for x in xs for z in pts)
            if kind != "random":
                continue
            if c.collide:
                assert len(set(indices)) < len(indices), indices
            if name in oc.SWEEP_WHOLE:   # the model prover makes the same proof, word for word
                pch = model_challenger(c)
                model_proof, model_caps = fo.prove([[list(map(int, col)) for col in k] for k in coeffs], c.cfg, c.log_n, c.points_ranges, pts, pch)
                assert all(np.array_equal(a, b) for a, b in zip(model_caps, caps))
                assert np.array_equal(model_proof, proof)
            # ---- one-word changes: all of the proof, or 200 positions spread over its sections
            where = range(L.total) if name in oc.SWEEP_WHOLE else oc.sweep_positions(L, fo.sections(L), 200, c.seed)
            if name not in oc.SWEEP_WHOLE:
                assert len(where) == len(set(where)) == min(200, L.total)
                assert all(any(first <= w < first + words for w in where) for (_, first, words) in fo.sections(L) if words)
            accepted = []
            for w in where:
                bad = proof.copy()
                bad[w] = (int(proof[w]) + 1) % P
                if library_verdict(m, c, caps, pts, bad)[0] == 0:
                    accepted.append(w)
                if int(proof[w]) < (1 << 64) - P:
                    bad[w] = int(proof[w]) + P
                    assert library_verdict(m, c, caps, pts, bad)[0] == 1, w
            assert not accepted, accepted
            # ---- a cap word of each oracle, a point, the incoming transcript
            # (a path ends in ONE cap entry: the word changed is of the entry the first query's path reaches)
            for o in range(len(caps)):
                bad_caps = [k.copy() for k in caps]
                word = 4 * (indices[0] >> L.init_sib) + o % 4
                bad_caps[o][word] = (int(bad_caps[o][word]) + 1) % P
                assert library_verdict(m, c, bad_caps, pts, proof)[0] == 3, o
            for b in range(len(pts)):
                bad_pts = list(pts)
                bad_pts[b] = (pts[b][0], (pts[b][1] + 1) % P)
                assert library_verdict(m, c, caps, bad_pts, proof)[0] != 0, b
            assert library_verdict(m, c, caps, pts, proof, extra=1)[0] != 0
    finally:   # nothing of the context may outlive it, also when an assertion keeps this frame alive
        for o in oracles + dev_oracles:
            o.close()
        for p in dev_ptrs:
            gpu_ctx.buffer_free(p)


# The proof-of-work search of the bare path beyond its first batch of 2^20 candidates (fri_proof_of_work in csrc/fri_commit.hip, the loop
# test_pow_search.py pins through the Plonk prover): the smallest case with at least two FRI layers, on a transcript seed and at the fewest
# proof-of-work bits under which the minimum witness lies beyond the first batch.  Both were found on the CPU alone: the model prover's
# challenger up to the final polynomial, then every candidate from 0 upwards through the oracle's permutation.  Among the first seed
# words 13 to 24 at 20 bits, 23 gives the witness nearest the start of the second batch; under that seed the minimum witness is 46 696
# at 18 bits and 1 122 902 at 19 (and at 20).
LATE_POW_CASE, LATE_POW_BITS, LATE_POW_SEED, LATE_POW_WITNESS = "3_overlap", 19, 23, 1122902


def test_proof_of_work_beyond_the_first_batch(gpu_ctx, oracle):
    from types import SimpleNamespace
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import fri_openings as fo
    import pow_cases
    deep = [oc.case(n) for n in oc.CASES if oc.case(n).cfg.num_fri_layers >= 2]   # smallest: the shortest proof (and no larger an LDE than any)
    assert LATE_POW_CASE == min(deep, key=lambda k: fo.layout(k.cfg, k.log_n, k.cols, k.points_ranges).total).name
    assert all(oc.CASES[LATE_POW_CASE][0] + oc.CASES[LATE_POW_CASE][1] <= k.log_n + k.rate_bits for k in deep)
    c = oc.case(LATE_POW_CASE)
    log_n, rate, cap, _, _, how, _, queries, _, _ = oc.CASES[LATE_POW_CASE]
    cfg = m.fri_config(log_n, rate, cap, LATE_POW_BITS, queries, 1, log_n, schedule=how[1])
    assert cfg.num_fri_layers == c.cfg.num_fri_layers >= 2 and cfg.proof_of_work_bits == LATE_POW_BITS
    seed = [LATE_POW_SEED] + oc.transcript_seed(c)[1:]
    coeffs = oc.coefficients(c)
    pts = oc.points(c, "random")
    L = fo.layout(cfg, c.log_n, c.cols, c.points_ranges)
    oracles = [gpu_ctx.commit_coeffs(k, c.rate_bits, c.cap_height) for k in coeffs]
    try:
        caps = [o.cap.ravel() for o in oracles]
        ch = m.binding.Challenger()
        ch.observe(seed)
        proof = gpu_ctx.fri_prove_openings(oracles, c.inst, pts, cfg, ch.state)
    finally:
        for o in oracles:
            o.close()
    witness = int(proof[L.pow_witness])
    print("proof-of-work witness", witness, "batch", witness // pow_cases.BATCH)
    assert pow_cases.BATCH <= witness < 2 * pow_cases.BATCH and witness == LATE_POW_WITNESS
    # the minimum: the model's transcript of this proof up to the final polynomial, then the oracle's permutation on every candidate below
    before = fo.Challenger()
    before.observe(seed)
    before.observe(proof[:L.fri_caps])
    before.get_ext()
    for l in range(len(L.arity)):
        before.observe(proof[L.fri_caps + l * L.capw:L.fri_caps + (l + 1) * L.capw])
        before.get_ext()
    before.observe(proof[L.final_poly:L.final_poly + 2 * L.final_len])
    sponge, pending, _ = before.words()
    state = SimpleNamespace(s=np.array(sponge, dtype=np.uint64), inp=pending)
    assert pow_cases.next_solution(oracle, state, -1, LATE_POW_BITS) == witness
    # the model prover's proof, word for word (its own scan starts at the witness: the candidates below it were just ruled out)
    pch = fo.Challenger()
    pch.observe(seed)
    model_proof, model_caps = fo.prove([[list(map(int, col)) for col in k] for k in coeffs], cfg, c.log_n, c.points_ranges, pts, pch, first_witness=witness)
    assert all(np.array_equal(a, b) for a, b in zip(model_caps, caps))
    assert np.array_equal(model_proof, proof)
    assert pch.words() == fo.state_words(ch.state)
    # both verifiers
    vch = m.binding.Challenger()
    vch.observe(seed)
    assert m.fri_verify_openings(caps, c.cols, c.log_n, c.inst, pts, cfg, vch.state, proof) == 0
    assert fo.state_words(vch.state) == fo.state_words(ch.state)
    mch = fo.Challenger()
    mch.observe(seed)
    assert fo.verify(caps, cfg, c.log_n, c.cols, c.points_ranges, pts, mch, proof) == 0
    assert mch.words() == fo.state_words(ch.state)


def test_prover_refusals(gpu_ctx):
    """LCP2_E_INVALID before anything is touched: zeta = 0 (the point index is named), a config that is not the oracles', a wrong
    proof length; LCP2_E_UNSUPPORTED for a coset-sharded oracle"""
    import ctypes
    import eth_lc_plonky2_amd as m
    c = oc.case("2_two_oracles")
    coeffs = oc.coefficients(c)
    oracles = [gpu_ctx.commit_coeffs(k, c.rate_bits, c.cap_height) for k in coeffs]
    pts = oc.points(c, "random")

    def refused(status, oracles=oracles, pts=pts, cfg=c.cfg, inst=c.inst, words=None):
        ch = m.binding.Challenger()
        handles = (ctypes.c_void_p * len(oracles))(*[o.handle for o in oracles])
        cols = np.array([o.ncols for o in oracles], dtype=np.uint32)
        words = m.fri_openings_words(cfg, c.log_n, cols, inst) if words is None else words
        proof = np.full(max(words, 1), 0xABAB, dtype=np.uint64)
        flat = np.array([w for z in pts for w in z], dtype=np.uint64)
        rc = gpu_ctx.lib.lcp2_fri_prove_openings(gpu_ctx.handle, handles, ctypes.byref(inst), flat.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg),
                                                 ctypes.byref(ch.state), proof.ctypes.data_as(ctypes.c_void_p), words)
        assert rc == status, rc
        assert (proof == 0xABAB).all() and list(ch.state.sponge) == [0] * 12
        return gpu_ctx.lib.lcp2_last_error(gpu_ctx.handle).decode()

    extra = []
    try:
        _refusals(m, c, coeffs, oracles, pts, refused, gpu_ctx, extra)
    finally:
        for o in oracles + extra:
            o.close()


def _refusals(m, c, coeffs, oracles, pts, refused, gpu_ctx, extra):
    assert "point 1" in refused(-1, pts=[pts[0], (0, 0)])
    assert "point 0" in refused(-1, pts=[(P, 0), pts[1]])
    other_rate = m.fri_config(c.log_n, c.rate_bits - 1, c.cap_height, 3, 6, 2, 1)
    assert "does not share" in refused(-1, cfg=other_rate, words=100)
    other_cap = m.fri_config(c.log_n, c.rate_bits, c.cap_height + 1, 3, 6, 2, 1)
    assert "does not share" in refused(-1, cfg=other_cap, words=100)
    refused(-1, words=m.fri_openings_words(c.cfg, c.log_n, c.cols, c.inst) - 1)
    refused(-1, inst=m.fri_instance(2, [[(0, 0, 3), (1, 0, 3)], [(1, 1, 1)]]), words=100)
    sharded = gpu_ctx.commit_cosets(coeffs[1], 0, 4, c.rate_bits, c.rate_bits)
    extra.append(sharded)
    both = m.fri_config(c.log_n, c.rate_bits, c.rate_bits, 3, 6, 2, 1)
    plain = gpu_ctx.commit_coeffs(coeffs[0], c.rate_bits, c.rate_bits)
    extra.append(plain)
    assert "coset-sharded" in refused(-6, oracles=[plain, sharded], cfg=both, words=100)
    with pytest.raises(m.Lcp2Error) as e:
        sharded.eval([(1, 2)])
    assert e.value.status == -6


def test_commitment_and_openings_of_the_wire_columns_match_the_plonk_prover(gpu_ctx):
    """the wire columns of a 2^5-row circuit committed as a bare oracle: the cap is the wires cap of the proof, and Oracle.eval at the
    proof's zeta is the wires part of its opening section"""
    import eth_lc_plonky2_amd as m
    params = m.standard_params(5, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=3)
    data = m.CircuitData.build(gpu_ctx, circ)
    o = None
    try:
        proof = data.prove(wires, pis)
        lay = m.proof_layout(params)
        zeta = data.last_challenges()["zeta"]
        o = gpu_ctx.commit_values(wires, params.rate_bits, params.cap_height)
        assert np.array_equal(o.cap.ravel(), proof[lay.wires_cap:lay.wires_cap + lay.cap_words])
        assert np.array_equal(o.eval([zeta]).ravel(), proof[lay.op_wires:lay.op_wires + 2 * params.num_wires])
    finally:
        if o is not None:
            o.close()
        data.close()
