"""K6's half tier: gates whose constraints (times the filter factors of their bundle) have degree <= 2^(q-1) are evaluated on
half of the quotient coset, extended by an iNTT / coset NTT pair and combined with the rest of their filters.  The proof must
not change by a word: every case proves with the tiers on and with LCP2_QUOTIENT_TIERS=0 (read by lcp2_circuit_create) and
compares both proofs with each other and with the oracle's.  Every case also holds the handle's gate -> bundle map
(lcp2_circuit_gate_tiers) to the map tier_lib derives from the programs, so that no case passes because nothing was tiered.

The light-client gate set (the four SHA-256 gates, three selector groups) exists in the C++ host layer: its cases run in
tests/cpp/test_tiers.cpp, which this file builds, starts once per circuit and whose printed gate -> bundle map it checks.  The
circuits made in Python add the generated u32 and recursion gate sets."""
import numpy as np
import pytest

import oracle_lib
import tier_lib


def _u32(m):
    from eth_lc_plonky2_amd import u32_gates as ug
    return ug.reference_gates_circuit(m.standard_params(6, 5), seed=66, native=True)


def _recursion(m):
    from eth_lc_plonky2_amd import recursion_gates as rg
    return rg.recursion_gates_circuit(m.standard_params(5, 4), seed=45, native=True)


def _one_group(m):
    from test_high_rate import low_degree_circuit
    circ, wires, pis = low_degree_circuit(m.standard_params(6, 4), seed=77, max_degree=9)
    assert circ.gateset.num_selectors == 1   # no unused-selector factor
    return circ, wires, pis


def _q4_rate3(m):
    from test_high_rate import oracle_config
    return oracle_config(m, "q4_rate3")


CASES = {
    "synthetic_d5": lambda m: m.circuit.synthetic_circuit(m.standard_params(5, 4), seed=1401),   # tiny transforms (2^7 points)
    "u32_d6": _u32,
    "recursion_d5": _recursion,
    "synthetic_d12": lambda m: m.circuit.synthetic_circuit(m.standard_params(12, 4), seed=1402),  # 4n = 2^14: two-pass plane transforms
    "one_selector_group_d6": _one_group,
    "q4_rate3": _q4_rate3,      # q = 2: the half tier is 2n, only gates of degree <= 2 qualify
}
# gates that must sit on the half tier / must stay on the full tier, by name
MUST_BE_TIERED = {
    "synthetic_d5": ["ConstantGate", "PublicInputGate", "BaseSumGate", "ArithmeticGate"], "synthetic_d12": ["BaseSumGate", "ArithmeticGate"],
    "u32_d6": ["U32ArithmeticGate", "U32AddManyGate", "ComparisonGate"], "recursion_d5": ["ReducingGate", "ArithmeticExtensionGate", "ExponentiationGate"],
    "one_selector_group_d6": ["BaseSumGate", "ArithmeticGate"], "q4_rate3": ["ConstantGate", "PublicInputGate", "BaseSumGate"],
}
MUST_BE_FULL = {"synthetic_d5": ["PoseidonGate"], "synthetic_d12": ["PoseidonGate"], "u32_d6": ["CosetInterpolationGate"],
                "recursion_d5": ["RandomAccessGate"], "one_selector_group_d6": [], "q4_rate3": ["ArithmeticGate"]}


def _build(m, monkeypatch, ctx, circ, tiers):
    if tiers:
        monkeypatch.delenv("LCP2_QUOTIENT_TIERS", raising=False)
    else:
        monkeypatch.setenv("LCP2_QUOTIENT_TIERS", "0")
    data = m.CircuitData.build(ctx, circ)
    monkeypatch.delenv("LCP2_QUOTIENT_TIERS", raising=False)
    return data


def _check_map(circ, data, name):
    gs = circ.gateset
    deg, bun = data.gate_tiers()
    assert list(deg) == tier_lib.gateset_degrees(gs)
    want = tier_lib.expected_bundles(gs, circ.params.quotient_degree_factor)
    assert list(bun) == want, (list(bun), want)
    for g in MUST_BE_TIERED[name]:
        assert bun[gs.index(g)] >= 0, g
    for g in MUST_BE_FULL[name]:
        assert bun[gs.index(g)] == -1, g


@pytest.fixture(scope="module")
def references(oracle):
    """circuit and oracle proof per case, made once"""
    made = {}

    def get(name):
        if name not in made:
            import eth_lc_plonky2_amd as m
            circ, wires, pis = CASES[name](m)
            oc = oracle_lib.OracleCircuit(oracle, circ)
            want = oc.prove(wires, pis)
            want.flags.writeable = False
            made[name] = (circ, wires, pis, oc, want)
        return made[name]
    yield get
    for v in made.values():
        v[3].close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_tiered_proof_equals_untiered_proof_and_oracle(gpu_ctx, references, monkeypatch, name):
    import eth_lc_plonky2_amd as m
    circ, wires, pis, _, want = references(name)
    on, off = _build(m, monkeypatch, gpu_ctx, circ, True), _build(m, monkeypatch, gpu_ctx, circ, False)
    try:
        _check_map(circ, on, name)
        assert (off.gate_tiers()[1] == -1).all() and list(off.gate_tiers()[0]) == tier_lib.gateset_degrees(circ.gateset)
        p_on, p_off = on.prove(wires, pis), off.prove(wires, pis)
        assert oracle_lib.first_mismatch(m, circ.params, p_on, p_off) is None, oracle_lib.first_mismatch(m, circ.params, p_on, p_off)
        assert oracle_lib.first_mismatch(m, circ.params, p_on, want) is None, oracle_lib.first_mismatch(m, circ.params, p_on, want)
        assert (p_on == want).all() and (p_off == want).all()
        assert (on.prove(wires, pis) == want).all()   # the planes of the proof before are scratch, not state
    finally:
        on.close()
        off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alphas", [(0, 1), (1, 0), (0, 0)])
def test_quotient_seam_at_alpha_zero(gpu_ctx, oracle, references, monkeypatch, alphas):
    """lcp2_quotient with forced alpha = 0 / 1 (the edge the weighted-term evaluators special-case): the quotient cap, and the rest
    of the proof, both ways and against the oracle under the same forced challenges"""
    import eth_lc_plonky2_amd as m
    from test_forced_challenges import _case_values, _gpu_forced_proof
    circ, wires, pis, oc, _ = references("u32_d6")
    v = _case_values("random", circ.params.num_challenges, circ.params.degree_bits)
    v["alphas"] = list(alphas)
    rc, want = oc.prove_forced(wires, pis, **v)
    assert rc == 0
    for tiers in (True, False):
        data = _build(m, monkeypatch, gpu_ctx, circ, tiers)
        try:
            assert (data.gate_tiers()[1] >= 0).any() == tiers
            _gpu_forced_proof(m, oracle, data, wires, pis, v, want)   # asserts every stage, the quotient cap among them
        finally:
            data.close()


@pytest.mark.gpu
def test_sharded_circuit_keeps_the_full_tier(gpu_ctx, references):
    """one rank holding all 8 leaf blocks: no gate is tiered, the proof is the unsharded (tiered) proof word for word"""
    import eth_lc_plonky2_amd as m
    from test_sharded_prover import _run_lockstep
    circ, wires, pis, _, want = references("synthetic_d5")
    ranks = _run_lockstep(m, gpu_ctx, circ, wires, pis, 1)
    try:
        deg, bun = ranks[0].data.gate_tiers()
        assert (bun == -1).all() and list(deg) == tier_lib.gateset_degrees(circ.gateset)
        assert (ranks[0].proof == want).all()
    finally:
        for r in ranks:
            r.close()


# ------------------------------------------------------------------ the light-client gate set (host/gates.cpp) through tests/cpp/test_tiers

LC_BUNDLES = [{"ArithmeticGate", "ShaRoundAGate"}, {"ShaAddGate", "ConstantGate", "PublicInputGate"}, {"ShaRoundEGate", "ShaScheduleGate"}]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tiny", "sha"])
def test_light_client_gate_set(which):
    """tiny: the smallest circuit the host builder makes (arithmetic rows and public inputs; the SHA kernels still run at every point
    of the coset); sha: one two_to_one_sha256, 310 rows of the four SHA gates (2^9 rows: the smallest circuit that has them).
    The program itself compares the tiered, the untiered and the oracle's proof word for word, and the caps of the lcp2_commit_wires /
    lcp2_perm_zs / lcp2_quotient seams under forced challenges with alpha = (0, 1), both ways, with orc_prove_forced.  Here: the gate ->
    bundle map it read from the handle is the one the programs' degrees give, the SHA gates are on the half tier, the bundles are
    the three DESIGN.md section 3 names, nothing is tiered with the switch off."""
    r = tier_lib.run_tiers_binary("prove", which)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "proofs equal: tiers on = tiers off = oracle" in r.stdout and "forced alpha = (0, 1) caps equal both ways" in r.stdout
    head = r.stdout.split("\n")[0].split()
    info = dict(zip(head[2::2], head[3::2]))
    assert info["num_selectors"] == "3" and info["quotient_degree_factor"] == "8"
    if which == "sha":
        assert info["degree_bits"] == "9"
    else:
        assert int(info["degree_bits"]) <= 6
    rows = {"on": [], "off": []}
    for ln in r.stdout.splitlines():
        if ln.startswith("tier "):
            _, mode, name, sel, gs, ge, ncons, deg, bun = ln.split()
            rows[mode].append((name, int(sel), int(gs), int(ge), int(ncons), int(deg), int(bun)))
    assert len(rows["on"]) == 9 and [x[:6] for x in rows["on"]] == [x[:6] for x in rows["off"]]
    assert all(x[6] == -1 for x in rows["off"])
    deg = [x[5] for x in rows["on"]]
    assert deg == [0, 1, 1, 2, 3, 3, 3, 3, 7]
    want = tier_lib.bundles_of([x[1:5] for x in rows["on"]], deg, 8)
    got = [x[6] for x in rows["on"]]
    assert got == want, (got, want)
    by_name = {x[0]: x[6] for x in rows["on"]}
    for g in ("ShaAddGate", "ShaRoundAGate", "ShaRoundEGate", "ShaScheduleGate", "ArithmeticGate", "ConstantGate", "PublicInputGate"):
        assert by_name[g] >= 0, g
    assert by_name["PoseidonGate"] == -1 and by_name["NoopGate"] == -1
    bundles = {}
    for name, b in by_name.items():
        if b >= 0:
            bundles.setdefault(b, set()).add(name)
    assert sorted(map(sorted, bundles.values())) == sorted(map(sorted, LC_BUNDLES))
