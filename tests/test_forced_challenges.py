"""Permutation, quotient and opening stages at challenge values a Poseidon transcript never draws.

In a whole proof beta, gamma, alpha and zeta are random-looking canonical field elements, so the places where the kernels branch
on, or divide by, a challenge never see their edge: alpha = 0 (k_q_perm's Horner chain in 1 / alpha, the alpha tables of the gate
kernels, QEmit's zero step), beta = 0 (every chunk quotient is 1), zeta with a zero component, in the subgroup H, on the LDE
coset, g zeta = 1 (k_compose_tables / k_divide_finalize divide by powers of zeta and g zeta), non-canonical encodings (gl_canon in
perm_begin, stage_quotient_values, lcp2_fri_open*), and one challenge slot instead of two.  (QUOTIENT_MAX_CH is 2: three and four slots, which the oracle proves, are refused by the
library, and that refusal is pinned here.)

The seams lcp2_perm_zs / lcp2_quotient / lcp2_fri_open take the challenges from the caller; the reference is the oracle proving
under the same forced challenges (orc_prove_forced: the transcript runs as always, the drawn value is replaced).  That path is
pinned on the CPU first: forcing the transcript's own values is orc_prove word for word, Z and the partial products equal a
restatement of the plonky2 definition in Python integers, the verifier checks the identity at alpha = 0, a zero denominator is
an error and not a silent 0.  Then every case is driven through the GPU seams and compared stage by stage.

zeta = 0 is the one value the library refuses (LCP2_E_INVALID, include/lcp2.h at lcp2_fri_open)."""
import zlib

import numpy as np
import pytest

import oracle_lib
from oracle_lib import Challenger, first_mismatch

P = oracle_lib.P
U64 = (1 << 64) - 1
E_INVALID, E_UNSUPPORTED = -1, -6


# ------------------------------------------------------------------ circuits (nothing above 2^9 rows; the smallest the suite proves)

def _synthetic(num_challenges):
    def make(m):
        params = m.standard_params(6, 4)
        params.num_challenges = num_challenges
        return m.circuit.synthetic_circuit(params, seed=1300 + num_challenges)
    return make


def _reference_gates(native):
    def make(m):
        from eth_lc_plonky2_amd import u32_gates as ug
        return ug.reference_gates_circuit(m.standard_params(6, 5), seed=66, native=native)
    return make


def _recursion_gates(m):
    from eth_lc_plonky2_amd import recursion_gates as rg
    return rg.recursion_gates_circuit(m.standard_params(5, 4), seed=45, native=True)


def _high_rate(name):
    def make(m):
        from test_high_rate import oracle_config
        return oracle_config(m, name)
    return make


CIRCUITS = {
    "A": _synthetic(2),                  # native Poseidon k_q_gate, Arithmetic + BaseSum in k_q_light, interpreted Constant / PublicInput
    "A1": _synthetic(1),                 # one challenge slot: the second row of hh[c2][c] and of every table stays unused
    "A3": _synthetic(3), "A4": _synthetic(4),   # oracle only: the library takes at most QUOTIENT_MAX_CH = 2 slots (refusal pinned below)
    "B": _reference_gates(True),         # generated evaluators
    "Bi": _reference_gates(False),       # B': the gate-program interpreter
    "C": _recursion_gates,               # generated evaluators of the recursion gates
    "D_q3_rate2": _high_rate("q3_rate2"),  # chunks of 3 and 4 routed wires: no multiple of k_q_perm's batches of 8; Q < 2^rate_bits
    "D_q4_rate6": _high_rate("q4_rate6"),
}


# ------------------------------------------------------------------ challenge values

def _root_of_unity(bits):
    """plonky2's primitive 2^bits-th root of unity: the multiplicative generator 7 to the (p - 1) / 2^bits"""
    return pow(7, (P - 1) >> bits, P)


def _case_values(case, ch, degree_bits):
    """{betas, gammas, alphas, zeta} of a case for `ch` challenge slots: the kind the case names takes its edge values, the
    others are seeded random canonical values (r).  Any u64 is a legal input; values >= p are the non-canonical cases."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (case, ch, degree_bits)).encode()))

    def r(k=ch):
        return [int(v) for v in rng.integers(1, P, size=k, dtype=np.uint64)]

    v = {"betas": r(), "gammas": r(), "alphas": r(), "zeta": r(2)}
    w = _root_of_unity(degree_bits)
    kind, _, what = case.partition(":")
    if kind == "alpha":
        rr = r()
        v["alphas"] = {
            "0,r": [0] + rr[1:], "r,0": rr[:-1] + [0] if ch > 1 else [0], "0,0": [0] * ch, "1,p-1": [1, P - 1, 1, P - 1][:ch],
            "p,p+1": [P, P + 1, U64, P + 2][:ch], "2^32-1,2^32": [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) - 2][:ch],
            "2^64-1,r": [U64] + rr[1:],
        }[what]
    elif kind == "beta_gamma":   # every slot takes the pair; r differs from slot to slot
        b, g = what.split(",")
        one = {"0": 0, "1": 1, "p-1": P - 1, "p+5": P + 5, "2^64-1": U64}
        v["betas"] = r() if b == "r" else [one[b]] * ch
        v["gammas"] = r() if g == "r" else [one[g]] * ch
    elif kind == "zeta":
        v["zeta"] = {
            "r,0": [r(1)[0], 0], "0,r": [0, r(1)[0]], "1,0": [1, 0], "w,0": [w, 0], "1/w,0": [pow(w, P - 2, P), 0],
            "7,0": [7, 0], "p-1,0": [P - 1, 0], "p+3,2^64-1": [P + 3, U64],
        }[what]
    else:
        assert case == "random"
    return v


def _verifier_applies(zeta, degree_bits, rate_bits):
    """orc_verify_forced divides by n (zeta - 1), x - zeta and x - g zeta, x on the LDE coset 7 <w_N>: its verdict is asserted
    only for zeta outside H and outside that coset (elsewhere the proofs are compared word for word and nothing more)"""
    z0, z1 = zeta[0] % P, zeta[1] % P
    if z1:
        return True
    n = 1 << degree_bits
    in_h = pow(z0, n, P) == 1
    in_coset = pow(z0 * pow(7, P - 2, P) % P, n << rate_bits, P) == 1
    return not (in_h or in_coset)


FULL_CASES = (["random"]
              + ["alpha:" + s for s in ("0,r", "r,0", "0,0", "1,p-1", "p,p+1", "2^32-1,2^32", "2^64-1,r")]
              # beta = 0 and gamma = p - 1 in separate cases: w + gamma = 0 for a wire holding 1
              + ["beta_gamma:" + s for s in ("0,r", "1,r", "p-1,r", "r,0", "r,p-1", "p+5,2^64-1")]
              + ["zeta:" + s for s in ("r,0", "0,r", "1,0", "w,0", "1/w,0", "7,0", "p-1,0", "p+3,2^64-1")])
REDUCED_CASES = ["random", "alpha:0,r", "alpha:0,0", "beta_gamma:0,r", "zeta:r,0", "alpha:p,p+1", "beta_gamma:p+5,2^64-1", "zeta:p+3,2^64-1"]
PARITY_CIRCUITS = [cid for cid in CIRCUITS if cid not in ("A3", "A4")]
ALL_CASES = [("A", c) for c in FULL_CASES] + [(cid, c) for cid in PARITY_CIRCUITS if cid != "A" for c in REDUCED_CASES]
CASE_IDS = ["%s-%s" % cc for cc in ALL_CASES]


# ------------------------------------------------------------------ the reference, computed once per (circuit, case)

class _Rig:
    """circuits, their oracle handles and the oracle's forced proofs, made on first use and shared by the CPU and GPU tests"""

    def __init__(self, oracle):
        self.oracle, self.circuits, self.proofs, self.gpu = oracle, {}, {}, {}

    def circuit(self, cid):
        if cid not in self.circuits:
            import eth_lc_plonky2_amd as m
            circ, wires, pis = CIRCUITS[cid](m)
            self.circuits[cid] = (circ, wires, pis, oracle_lib.OracleCircuit(self.oracle, circ))
        return self.circuits[cid]

    def values(self, cid, case):
        p = self.circuit(cid)[0].params
        return _case_values(case, p.num_challenges, p.degree_bits)

    def oracle_proof(self, cid, case):
        """(status, proof) of orc_prove_forced; never modified by a test"""
        if (cid, case) not in self.proofs:
            _, wires, pis, oc = self.circuit(cid)
            rc, proof = oc.prove_forced(wires, pis, **self.values(cid, case))
            proof.flags.writeable = False
            self.proofs[(cid, case)] = (rc, proof)
        return self.proofs[(cid, case)]

    def gpu_data(self, gpu_ctx, cid):
        if cid not in self.gpu:
            import eth_lc_plonky2_amd as m
            self.gpu[cid] = m.CircuitData.build(gpu_ctx, self.circuit(cid)[0])
        return self.gpu[cid]

    def close(self):
        for d in self.gpu.values():
            d.close()
        for c in self.circuits.values():
            c[3].close()


@pytest.fixture(scope="module")
def rig(oracle):
    r = _Rig(oracle)
    yield r
    r.close()


def _tampered(m, params, proof):
    """the proof with one word of the quotient openings changed"""
    bad = np.array(proof, dtype=np.uint64)
    bad[m.proof_layout(params).op_quotient] ^= np.uint64(1)
    return bad


# ------------------------------------------------------------------ CPU: the forced path of the oracle is a reference, so it is pinned itself

@pytest.mark.parametrize("cid", ["A", "A3", "D_q3_rate2"])
def test_forcing_the_transcripts_own_values_reproduces_orc_prove(oracle, rig, cid):
    """each mask bit alone and all four together, with the values orc_prove drew: the same proof word for word, the same
    recorded challenges, and orc_verify_forced accepts it (as does orc_verify)"""
    circ, wires, pis, oc = rig.circuit(cid)
    ch_n = circ.params.num_challenges
    want = oc.prove(wires, pis)
    own = oc.challenges()
    own = {"betas": list(own.betas)[:ch_n], "gammas": list(own.gammas)[:ch_n], "alphas": list(own.alphas)[:ch_n], "zeta": list(own.zeta)}
    assert oc.verify(want, pis) == 0
    for kinds in (["betas"], ["gammas"], ["alphas"], ["zeta"], list(own)):
        forced = {k: own[k] for k in kinds}
        rc, got = oc.prove_forced(wires, pis, **forced)
        assert rc == 0, kinds
        assert (got == want).all(), kinds
        used = oc.challenges()
        assert [list(used.betas)[:ch_n], list(used.gammas)[:ch_n], list(used.alphas)[:ch_n], list(used.zeta)] == list(own.values()), kinds
        assert oc.verify_forced(got, pis, **forced) == 0, kinds
    # and a forced value is what the proof is made with: another zeta gives other openings, which only the forced verifier accepts
    other = {"zeta": [own["zeta"][0] ^ 1, own["zeta"][1]]}
    rc, got = oc.prove_forced(wires, pis, **other)
    assert rc == 0 and (got != want).any() and list(oc.challenges().zeta) == other["zeta"]
    assert oc.verify_forced(got, pis, **other) == 0 and oc.verify(got, pis) != 0
    # no mask: the plain prover
    rc, got = oc.prove_forced(wires, pis)
    assert rc == 0 and (got == want).all() and oc.verify_forced(got, pis) == 0


def _permutation_reference(circ, wires, betas, gammas):
    """wires_permutation_partial_products_and_zs from its definition (plonky2 plonk/prover.rs, plonk/permutation_argument), in
    Python integers: on row x = w^i the routed wires are cut into chunks of quotient_degree_factor, chunk k has the quotient
        q_k(x) = prod_{j in chunk k} (w_j(x) + beta k_j x + gamma) / (w_j(x) + beta sigma_j(x) + gamma),
    Z(1) = 1, the partial products are pp_k(x) = Z(x) q_0(x) .. q_k(x) for all chunks but the last, and Z(w x) = Z(x) prod_k q_k(x).
    Columns: Z of every challenge, then the partial products challenge by challenge."""
    p = circ.params
    n, nr, nc, q = 1 << p.degree_bits, p.num_routed_wires, p.num_constants, p.quotient_degree_factor
    nchunks = (nr + q - 1) // q
    w = _root_of_unity(p.degree_bits)
    k_is = [int(k) % P for k in circ.k_is]
    zs, pps = [], []
    for beta, gamma in zip(betas, gammas):
        beta, gamma = beta % P, gamma % P
        z, x = 1, 1
        z_col, pp_cols = [], [[] for _ in range(nchunks - 1)]
        for i in range(n):
            z_col.append(z)
            acc = z
            for k in range(nchunks):
                for j in range(k * q, min((k + 1) * q, nr)):
                    wv, sg = int(wires[j, i]) % P, int(circ.constants_sigmas[nc + j, i]) % P
                    den = (wv + beta * sg + gamma) % P
                    assert den, "the reference needs non-zero denominators"
                    acc = acc * (wv + beta * k_is[j] * x + gamma) % P * pow(den, P - 2, P) % P
                if k < nchunks - 1:
                    pp_cols[k].append(acc)
            z, x = acc, x * w % P
        assert z == 1, "the permutation product returns to 1 on a satisfied circuit"
        zs.append(z_col)
        pps.extend(pp_cols)
    return np.array(zs + pps, dtype=np.uint64)


BETA_GAMMA_CASES = [c for c in FULL_CASES if c.startswith("beta_gamma:")]


@pytest.mark.parametrize("case", BETA_GAMMA_CASES)
def test_forced_zs_cap_equals_an_independent_permutation_reference(oracle, case):
    """2^5 rows: Z and the partial products from the definition, committed with the oracle's primitives, give the Zs cap of the
    forced proof (nothing of plonk.c's prover is called for the reference side)"""
    import eth_lc_plonky2_amd as m
    params = m.standard_params(5, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=1205)
    assert oracle.orc_gl_root_of_unity(5) == _root_of_unity(5)
    v = _case_values(case, 2, 5)
    oc = oracle_lib.OracleCircuit(oracle, circ)
    rc, proof = oc.prove_forced(wires, pis, betas=v["betas"], gammas=v["gammas"])
    oc.close()
    assert rc == 0
    values = _permutation_reference(circ, wires, v["betas"], v["gammas"])
    assert values.shape == (2 * (1 + 9), 32)
    if case == "beta_gamma:0,r":
        assert (values == 1).all()  # beta = 0: numerator = denominator everywhere
    _, _, cap = oracle_lib.commit_reference(oracle, values, params.rate_bits, params.cap_height)
    capw = 4 << params.cap_height
    assert (cap.ravel() == proof[capw:2 * capw]).all()


@pytest.mark.parametrize("alphas", [(0, 0), (0, None), (None, 0)])
def test_alpha_zero_proof_satisfies_the_identity_at_zeta(oracle, rig, alphas):
    """alpha = 0 keeps the first term alone, L_0 (Z_0 - 1) (and with a non-zero alpha in the other slot the whole combination
    there): orc_verify_forced under the same mask checks exactly that identity at zeta, accepts the proof and rejects it after
    one word of the quotient openings changed; the plain verifier (other alphas) rejects it at the identity"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, oc = rig.circuit("A")
    forced = {"alphas": [0 if a == 0 else 0x123456789ABCDEF for a in alphas]}
    rc, proof = oc.prove_forced(wires, pis, **forced)
    assert rc == 0 and list(oc.challenges().alphas)[:2] == forced["alphas"]
    assert oc.verify_forced(proof, pis, **forced) == 0
    assert oc.verify_forced(_tampered(m, circ.params, proof), pis, **forced) != 0
    assert oc.verify(proof, pis) == 3  # the transcript's own alphas: same transcript, the vanishing identity fails


def test_zero_denominator_is_an_error_on_the_forced_path(oracle, rig):
    """gamma solved from one cell so that w + beta sigma + gamma = 0 there: ORC_E_ZERO_DENOMINATOR (plonky2 panics), in either
    challenge slot; one off, the proof goes through; orc_prove itself is as before"""
    circ, wires, pis, oc = rig.circuit("A")
    nc = circ.params.num_constants
    beta = [0x1122334455667788 % P, 0x99AABBCCDDEEFF % P]
    for slot, (col, row) in enumerate([(17, 41), (79, 63)]):
        gamma = [5, 6]
        gamma[slot] = -(int(wires[col, row]) + beta[slot] * int(circ.constants_sigmas[nc + col, row])) % P
        rc, _ = oc.prove_forced(wires, pis, betas=beta, gammas=gamma)
        assert rc == oracle_lib.E_ZERO_DENOMINATOR, slot
        gamma[slot] = (gamma[slot] + 1) % P
        rc, proof = oc.prove_forced(wires, pis, betas=beta, gammas=gamma)
        assert rc == 0 and oc.verify_forced(proof, pis, betas=beta, gammas=gamma) == 0, slot
    rc, proof = oc.try_prove(wires, pis)
    assert rc == 0 and oc.verify(proof, pis) == 0


@pytest.mark.parametrize("cid,case", ALL_CASES, ids=CASE_IDS)
def test_oracle_proves_every_listed_case(rig, cid, case):
    """orc_prove_forced returns 0 for every case the GPU tests use (no zero denominator, the quotient fits), and its own
    verifier accepts the proof and rejects a changed quotient opening wherever it applies"""
    import eth_lc_plonky2_amd as m
    circ, _, pis, oc = rig.circuit(cid)
    rc, proof = rig.oracle_proof(cid, case)
    assert rc == 0
    v = rig.values(cid, case)
    if _verifier_applies(v["zeta"], circ.params.degree_bits, circ.params.rate_bits):
        assert oc.verify_forced(proof, pis, **v) == 0
        assert oc.verify_forced(_tampered(m, circ.params, proof), pis, **v) != 0
    else:
        assert case in ("zeta:1,0", "zeta:w,0", "zeta:1/w,0", "zeta:7,0", "zeta:p-1,0")


def test_case_list_is_the_one_the_stages_need():
    """the edge values are what they are named: canonical forms, membership in H and in the coset"""
    v = _case_values("zeta:1/w,0", 2, 6)
    assert v["zeta"][0] * _root_of_unity(6) % P == 1            # g zeta = 1
    assert not _verifier_applies(v["zeta"], 6, 3) and not _verifier_applies([7, 0], 6, 3) and not _verifier_applies([P - 1, 0], 6, 3)
    assert _verifier_applies([P + 3, U64], 6, 3) and _verifier_applies([5, 0], 6, 3) and _verifier_applies([0, 5], 6, 3)
    assert [a % P for a in _case_values("alpha:p,p+1", 4, 6)["alphas"]] == [0, 1, (1 << 32) - 2, 2]
    assert [a % P for a in _case_values("zeta:p+3,2^64-1", 2, 6)["zeta"]] == [3, (1 << 32) - 2]
    assert _case_values("beta_gamma:p+5,2^64-1", 3, 6)["betas"] == [P + 5] * 3
    for ch in (1, 3, 4):
        assert _case_values("alpha:0,r", ch, 6)["alphas"][0] == 0 and all(_case_values("alpha:0,r", ch, 6)["alphas"][1:])
    assert len(ALL_CASES) == len(FULL_CASES) + 6 * len(REDUCED_CASES) and len(set(ALL_CASES)) == len(ALL_CASES)


@pytest.mark.parametrize("ch", [3, 4])
def test_three_and_four_challenges_are_refused_by_the_library(oracle, rig, ch):
    """the oracle proves and verifies with 3 and 4 challenge slots (forced and not); the library's shape check, shared by
    lcp2_circuit_create, lcp2_verifier_create, lcp2_proof_words and lcp2_proof_layout_of, takes 1 or 2 (QUOTIENT_MAX_CH)"""
    import ctypes
    import eth_lc_plonky2_amd as m
    circ, wires, pis, oc = rig.circuit("A%d" % ch)
    v = rig.values("A%d" % ch, "alpha:0,r")
    rc, proof = oc.prove_forced(wires, pis, **v)
    assert rc == 0 and oc.verify_forced(proof, pis, **v) == 0
    assert m.load_library().lcp2_proof_words(ctypes.byref(circ.params)) == 0
    with pytest.raises(m.Lcp2Error) as e:
        m.CircuitData.verifier_only(circ, *oc.digest())
    assert e.value.status in (E_INVALID, E_UNSUPPORTED)
    with pytest.raises(m.Lcp2Error):
        m.proof_layout(circ.params)


# ------------------------------------------------------------------ GPU: the seams under the same challenges

def _u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


def _gpu_transcript(m, oracle, data, wires, pis):
    """the wires committed, and the transcript after observing digest, public-input hash and the wires cap, exactly as
    test_gpu_prover.test_staged_seams_compose_to_prove runs it"""
    capw = 4 << data.circ.params.cap_height
    proof = np.zeros(data.proof_words, dtype=np.uint64)
    digest, _ = data.digest()
    pi_hash = np.zeros(4, dtype=np.uint64)
    p = np.asarray(pis, dtype=np.uint64)
    oracle.orc_hash_no_pad(oracle_lib.vp(p), len(p), oracle_lib.vp(pi_hash))
    t = Challenger(oracle)
    t.observe(digest)
    t.observe(pi_hash)
    proof[0:capw] = data.commit_wires(wires).ravel()
    t.observe(proof[0:capw])
    return proof, t, pi_hash


def _gpu_forced_proof(m, oracle, data, wires, pis, v, want):
    """drive commit_wires -> perm_zs -> quotient -> fri_open with a Python transcript; after each draw the drawn value is
    replaced by the forced one.  Compared with the oracle's proof `want` stage by stage, so that a failure names the stage."""
    params = data.circ.params
    capw, ch = 4 << params.cap_height, params.num_challenges
    proof, t, pi_hash = _gpu_transcript(m, oracle, data, wires, pis)
    assert (proof[0:capw] == want[0:capw]).all(), "wires cap"
    t.get(ch), t.get(ch)                                    # betas, gammas: drawn ...
    proof[capw:2 * capw] = data.perm_zs(_u64(v["betas"]), _u64(v["gammas"])).ravel()   # ... and replaced
    assert (proof[capw:2 * capw] == want[capw:2 * capw]).all(), "Zs cap (permutation stage, K5)"
    t.observe(proof[capw:2 * capw])
    t.get(ch)                                               # alphas
    proof[2 * capw:3 * capw] = data.quotient(_u64(v["alphas"]), pi_hash).ravel()
    assert (proof[2 * capw:3 * capw] == want[2 * capw:3 * capw]).all(), "quotient cap (quotient stage, K6)"
    t.observe(proof[2 * capw:3 * capw])
    t.get(2)                                                # zeta
    data.fri_open(_u64(v["zeta"]), t.state(m), proof)
    assert first_mismatch(m, params, proof, want) is None, "opening stage (K7-K9): " + first_mismatch(m, params, proof, want)
    return proof


@pytest.mark.gpu
@pytest.mark.parametrize("cid,case", ALL_CASES, ids=CASE_IDS)
def test_gpu_seams_equal_the_oracle_under_forced_challenges(gpu_ctx, oracle, rig, cid, case):
    import eth_lc_plonky2_amd as m
    circ, wires, pis, oc = rig.circuit(cid)
    rc, want = rig.oracle_proof(cid, case)
    assert rc == 0
    v = rig.values(cid, case)
    data = rig.gpu_data(gpu_ctx, cid)
    got = _gpu_forced_proof(m, oracle, data, wires, pis, v, want)
    if _verifier_applies(v["zeta"], circ.params.degree_bits, circ.params.rate_bits):
        assert oc.verify_forced(got, pis, **v) == 0
        assert oc.verify_forced(_tampered(m, circ.params, got), pis, **v) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [0, 3, 4, 5])
def test_circuit_create_takes_one_or_two_challenges(gpu_ctx, ch):
    """lcp2_circuit_create refuses every challenge count but 1 and 2 with LCP2_E_UNSUPPORTED and says which parameter it is"""
    import eth_lc_plonky2_amd as m
    circ, _, _ = _synthetic(ch)(m)
    with pytest.raises(m.Lcp2Error) as e:
        m.CircuitData.build(gpu_ctx, circ)
    assert e.value.status == E_UNSUPPORTED and "num_challenges" in str(e.value)


@pytest.mark.gpu
def test_zeta_zero_is_refused_and_the_handle_proves_on(gpu_ctx, oracle, rig):
    """zeta = 0 (also as (p, p), and g zeta = 0 is the same condition) is LCP2_E_INVALID with a message from lcp2_fri_open and
    lcp2_fri_open_begin, nothing is written; the same handle then finishes the same proof with another zeta - the oracle's
    proof word for word - and proves normally"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, oc = rig.circuit("A")
    rc, want = rig.oracle_proof("A", "random")
    assert rc == 0
    v = rig.values("A", "random")
    data = rig.gpu_data(gpu_ctx, "A")
    capw = 4 << circ.params.cap_height
    proof, t, pi_hash = _gpu_transcript(m, oracle, data, wires, pis)
    t.get(2), t.get(2)
    proof[capw:2 * capw] = data.perm_zs(_u64(v["betas"]), _u64(v["gammas"])).ravel()
    t.observe(proof[capw:2 * capw])
    t.get(2)
    proof[2 * capw:3 * capw] = data.quotient(_u64(v["alphas"]), pi_hash).ravel()
    t.observe(proof[2 * capw:3 * capw])
    t.get(2)
    for zero in ([0, 0], [P, P], [P, 0]):
        for call in (data.fri_open, data.fri_open_begin):
            before = proof.copy()
            with pytest.raises(m.Lcp2Error) as e:
                call(_u64(zero), t.state(m), proof)
            assert e.value.status == E_INVALID and "zeta = 0" in str(e.value), zero
            assert (proof == before).all()
    with pytest.raises(m.Lcp2Error):   # the refused begin left no phase behind
        data.fri_open_commit(proof)
    data.fri_open(_u64(v["zeta"]), t.state(m), proof)
    assert first_mismatch(m, circ.params, proof, want) is None, first_mismatch(m, circ.params, proof, want)
    got = data.prove(wires, pis)
    assert (got == oc.prove(wires, pis)).all()
    data.verify(got, pis)
