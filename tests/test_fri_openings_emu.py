"""Openings of bare oracles on the CPU: the layout (numpy model, lcp2_fri_openings_words and the shared offset function agree), the
portable composition and division of csrc/fri_openings.hpp against the definition and against verify_query.hpp's formula for the two
batches of a Plonk proof, lcp2_fri_verify_openings against the independent verifier of eth_lc_plonky2_amd.fri_openings on proofs the
model assembles (verdict and failed check, also after every one-word change), and the refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

import openings_cases as oc
from rows_lib import vp

P = oc.P


@pytest.fixture(scope="module")
def m():
    import eth_lc_plonky2_amd as mod
    return mod


def ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


# ---- extension arithmetic through the oracle's field functions
def x_mul(L, a, b):
    o, aa, bb = np.zeros(2, dtype=np.uint64), np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)
    L.orc_gl2_mul(vp(aa), vp(bb), vp(o))
    return int(o[0]), int(o[1])


def x_inv(L, a):
    o, aa = np.zeros(2, dtype=np.uint64), np.array(a, dtype=np.uint64)
    L.orc_gl2_inv(vp(aa), vp(o))
    return int(o[0]), int(o[1])


def x_add(L, a, b):
    return L.orc_gl_add(a[0], b[0]), L.orc_gl_add(a[1], b[1])


def x_sub(L, a, b):
    return L.orc_gl_sub(a[0], b[0]), L.orc_gl_sub(a[1], b[1])


def x_horner(L, coeffs, x):
    acc = (0, 0)
    for c in coeffs[::-1]:
        acc = x_add(L, x_mul(L, acc, x), c)
    return acc


@pytest.mark.parametrize("name", list(oc.CASES))
def test_layout_agrees(m, name):
    from eth_lc_plonky2_amd import fri_openings as fo
    c = oc.case(name)
    L = fo.layout(c.cfg, c.log_n, c.cols, c.points_ranges)
    cols = np.array(c.cols, dtype=np.uint32)
    assert m.fri_openings_words(c.cfg, c.log_n, c.cols, c.inst) == L.total == oc.emu().emu_open_words(ctypes.byref(c.cfg), c.log_n, vp(cols), ctypes.byref(c.inst))
    out = np.zeros(48, dtype=np.uint64)
    assert oc.emu().emu_open_layout(ctypes.byref(c.cfg), c.log_n, vp(cols), ctypes.byref(c.inst), vp(out)) == 0
    o = [int(v) for v in out]
    assert o[:8] == [L.total, L.fri_caps, L.queries, L.query_words, L.final_poly, L.pow_witness, L.final_len, L.init_sib]
    assert o[8:8 + len(L.point_off)] == L.point_off and o[12:12 + len(c.cols)] == L.init_off
    assert o[20:20 + len(L.arity)] == L.step_off and o[28:28 + len(L.arity)] == L.step_sib
    assert o[36:36 + len(L.point_polys)] == L.point_polys and o[40:40 + len(c.cols)] == c.cols
    # the sections tile the proof
    at = 0
    for _, first, words in fo.sections(L):
        assert first == at
        at += words
    assert at == L.total


def composed(c, coeffs, alpha, pts):
    n = 1 << c.log_n
    out0, out1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    cols = np.array(c.cols, dtype=np.uint32)
    flat = np.array([w for z in pts for w in z], dtype=np.uint64)
    assert oc.emu().emu_open_compose(ctypes.byref(c.inst), vp(cols), ptrs(coeffs), c.log_n, vp(np.array(alpha, dtype=np.uint64)), vp(flat), vp(out0), vp(out1)) == 0
    return [(int(a), int(b)) for a, b in zip(out0, out1)]


@pytest.mark.parametrize("name", ["1_zero_layers", "2_two_oracles", "3_overlap", "5_maxima", "6_two_arities"])
@pytest.mark.parametrize("kind", oc.POINT_KINDS)
def test_compose_and_divide_give_the_batch_combination(oracle, name, kind):
    """F(x) = sum_b alpha^(polynomials of the batches after b) (C_b(x) - C_b(zeta_b)) / (x - zeta_b) at random x"""
    c = oc.case(name)
    coeffs, pts = oc.coefficients(c), oc.points(c, kind)
    rng = np.random.default_rng(c.seed)
    alpha = (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    F = composed(c, coeffs, alpha, pts)
    assert all(a < P and b < P for a, b in F)
    for _ in range(3):
        x = (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
        want = (0, 0)
        for b, ranges in enumerate(c.points_ranges):
            polys = [[(int(v), 0) for v in coeffs[o][first + j]] for (o, first, count) in ranges for j in range(count)]
            at_x = x_horner(oracle, [x_horner(oracle, p, x) for p in polys], alpha)
            at_z = x_horner(oracle, [x_horner(oracle, p, pts[b]) for p in polys], alpha)
            shift = (1, 0)
            for _k in polys:
                shift = x_mul(oracle, shift, alpha)
            want = x_add(oracle, x_mul(oracle, want, shift), x_mul(oracle, x_sub(oracle, at_x, at_z), x_inv(oracle, x_sub(oracle, x, pts[b]))))
        assert x_horner(oracle, F, x) == want


def test_plonk_shape_equals_the_formula_of_verify_query(oracle):
    """two batches, the second the first CH columns of the third oracle at g zeta: the composed polynomial at a base-field x is what
    vq_combine_initial (csrc/verify_query.hpp) makes of the four leaves for the same alpha, zeta and reduced openings"""
    c = oc.case("4_plonk_shape")
    coeffs = oc.coefficients(c)
    rng = np.random.default_rng(5)
    zeta = (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    g = oracle.orc_gl_root_of_unity(c.log_n)
    g_zeta = (oracle.orc_gl_mul(zeta[0], g), oracle.orc_gl_mul(zeta[1], g))
    alpha = (int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    F = composed(c, coeffs, alpha, [zeta, g_zeta])
    all_polys = [[(int(v), 0) for v in col] for o in range(4) for col in coeffs[o]]
    zs = [[(int(v), 0) for v in col] for col in coeffs[2][:2]]
    red0 = x_horner(oracle, [x_horner(oracle, p, zeta) for p in all_polys], alpha)
    red1 = x_horner(oracle, [x_horner(oracle, p, g_zeta) for p in zs], alpha)
    for _ in range(3):
        x = int(rng.integers(1, P, dtype=np.uint64))
        leaves = np.array([x_horner(oracle, p, (x, 0))[0] for p in all_polys], dtype=np.uint64)
        out = np.zeros(2, dtype=np.uint64)
        A = lambda v: vp(np.array(v, dtype=np.uint64))
        oc.emu().emu_open_vq_combine(vp(np.array(c.cols, dtype=np.uint32)), 2, vp(leaves), A(alpha), A(zeta), A(g_zeta), A(red0), A(red1), x, vp(out))
        assert x_horner(oracle, F, (x, 0)) == (int(out[0]), int(out[1]))


# ---- the verifier against the model
SMALL = {  # log_n 2 and 3: (log_n, rate_bits, cap_height, columns, points -> ranges, schedule, pow bits, queries)
    "log_n_2": (2, 1, 0, [2, 1], [[(0, 0, 2), (1, 0, 1)], [(0, 1, 1)]], [1], 2, 3),
    "log_n_3": (3, 1, 1, [3, 2], [[(0, 0, 3), (1, 0, 2)], [(1, 1, 1)]], [1, 1], 3, 3),
}


def small_proof(m, name, pts=None, seed=1):
    from eth_lc_plonky2_amd import fri_openings as fo
    log_n, rate, cap, cols, pr, schedule, pow_bits, queries = SMALL[name]
    cfg = m.fri_config(log_n, rate, cap, pow_bits, queries, 1, log_n, schedule=schedule)
    rng = np.random.default_rng(seed)
    coeffs = [[[int(v) for v in rng.integers(0, P, 1 << log_n, dtype=np.uint64)] for _ in range(k)] for k in cols]
    pts = pts or [(int(rng.integers(1, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64))) for _ in pr]
    ch = fo.Challenger()
    ch.observe([seed, 3])
    proof, caps = fo.prove(coeffs, cfg, log_n, pr, pts, ch)
    return dict(cfg=cfg, log_n=log_n, cols=cols, pr=pr, pts=pts, proof=proof, caps=caps, inst=m.fri_instance(len(cols), pr), seed=seed, after=ch.words())


def verdicts(m, s, proof, caps=None, pts=None, seed=None):
    """(library, harness, model): each the failed check, 0 if accepted; the outgoing transcripts are compared where all accept"""
    from eth_lc_plonky2_amd import fri_openings as fo
    caps, pts, seed = caps or s["caps"], pts or s["pts"], s["seed"] if seed is None else seed
    c1, c2, c3 = m.binding.Challenger(), m.binding.Challenger(), fo.Challenger()
    for c in (c1, c2, c3):
        c.observe([seed, 3])
    lib = m.fri_verify_openings(caps, s["cols"], s["log_n"], s["inst"], pts, s["cfg"], c1.state, proof)
    failed = ctypes.c_int(0)
    flat = np.array([w for z in pts for w in z], dtype=np.uint64)
    rc = oc.emu().emu_open_verify(ptrs(caps), vp(np.array(s["cols"], dtype=np.uint32)), s["log_n"], ctypes.byref(s["inst"]), vp(flat), ctypes.byref(s["cfg"]),
                                  ctypes.byref(c2.state), vp(np.ascontiguousarray(proof)), proof.size, ctypes.byref(failed))
    assert rc in (0, -7) and (rc == 0) == (failed.value == 0)
    model = fo.verify(caps, s["cfg"], s["log_n"], s["cols"], s["pr"], pts, c3, proof)
    if lib == 0:
        assert fo.state_words(c1.state) == fo.state_words(c2.state) == c3.words()
    return lib, failed.value, model


@pytest.mark.parametrize("name", list(SMALL))
def test_verifier_agrees_with_the_model_on_every_one_word_change(m, name):
    s = small_proof(m, name)
    assert verdicts(m, s, s["proof"]) == (0, 0, 0)
    seen = set()
    for w in range(s["proof"].size):
        bad = s["proof"].copy()
        bad[w] = (int(bad[w]) + 1) % P
        v = verdicts(m, s, bad)
        assert v[0] == v[1] == v[2] != 0, (w, v)
        seen.add(v[0])
        if int(s["proof"][w]) < (1 << 64) - P:
            bad[w] = int(s["proof"][w]) + P
            assert verdicts(m, s, bad) == (1, 1, 1), w
    assert {3, 5} <= seen and (seen & {2, 4, 6})  # (a changed final polynomial moves the transcript: it mostly fails the proof of work first)
    # a word of a cap, a point, the incoming transcript
    caps = [c.copy() for c in s["caps"]]
    caps[-1][1] = (int(caps[-1][1]) + 1) % P
    v = verdicts(m, s, s["proof"], caps=caps)
    assert v[0] == v[1] == v[2] == 3
    pts = list(s["pts"])
    pts[0] = ((pts[0][0] + 1) % P, pts[0][1])
    v = verdicts(m, s, s["proof"], pts=pts)
    assert v[0] == v[1] == v[2] != 0
    v = verdicts(m, s, s["proof"], seed=s["seed"] + 1)
    assert v[0] == v[1] == v[2] != 0


def test_a_query_at_an_opened_point_is_check_7(m):
    """a point ON the LDE coset: the prover's division is exact there, the verifier cannot divide where a query lands on it"""
    from eth_lc_plonky2_amd import fri_openings as fo
    log_n, rate = SMALL["log_n_2"][0], SMALL["log_n_2"][1]
    hit = None
    for k in range(1 << (log_n + rate)):   # the first coset point that a query of its own proof lands on (seeded: always the same)
        x = fo.GENERATOR * pow(fo.root_of_unity(log_n + rate), k, P) % P
        s = small_proof(m, "log_n_2", pts=[(x, 0), (12345, 678)])
        c = fo.Challenger()
        c.observe([s["seed"], 3])
        idx = fo.query_indices(s["cfg"], s["log_n"], s["cols"], s["pr"], c, s["proof"])
        if any(fo.query_points(fo.layout(s["cfg"], s["log_n"], s["cols"], s["pr"]), i) == x for i in idx):
            hit = s
            break
    assert hit is not None
    assert verdicts(m, hit, hit["proof"]) == (7, 7, 7)


def test_refusals(m):
    s = small_proof(m, "log_n_3")
    words = s["proof"].size
    lib = m.load_library()
    ok = lambda inst, cfg=s["cfg"], cols=s["cols"]: m.fri_openings_words(cfg, s["log_n"], cols, inst)
    assert ok(s["inst"]) == words

    def refused(inst, cfg=None, cols=None, pts=None, proof=None):
        ch = m.binding.Challenger()
        with pytest.raises(m.Lcp2Error) as e:
            m.fri_verify_openings(s["caps"] if cols is None else s["caps"] * 5, s["cols"] if cols is None else cols, s["log_n"], inst, pts or s["pts"] * 3,
                                  cfg or s["cfg"], ch.state, s["proof"] if proof is None else proof)
        assert e.value.status == -1
        assert list(ch.state.sponge) == [0] * 12 and ch.state.input_len == 0   # the transcript was not touched
        return True

    past = m.fri_instance(2, [[(0, 0, 3), (1, 0, 3)], [(1, 1, 1)]])          # oracle 1 has 2 columns
    past2 = m.fri_instance(2, [[(0, 2, 2), (1, 0, 2)], [(1, 1, 1)]])         # first_poly + num_polys past oracle 0
    no_range = m.fri_instance(2, [[(0, 0, 3), (1, 0, 2)], []])
    empty_range = m.fri_instance(2, [[(0, 0, 3), (1, 0, 0)], [(1, 1, 1)]])
    bad_oracle = m.fri_instance(2, [[(0, 0, 3), (2, 0, 1)], [(1, 1, 1)]])
    five_points = m.fri_instance(2, [[(0, 0, 1)]] * 5)
    nine_oracles = m.fri_instance(9, [[(0, 0, 1)]])
    for inst in (past, past2, no_range, empty_range, bad_oracle, five_points):
        assert ok(inst) == 0 and refused(inst)
    assert ok(nine_oracles, cols=[1] * 9) == 0 and refused(nine_oracles, cols=[1] * 9)
    # configs the shape does not fit: a cap above the tree, a schedule that folds below the cap or past the polynomial, 65 queries
    for change in (dict(cap_height=5), dict(schedule=[1, 1, 1, 1]), dict(schedule=[6]), dict(queries=65), dict(queries=0), dict(pow_bits=41)):
        cfg = m.fri_config(3, 1, change.get("cap_height", 1), change.get("pow_bits", 3), change.get("queries", 3), 1, 3, schedule=change.get("schedule", [1, 1]))
        assert ok(s["inst"], cfg=cfg) == 0 and refused(s["inst"], cfg=cfg)
    # the same schedule with another cap height: a valid config, but not this proof's length
    other = m.fri_config(3, 1, 0, 3, 3, 1, 3, schedule=[1, 1])
    assert ok(s["inst"], cfg=other) not in (0, words) and refused(s["inst"], cfg=other)
    assert refused(s["inst"], proof=s["proof"][:-1]) and refused(s["inst"], proof=np.concatenate([s["proof"], s["proof"][:1]]))
    assert refused(s["inst"], pts=[(0, 0), s["pts"][1]]) and refused(s["inst"], pts=[s["pts"][0], (P, P)])   # zeta = 0, also as p
    # lcp2_fri_config_of: the refusals of lcp2_params_config
    cfg = m.FriConfig()
    assert lib.lcp2_fri_config_of(0, 3, 4, 16, 28, 4, 5, ctypes.byref(cfg)) == -1 and lib.lcp2_fri_config_of(5, 9, 4, 16, 28, 4, 5, ctypes.byref(cfg)) == -1
    assert lib.lcp2_fri_config_of(5, 3, 4, 16, 28, 6, 5, ctypes.byref(cfg)) == -1 and lib.lcp2_fri_config_of(28, 3, 4, 16, 28, 1, 5, ctypes.byref(cfg)) == -6
    p = m.params_config(19, 4, 3, 4, 16, 28, 4, 5)
    cfg = m.fri_config(19)
    assert cfg.num_fri_layers == p.num_fri_layers and list(cfg.fri_arity_bits) == list(p.fri_arity_bits)
