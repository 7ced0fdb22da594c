"""The low-degree extension, the commitment and its openings at every rate, not only 8 (rate_bits 3).

The first pass of NttHost::forward depends on the coset count nz = 2^rate_bits in its block mapping (k_ntt_pass / k_ntt_pass_pf,
csrc/kernels_ntt.hip), in the layout of its coset-scale tables ([z][2^lg] one-level, [z][2^h] two-level, [z][16] for the computed
scale) and in the block bitrev(z) a coset is written to.  launch_rule restates which of these a shape takes, the shape lists below
reach every combination, and every result is compared word for word with the oracle's textbook transforms (tests/oracle_lib.py)
and, independently, with the polynomial evaluated at 7 * W^bitrev(i)."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from oracle_lib import P, bitrev_perm, commit_reference, lde_leaf_order, merkle_verify, rand_field, vp

PP = np.uint64(P)
Rule = namedtuple("Rule", "wgs nz mapping table prefetch")


def launch_rule(lg, ncols, rate):
    """The first pass of an LDE of ncols columns of 2^lg coefficients at rate_bits = rate, restated from csrc/ntt_host.hpp
    (NttHost::forward: wgs, nz, xcd_group; shift_table: the one-level table) and csrc/ntt.hpp (ntt_pf_slabs_per_wg; the strided
    shapes of ntt_pf_strided_s are the plans of lg 19 and 22)."""
    wgs, nz = 1 << max(lg - 13, 0), 1 << rate
    if nz == 1 or (wgs * ncols) % 8:
        mapping = 0
    elif wgs % 8 == 0:
        mapping = 2
    else:
        mapping = 1
    table = "direct" if 14 <= lg <= 22 else "two-level"
    total = wgs * ncols * nz
    prefetch = lg in (19, 22) and any(total % (8 * k) == 0 and total // k >= 2048 for k in (16, 8, 4, 2))
    return Rule(wgs, nz, mapping, table, prefetch)


ONE_SLAB = [(1, 1, 1), (3, 8, 2), (5, 3, 4), (9, 16, 5), (12, 5, 8), (13, 8, 1), (13, 3, 6), (4, 5, 7),
            (7, 2, 3)]  # rate 3 at a size the other files do not run: the list covers every rate from 0 to 8 on its own
MULTI_PASS = [(14, 2, 1), (15, 3, 2),                         # mapping 0
              (14, 4, 2), (15, 2, 4),                         # mapping 1
              (16, 1, 1), (16, 3, 4), (17, 2, 5), (18, 1, 2)]  # mapping 2
RATE_0 = [(10, 3, 0), (16, 2, 0)]
TWO_STRIDED = [(23, 1, 1)]
PARITY_SHAPES = ONE_SLAB + MULTI_PASS + RATE_0 + TWO_STRIDED
PREFETCH_SHAPES = [(19, 4, 4), (19, 32, 1), (22, 4, 1), (22, 1, 4)]
PREFETCH_ORACLE_BLOCKS = (0, 1, 5, 15)  # of the 16 leaf blocks of (22, 1, 4): cosets 0, 8, 10 and 15


def test_shape_lists_cover_every_rate_mapping_and_table():
    rules = {s: launch_rule(*s) for s in PARITY_SHAPES + PREFETCH_SHAPES}
    assert {s[2] for s in rules} >= set(range(9))
    assert {(r.mapping, r.table) for r in rules.values()} == {(m, t) for m in (0, 1, 2) for t in ("direct", "two-level")}
    assert len({r.nz for r in rules.values() if r.mapping == 2}) >= 4
    assert not any(rules[s].prefetch for s in PARITY_SHAPES)
    assert all(rules[s].prefetch for s in PREFETCH_SHAPES)
    assert {rules[s].nz for s in PREFETCH_SHAPES} == {2, 16}
    assert {s[0] for s in PREFETCH_SHAPES} == {19, 22}
    # the single-column calls the prefetching form is compared with take the plain kernel
    assert not any(launch_rule(lg, 1, rate).prefetch for lg, ncols, rate in PREFETCH_SHAPES if ncols > 1)
    # the groups are what their names say
    assert all(rules[s].wgs == 1 and rules[s].table == "two-level" for s in ONE_SLAB)
    assert [rules[s].mapping for s in MULTI_PASS] == [0, 0, 1, 1, 2, 2, 2, 2] and all(rules[s].table == "direct" for s in MULTI_PASS)
    assert all(rules[s] == Rule(1 << 10, 2, 2, "two-level", False) for s in TWO_STRIDED)
    # the rule itself at the shapes the other files run: the headline LDE and the light-client step (rate 3)
    assert launch_rule(22, 1, 3) == Rule(512, 8, 2, "direct", True) and launch_rule(19, 8, 3) == Rule(64, 8, 2, "direct", True)
    assert not launch_rule(19, 2, 3).prefetch and launch_rule(13, 7, 3).mapping == 0 and launch_rule(14, 3, 3).mapping == 0


def _assert_lde_equal(got, want, lg, ncols, rate):
    """word for word; a mismatch is reported by column, leaf block, coset and launch rule"""
    if (got == want).all():
        return
    col, i = (int(v[0]) for v in np.nonzero(got != want))
    block = i >> lg
    coset = int(format(block, "0%db" % rate)[::-1], 2) if rate else 0
    cols = sorted({int(c) for c in np.nonzero((got != want).any(axis=1))[0]})
    raise AssertionError(f"LDE differs: {int((got != want).sum())} words in columns {cols[:8]}; first at column {col}, leaf {i} "
                         f"(block {block} = coset {coset}, offset {i & ((1 << lg) - 1)}); {launch_rule(lg, ncols, rate)}")


def _root(bits):
    return pow(pow(7, (P - 1) >> 32, P), 1 << (32 - bits), P)  # plonky2's primitive 2^bits-th root of unity


def _leaf_points(lg, rate, more=()):
    """(i, 7 * W^bitrev(i)) for the first leaf, the last, one in the middle and the leaves of `more`"""
    bits, W = lg + rate, _root(lg + rate)
    N = 1 << bits
    idx = (0, N - 1, (N // 3) | 1) + tuple(more)
    return [(i, 7 * pow(W, int(format(i, "0%db" % bits)[::-1], 2), P) % P) for i in idx]


def _check_definition(gpu_ctx, coeffs, got, lg, ncols, rate, rng, more=()):
    """out[c, i] = poly_c(7 * W^bitrev(i)), independently of the oracle: Horner over the column up to 2^16 coefficients, above that
    a second call on polynomials with three non-zero coefficients (same shape, so the same kernels)"""
    n = 1 << lg
    if lg <= 16:
        c = ncols // 2
        cc = [int(v) % P for v in coeffs[c]]
        for i, x in _leaf_points(lg, rate):
            acc = 0
            for a in reversed(cc):
                acc = (acc * x + a) % P
            assert acc == int(got[c, i]), (c, i)
        return
    sp = np.zeros((ncols, n), dtype=np.uint64)
    terms = []
    for c in range(ncols):
        pos = [1, n // 2 + 3 + c, n - 1]
        val = [int(v) for v in rand_field(rng, 3, canonical=False)]
        val[2] = P + 5  # a non-canonical word at the last coefficient
        sp[c, pos] = np.array(val, dtype=np.uint64)
        terms.append(list(zip(pos, val)))
    out = gpu_ctx.lde_batch(sp, rate)
    for c in range(ncols):
        for i, x in _leaf_points(lg, rate, more):
            assert sum(v * pow(x, e, P) for e, v in terms[c]) % P == int(out[c, i]), (c, i)


@pytest.mark.gpu
@pytest.mark.parametrize("lg,ncols,rate", PARITY_SHAPES)
def test_lde_parity_over_rates(gpu_ctx, oracle, lg, ncols, rate):
    rng = np.random.default_rng(lg * 1000 + ncols * 16 + rate)
    c = rand_field(rng, (ncols, 1 << lg), canonical=False)
    got = gpu_ctx.lde_batch(c, rate)
    _assert_lde_equal(got, lde_leaf_order(oracle, c % PP, rate), lg, ncols, rate)
    if rate == 0:  # a coset NTT in leaf order
        assert (got == gpu_ctx.ntt_batch(c, shift=7)[:, bitrev_perm(lg)]).all()
    _check_definition(gpu_ctx, c, got, lg, ncols, rate, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("lg,ncols,rate", PREFETCH_SHAPES)
def test_lde_prefetching_form_over_rates(gpu_ctx, oracle, lg, ncols, rate):
    """k_ntt_pass_pf with gz = 2 and 16 cosets: its coords lambda and the [z][16] rows of the computed scale.  The kernel is not
    selected below 4096 slabs, so these are the size of test_lde_headline_size_parity.  Two columns against the oracle; the others
    against single-column calls, which stay below the slab threshold and take the plain kernel: the two forms check each other.
    The oracle's work stays at or below that test's one 2^25-point transform.  The single column of (22, 1, 4) would be a 2^26-point
    one, so it is compared leaf block by leaf block instead - block b is the coset NTT with shift 7 * W^bitrev(b), 2^22 points - over
    PREFETCH_ORACLE_BLOCKS, and the sparse-polynomial check of the definition reads one leaf of every other block."""
    rng = np.random.default_rng(lg * 1000 + ncols * 16 + rate)
    n = 1 << lg
    c = rand_field(rng, (ncols, n), canonical=False)
    got = gpu_ctx.lde_batch(c, rate)
    more = ()
    if ncols == 1:
        against_oracle = [0]
        W = _root(lg + rate)
        for b in PREFETCH_ORACLE_BLOCKS:
            shift = 7 * pow(W, int(format(b, "0%db" % rate)[::-1], 2), P) % P
            want = lde_leaf_order(oracle, c % PP, 0, shift)
            assert (got[:, b * n:(b + 1) * n] == want).all(), (b, int((got[:, b * n:(b + 1) * n] != want).sum()), launch_rule(lg, ncols, rate))
        more = tuple(b * n + (b * 262147 + 5) % n for b in range(1 << rate) if b not in PREFETCH_ORACLE_BLOCKS)
    else:
        against_oracle = [1, ncols - 1]
        want = lde_leaf_order(oracle, c[against_oracle] % PP, rate)
        for k, col in enumerate(against_oracle):
            _assert_lde_equal(got[col:col + 1], want[k:k + 1], lg, ncols, rate)
    del want
    for col in range(ncols):
        if col not in against_oracle:
            assert (got[col] == gpu_ctx.lde_batch(c[col:col + 1], rate)[0]).all(), (col, launch_rule(lg, ncols, rate))
    _check_definition(gpu_ctx, c, got, lg, ncols, rate, rng, more)


@pytest.mark.gpu
def test_size_one_transforms_return_canonical_words(gpu_ctx):
    """log_n = 0: the LDE of a constant is the constant in every word and the NTT is the identity - on the field element, so the
    words come back canonical as at every other size"""
    x = np.array([[0], [P - 1], [P + 5]], dtype=np.uint64)
    want = x % PP
    for rate in (0, 3):
        got = gpu_ctx.lde_batch(x, rate)
        assert got.shape == (3, 1 << rate) and (got == want).all()
    for inverse in (False, True):
        for shift in (1, 7):
            assert (gpu_ctx.ntt_batch(x, inverse=inverse, shift=shift) == want).all()


@pytest.mark.gpu
def test_ntt_batch_coset_shift_edges(gpu_ctx):
    import eth_lc_plonky2_amd as m
    x = rand_field(np.random.default_rng(77), (2, 1 << 6), canonical=False)
    assert (gpu_ctx.ntt_batch(x, shift=P + 7) == gpu_ctx.ntt_batch(x, shift=7)).all()
    assert (gpu_ctx.ntt_batch(x, inverse=True, shift=P + 7) == gpu_ctx.ntt_batch(x, inverse=True, shift=7)).all()
    for shift in (P, 0):
        for inverse in (False, True):
            with pytest.raises(m.Lcp2Error):
                gpu_ctx.ntt_batch(x, inverse=inverse, shift=shift)
    assert (gpu_ctx.ntt_batch(gpu_ctx.ntt_batch(x, shift=7), inverse=True, shift=7) == x % PP).all()  # the context still works


# ---------------------------------------------------------------- commitments and openings
def _check_openings(oracle, o, idx, lde, cap, first_leaf=0):
    """every opening: the leaf is the LDE row, the oracle's verifier accepts it at the global index and rejects it after one
    flipped leaf bit and after one flipped sibling word"""
    idx = np.asarray(idx, dtype=np.uint64)
    leaves, sib = o.open(idx)
    assert sib.shape[1] == o.log_n + o.rate_bits - o.cap_height
    for q, li in enumerate(idx):
        i = first_leaf + int(li)
        assert (leaves[q] == lde[:, i]).all(), i
        assert merkle_verify(oracle, leaves[q], i, sib[q], cap), i
        bad = leaves[q].copy()
        bad[q % bad.size] ^= np.uint64(1 << (q % 64))
        assert not merkle_verify(oracle, bad, i, sib[q], cap), i
        if sib.shape[1]:
            bs = sib[q].copy()
            bs[q % sib.shape[1], q % 4] ^= np.uint64(1 << ((7 * q) % 64))
            assert not merkle_verify(oracle, leaves[q], i, bs, cap), i


@pytest.mark.gpu
@pytest.mark.parametrize("lg,ncols,rate,cap_h", [(6, 9, 1, 0), (10, 20, 5, 2), (12, 135, 4, 4), (14, 3, 2, 16), (4, 5, 7, 4), (16, 2, 4, 4)])
def test_commit_and_open_over_rates(gpu_ctx, oracle, lg, ncols, rate, cap_h):
    import eth_lc_plonky2_amd as m
    rng = np.random.default_rng(lg * 1000 + ncols * 16 + rate)
    vals = rand_field(rng, (ncols, 1 << lg), canonical=False)
    coeffs, lde, cap = commit_reference(oracle, vals, rate, cap_h)
    N = 1 << (lg + rate)
    o = gpu_ctx.commit_values(vals, rate, cap_h)
    o2 = gpu_ctx.commit_coeffs(coeffs, rate, cap_h)
    for oc in (o, o2):
        assert (oc.cap == cap).all()
        gc, gl = oc.read()
        assert (gc == coeffs).all()
        _assert_lde_equal(gl, lde, lg, ncols, rate)
    _check_openings(oracle, o, [0, 1, N - 1, N // 3, N // 3], lde, cap)
    _check_openings(oracle, o, [N // 2 + 1], lde, cap)
    _check_openings(oracle, o2, [N - 2, 0], lde, cap)
    if (lg, ncols, rate, cap_h) == (10, 20, 5, 2):
        _check_openings(oracle, o, rng.integers(0, N, size=200, dtype=np.uint64), lde, cap)
    for bad in ([N], [0, N + 5, 1], [2 ** 64 - 1]):
        with pytest.raises(m.Lcp2Error):
            o.open(bad)
    _check_openings(oracle, o, [N - 1, 2], lde, cap)  # the oracle object still opens
    o.close()
    o2.close()


@pytest.fixture(scope="module")
def cosets_case(oracle):
    """(lg, ncols, rate) -> values, the oracle's coefficients and the oracle's LDE of them: computed once per shape, shared by the
    cap heights, left unchanged, freed with the module"""
    shared = {}

    def case(lg, ncols, rate):
        key = (lg, ncols, rate)
        if key not in shared:
            values = rand_field(np.random.default_rng(lg * 1000 + ncols * 16 + rate), (ncols, 1 << lg), canonical=False)
            coeffs = values % PP
            oracle.orc_ifft_batch(vp(coeffs), ncols, 1 << lg)
            want = lde_leaf_order(oracle, coeffs, rate)
            for a in (values, coeffs, want):
                a.setflags(write=False)
            shared[key] = values, coeffs, want
        return shared[key]

    yield case
    shared.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("cap_kind", ["rate", "rate+2", "lg+rate"])
@pytest.mark.parametrize("rate", [1, 2, 5])
@pytest.mark.parametrize("lg,ncols", [(10, 20), (16, 3)])
def test_commit_cosets_over_rates(gpu_ctx, oracle, cosets_case, lg, ncols, rate, cap_kind):
    """lcp2_commit_cosets (z_base = bitrev(b, rate_bits) per leaf block) at rates other than 3: the ranks of every split run one
    after the other; the assembled cap is the single-GPU cap, the blocks are slices of the full LDE and a local opening verifies
    against the global cap at the global leaf index"""
    import eth_lc_plonky2_amd as m
    n = 1 << lg
    cap_h = {"rate": rate, "rate+2": rate + 2, "lg+rate": lg + rate}[cap_kind]
    values, coeffs, want = cosets_case(lg, ncols, rate)
    full = gpu_ctx.commit_values(values, rate, cap_h)
    gc, lde = full.read()
    assert (gc == coeffs).all()
    _assert_lde_equal(lde, want, lg, ncols, rate)
    worlds = [w for w in (1, 2, 4, 8) if w <= min(1 << rate, 8)] + ([32] if rate == 5 else [])
    for world in worlds:
        caps = []
        for rank in range(world):
            first, count = m.parallel.block_range(rank, world, rate)
            o = gpu_ctx.commit_cosets(coeffs, first, count, rate, cap_h)
            caps.append(o.cap)
            _, part = o.read(coeffs=False)
            _assert_lde_equal(part, want[:, first * n:(first + count) * n], lg, ncols, rate)
            _check_openings(oracle, o, [(rank * 977 + (count * n) // 3) % (count * n)], want, full.cap, first_leaf=first * n)
            o.close()
        assert (np.concatenate(caps) == full.cap).all(), world
    full.close()


@pytest.mark.gpu
def test_commit_cosets_refusals(gpu_ctx, oracle):
    import eth_lc_plonky2_amd as m
    lg, ncols, rate = 6, 3, 5
    coeffs = rand_field(np.random.default_rng(65), (ncols, 1 << lg))

    def status(cap_h, first, count):
        h = ctypes.c_void_p()
        cap = np.zeros((max(count, 1) << max(cap_h - rate, 0), 4), dtype=np.uint64)
        rc = gpu_ctx.lib.lcp2_commit_cosets(gpu_ctx.handle, coeffs.ctypes.data_as(ctypes.c_void_p), ncols, lg, rate, cap_h, first, count,
                                            m.MEM_HOST, ctypes.byref(h), cap.ctypes.data_as(ctypes.c_void_p))
        assert (rc == 0) == bool(h.value)
        if h.value:
            gpu_ctx.lib.lcp2_oracle_destroy(h)
        return rc

    assert status(rate, 4, 4) == 0
    for cap_h, first, count in ((rate - 1, 0, 4), (0, 0, 32),             # cap_height < rate_bits
                                (lg + rate + 1, 0, 4),                     # above the tree
                                (rate, 2, 4), (rate, 1, 2), (rate, 30, 4),  # block_first not a multiple of block_count
                                (rate, 0, 3), (rate, 0, 6), (rate, 0, 0),  # block_count not a power of two
                                (rate, 32, 1), (rate, 0, 64)):             # beyond the 2^rate_bits blocks
        with pytest.raises(m.Lcp2Error):
            gpu_ctx._check(status(cap_h, first, count))
    # the context still commits afterwards
    o = gpu_ctx.commit_cosets(coeffs, 8, 2, rate, rate + 1)
    full = gpu_ctx.commit_coeffs(coeffs, rate, rate + 1)
    _check_openings(oracle, o, [5], lde_leaf_order(oracle, coeffs, rate), full.cap, first_leaf=8 << lg)
    o.close()
    full.close()
