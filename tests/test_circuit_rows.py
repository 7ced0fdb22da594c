"""lcp2_circuit_rows_expand and lcp2_circuit_create_from_rows on the GPU: the matrix against the numpy model and the circuit's own
constants_sigmas, a handle built from rows against the handle built from the expanded matrix (digest, cap, proof, copy classes), host
and device binding lists, refusals that leave the context usable, and an expansion in the middle of a proof in flight."""
import ctypes

import numpy as np
import pytest

import circuit_rows_cases as rc
import witness_check_cases as wc
from rows_lib import upload

pytestmark = pytest.mark.gpu


def model(circ, rows):
    import eth_lc_plonky2_amd as m
    return m.circuit.expand_rows_model(circ.params, circ.gateset, circ.k_is, rows)


@pytest.mark.parametrize("label,degree_bits,mix", rc.whole_circuits())
def test_whole_circuits_come_back_word_for_word(gpu_ctx, label, degree_bits, mix):
    circ, rows = rc.whole(degree_bits, mix)
    assert (gpu_ctx.expand_rows(circ, rows) == circ.constants_sigmas).all()


@pytest.mark.parametrize("label", list(rc.edge_lists()))
def test_edge_lists_equal_the_model(gpu_ctx, label):
    circ, _ = rc.base()
    rows = rc.edge_lists()[label]
    assert (gpu_ctx.expand_rows(circ, rows) == model(circ, rows)).all()


def test_null_constants_and_padding_rows(gpu_ctx):
    circ, _ = rc.base()
    rows = rc.without_constants()
    assert (gpu_ctx.expand_rows(circ, rows) == model(circ, rows)).all()


@pytest.mark.parametrize("label", ["random-classes", "tile-plus-one", "sparse-ids"])
def test_device_list_gives_the_matrix_of_the_host_list(gpu_ctx, label):
    circ, _ = rc.base()
    rows = rc.edge_lists()[label]
    ptr = upload(gpu_ctx, rows.bindings)
    got = gpu_ctx.expand_rows(circ, rows, bindings_ptr=ptr, num_bindings=rows.bindings.size)
    gpu_ctx.buffer_free(ptr)
    assert (got == gpu_ctx.expand_rows(circ, rows)).all() and (got == model(circ, rows)).all()


@pytest.fixture(scope="module")
def pair(gpu_ctx):
    """{mix: (circuit, wires, public inputs, handle from the matrix, handle from rows)} at 2^10 rows"""
    import eth_lc_plonky2_amd as m
    out = {}
    for mix in (False, True):
        circ, wires, pis = wc.circuit(10, mix)
        rows = m.circuit.circuit_rows_of(circ)
        out[mix] = (circ, wires, pis, m.CircuitData.build(gpu_ctx, circ), m.CircuitData.build_from_rows(gpu_ctx, circ, rows))
    yield out
    for entry in out.values():
        entry[3].close()
        entry[4].close()


@pytest.mark.parametrize("mix", [False, True])
def test_handle_from_rows_equals_handle_from_matrix(gpu_ctx, pair, mix):
    """same digest and cap, the same proof word for word, which verifies under both handles, and the same copy classes"""
    circ, wires, pis, plain, compact = pair[mix]
    (d0, cap0), (d1, cap1) = plain.digest(), compact.digest()
    assert (d0 == d1).all() and (cap0 == cap1).all()
    proof = compact.prove(wires, pis)
    assert (proof == plain.prove(wires, pis)).all()
    compact.verify(proof, pis)
    plain.verify(proof, pis)
    (c0, n0), (c1, n1) = plain.copy_classes(), compact.copy_classes()
    assert n0 == n1 > 0 and (c0 == c1).all()


@pytest.mark.parametrize("label", list(rc.refused_lists()))
def test_refused_list_leaves_the_context_usable(gpu_ctx, label):
    import eth_lc_plonky2_amd as m
    circ, good = rc.base()
    rows, status, message, _ = rc.refused_lists()[label]
    calls = [lambda: gpu_ctx.expand_rows(circ, rows), lambda: m.CircuitData.build_from_rows(gpu_ctx, circ, rows)]
    if label != "gate-out-of-range":
        ptr = upload(gpu_ctx, rows.bindings)
        calls.append(lambda: gpu_ctx.expand_rows(circ, rows, bindings_ptr=ptr, num_bindings=rows.bindings.size))
    for call in calls:
        with pytest.raises(m.Lcp2Error) as e:
            call()
        assert e.value.status == status and "circuit rows: " + message in str(e.value)
        if label.startswith("bound-twice"):
            assert "also bound by binding %d" % rc.twice_pair(label)[0] in str(e.value)
        assert (gpu_ctx.expand_rows(circ, good) == circ.constants_sigmas).all()
    if label != "gate-out-of-range":
        gpu_ctx.buffer_free(ptr)


def test_arguments(gpu_ctx):
    import eth_lc_plonky2_amd as m
    lib = gpu_ctx.lib
    circ, rows = rc.base()
    desc, keep = m.binding._describe(circ, 0)
    out = gpu_ctx.buffer_alloc((circ.params.num_constants + rc.NR) * rc.N)
    handle = ctypes.c_void_p()
    for label, (change, status, reason) in rc.argument_cases().items():
        r, keep_rows = m.binding._describe_rows(rows)
        for field, value in change.items():
            setattr(r, field, value)
        assert lib.lcp2_circuit_rows_expand(gpu_ctx.handle, ctypes.byref(desc), ctypes.byref(r), ctypes.c_void_p(out)) == status, label
        assert reason in lib.lcp2_last_error(gpu_ctx.handle).decode()
        assert lib.lcp2_circuit_create_from_rows(gpu_ctx.handle, ctypes.byref(desc), ctypes.byref(r), ctypes.byref(handle)) == status and not handle.value
    r, keep_rows = m.binding._describe_rows(rows)
    for args in ((None, ctypes.byref(desc), ctypes.byref(r)), (gpu_ctx.handle, None, ctypes.byref(r)), (gpu_ctx.handle, ctypes.byref(desc), None)):
        assert lib.lcp2_circuit_rows_expand(*args, ctypes.c_void_p(out)) == -1
        assert lib.lcp2_circuit_create_from_rows(*args, ctypes.byref(handle)) == -1
    assert lib.lcp2_circuit_rows_expand(gpu_ctx.handle, ctypes.byref(desc), ctypes.byref(r), None) == -1
    assert lib.lcp2_circuit_create_from_rows(gpu_ctx.handle, ctypes.byref(desc), ctypes.byref(r), None) == -1
    big = m.binding._describe(circ, 0)[0]
    big.params = m.standard_params(26, 4)   # 80 x 2^26 routed cells
    assert lib.lcp2_circuit_rows_expand(gpu_ctx.handle, ctypes.byref(big), ctypes.byref(r), ctypes.c_void_p(out)) == -6
    gpu_ctx.buffer_free(out)


def test_expansion_inside_a_proof_in_flight_changes_nothing(gpu_ctx):
    """lcp2_commit_wires, then an expansion (and a whole build from rows) on the same context, then the rest of the staged proof: the
    caps are those of the undisturbed sequence - the scratch slots of the expansion are none of the prover's buffers"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(10, False)
    rows = m.circuit.circuit_rows_of(circ)
    rng = np.random.default_rng(9)
    betas, gammas = rng.integers(1, wc.P, size=2, dtype=np.uint64), rng.integers(1, wc.P, size=2, dtype=np.uint64)
    alphas = rng.integers(1, wc.P, size=2, dtype=np.uint64)
    pi_hash = np.array(m.poseidon_py.hash_no_pad([int(v) for v in pis]), dtype=np.uint64)
    caps = []
    for disturb in (False, True):
        data = m.CircuitData.build(gpu_ctx, circ)
        wires_cap = data.commit_wires(wires)
        if disturb:
            assert (gpu_ctx.expand_rows(circ, rows) == circ.constants_sigmas).all()
            other = m.CircuitData.build_from_rows(gpu_ctx, circ, rows)
        zs_cap = data.perm_zs(betas, gammas)
        if disturb:
            small, edge = rc.base()[0], rc.edge_lists()["random-classes"]   # another size on the same context: the work area is reused
            assert (gpu_ctx.expand_rows(small, edge) == model(small, edge)).all()
            other.close()
        caps.append((wires_cap, zs_cap, data.quotient(alphas, pi_hash)))
        data.close()
    for a, b in zip(*caps):
        assert (a == b).all()
