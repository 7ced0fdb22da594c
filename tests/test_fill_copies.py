"""lcp2_witness_fill_copies and lcp2_circuit_copy_classes on the GPU: the class table against the numpy model, the round trip from one
cell per class to the witness and its proof, partial lists, conflicts, refusals, and a call in the middle of a proof in flight."""
import ctypes

import numpy as np
import pytest

import fill_copies_cases as fc
import witness_check_cases as wc
from rows_lib import TAG, DeviceMatrix, upload

pytestmark = pytest.mark.gpu
NOBODY = (1 << 64) - 1


@pytest.fixture(scope="module")
def big(gpu_ctx):
    """{mix: (circuit, wires, public inputs, handle, model table, classes, proof from the original witness)} at 2^10 rows"""
    import eth_lc_plonky2_amd as m
    out = {}
    for mix in (False, True):
        circ, wires, pis = wc.circuit(10, mix)
        data = m.CircuitData.build(gpu_ctx, circ)
        class_of, count = m.circuit.copy_classes_model(circ)
        out[mix] = (circ, wires, pis, data, class_of, count, data.prove(wires, pis))
    yield out
    for entry in out.values():
        entry[3].close()


@pytest.fixture(scope="module")
def small(gpu_ctx):
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(fc.DB, False)
    data = m.CircuitData.build(gpu_ctx, circ)
    class_of, count = m.circuit.copy_classes_model(circ)
    yield circ, wires, pis, data, class_of, count
    data.close()


@pytest.mark.parametrize("label,degree_bits,mix,base", fc.table_circuits(gpu=True))
def test_class_table_equals_the_model(gpu_ctx, label, degree_bits, mix, base):
    import eth_lc_plonky2_amd as m
    circ, _, _ = wc.circuit(degree_bits, mix, base)
    data = m.CircuitData.build(gpu_ctx, circ)
    want, count = m.circuit.copy_classes_model(circ)
    got, got_count = data.copy_classes()
    again, _ = data.copy_classes()   # the cached table
    data.close()
    assert got_count == count and (got == want).all() and (again == want).all()


@pytest.mark.parametrize("label", list(fc.hand_cycles()))
def test_hand_made_permutations(gpu_ctx, label):
    import eth_lc_plonky2_amd as m
    data = m.CircuitData.build(gpu_ctx, fc.hand_circuit(label))
    want, count = fc.hand_classes(label)
    got, got_count = data.copy_classes()
    data.close()
    assert got_count == count and (got == want).all()


@pytest.mark.parametrize("mix", [False, True])
def test_round_trip_gives_the_witness_and_its_proof(gpu_ctx, big, mix):
    """one random member of every class plus the free non-zero cells, into a zeroed device matrix: the witness word for word, the
    proof from it word for word, no violation; the same from a device list and from a shuffled list"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, data, class_of, count, proof = big[mix]
    rng = np.random.default_rng(7)
    cells = fc.one_per_class(circ, wires, class_of, count, rng)
    routed_in_classes = int((class_of != 0xFFFFFFFF).sum())
    dm = DeviceMatrix(gpu_ctx, np.zeros_like(wires))
    for how in ("host", "device", "shuffled"):
        gpu_ctx.buffer_zero(dm.ptr, wires.size)
        lst = cells[rng.permutation(cells.size)] if how == "shuffled" else cells
        if how == "device":
            ptr = upload(gpu_ctx, lst)
            report = data.fill_copies(ptr, dm.ptr, mem=m.binding.MEM_DEVICE, ncells=lst.size)
            gpu_ctx.buffer_free(ptr)
        else:
            report = data.fill_copies(lst, dm.ptr)
        assert not report.unsat and (report.num_classes, report.classes_set, report.conflicts) == (count, count, 0), how
        assert report.cells_filled == routed_in_classes - count and (report.conflict_index, report.owner_index) == (NOBODY, NOBODY)
        assert (dm.read() == wires).all(), how
        assert (data.prove(dm.ptr, pis, mem=m.binding.MEM_DEVICE) == proof).all(), how
        assert data.check_witness(dm.ptr, pis, mem=m.binding.MEM_DEVICE).ok
    dm.free()


def test_partial_list_leaves_the_other_classes_alone(gpu_ctx, big):
    """half of the classes listed: their cells hold the witness, every other word of a tagged matrix is as it was"""
    circ, wires, pis, data, class_of, count, _ = big[False]
    rng = np.random.default_rng(8)
    chosen = rng.permutation(count)[:count // 2]
    cells = fc.one_per_class(circ, wires, class_of, count, rng, classes=chosen)
    start = np.full(wires.shape, TAG, dtype=np.uint64)
    dm = DeviceMatrix(gpu_ctx, start)
    report = data.fill_copies(cells, dm.ptr)
    got = dm.read()
    dm.free()
    mine = np.zeros(wires.shape, dtype=bool)
    mine[:circ.params.num_routed_wires] = np.isin(class_of, chosen)
    assert report.classes_set == chosen.size and report.cells_filled == int(mine.sum()) - chosen.size
    assert (got[mine] == wires[mine]).all() and (got[~mine] == TAG).all()


@pytest.mark.parametrize("label", ["owner-is-smallest-index", "raw-value-kept", "canonical-equal-is-no-conflict", "three-listed-two-wrong"])
def test_conflicts_and_owners_equal_the_model(gpu_ctx, small, label):
    """two members of a class with different values: LCP2_E_UNSAT, both list indices, the owner's value in every cell of the class;
    three members, two of them wrong: two conflicts, the smaller index; raw values kept; v and v + p agree"""
    import eth_lc_plonky2_amd as m
    circ, _, _, data, class_of, count = small
    cells, _ = fc.semantics_lists(circ, class_of, count)[label]
    start = np.full((circ.params.num_wires, circ.n), TAG, dtype=np.uint64)
    want_matrix = start.copy()
    want = m.circuit.fill_copies_model(circ, cells, want_matrix, class_of)
    dm = DeviceMatrix(gpu_ctx, start)
    report = data.fill_copies(cells, dm.ptr)
    got = dm.read()
    dm.free()
    assert report.unsat == (want["status"] == -5)
    assert {k: getattr(report, k) for k in ("num_classes", "classes_set", "cells_filled", "conflicts", "conflict_index", "owner_index")} == \
        {k: want[k] for k in ("num_classes", "classes_set", "cells_filled", "conflicts", "conflict_index", "owner_index")}
    assert (got == want_matrix).all()
    if label == "owner-is-smallest-index":
        assert (report.conflicts, report.conflict_index, report.owner_index) == (1, 2, 0)
        assert "cell 2 " in report.message and "cell 0 " in report.message
    if label == "three-listed-two-wrong":
        assert (report.conflicts, report.conflict_index, report.owner_index) == (2, 2, 1)


def test_refusals(gpu_ctx, small):
    import eth_lc_plonky2_amd as m
    circ, wires, pis, data, class_of, count = small
    lists = fc.semantics_lists(circ, class_of, count)
    start = np.full((circ.params.num_wires, circ.n), TAG, dtype=np.uint64)
    dm = DeviceMatrix(gpu_ctx, start)
    # a host list with row == n: refused as a whole
    cells, _ = lists["row-out-of-range-host"]
    with pytest.raises(m.Lcp2Error) as e:
        data.fill_copies(cells, dm.ptr)
    assert e.value.status == -1 and "cell 1: row out of range" in str(e.value)
    assert (dm.read() == start).all()
    # a device list with bad entries: the others are written, the first refused entry is named
    cells, _ = lists["column-out-of-range-device"]
    want_matrix = start.copy()
    m.circuit.fill_copies_model(circ, cells, want_matrix, class_of)
    ptr = upload(gpu_ctx, cells)
    with pytest.raises(m.Lcp2Error) as e:
        data.fill_copies(ptr, dm.ptr, mem=m.binding.MEM_DEVICE, ncells=cells.size)
    gpu_ctx.buffer_free(ptr)
    assert e.value.status == -1 and "cell 1: column out of range" in str(e.value)
    assert (dm.read() == want_matrix).all()
    table, _ = data.copy_classes()
    assert (table == class_of).all()   # no mark is left in the table
    # nothing listed
    gpu_ctx.buffer_write(dm.ptr, start)
    report = data.fill_copies(np.zeros(0, dtype=m.binding.CELL_DTYPE), dm.ptr)
    assert not report.unsat and report.classes_set == 0 and (dm.read() == start).all()
    # arguments
    lib, good = data.lib, lists["raw-value-kept"][0]
    gp = good.ctypes.data_as(ctypes.c_void_p)
    assert lib.lcp2_witness_fill_copies(None, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -1
    assert lib.lcp2_witness_fill_copies(data.handle, gp, good.size, 0, None, None) == -1
    assert lib.lcp2_witness_fill_copies(data.handle, None, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -1
    assert lib.lcp2_witness_fill_copies(data.handle, gp, good.size, 2, ctypes.c_void_p(dm.ptr), None) == -1
    assert lib.lcp2_circuit_copy_classes(None, None, None) == -1
    assert (dm.read() == start).all()
    # a verifier-only handle, a sharded handle
    digest, cap = data.digest()
    verifier = m.CircuitData.verifier_only(circ, digest, cap)
    assert lib.lcp2_witness_fill_copies(verifier.handle, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -2
    assert lib.lcp2_circuit_copy_classes(verifier.handle, None, None) == -2
    verifier.close()
    shard = m.CircuitData.build_sharded(gpu_ctx, circ, 0, 4)
    assert lib.lcp2_witness_fill_copies(shard.handle, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -6
    assert lib.lcp2_circuit_copy_classes(shard.handle, None, None) == -6
    shard.close()
    assert (dm.read() == start).all()
    dm.free()


@pytest.mark.parametrize("kind,reason", [("no-id", "is the id of no cell"), ("shared", "have the same image")])
def test_malformed_sigma_columns_are_refused(gpu_ctx, kind, reason):
    import eth_lc_plonky2_amd as m
    circ, bad, other = fc.malformed(kind)
    data = m.CircuitData.build(gpu_ctx, circ)
    dm = DeviceMatrix(gpu_ctx, np.zeros((circ.params.num_wires, circ.n), dtype=np.uint64))
    cells = fc.cells_of([(0, 0, 5)])
    for call in (lambda: data.copy_classes(), lambda: data.fill_copies(cells, dm.ptr)):
        with pytest.raises(m.Lcp2Error) as e:
            call()
        assert e.value.status == -1 and reason in str(e.value) and "(row %d, wire %d)" % (bad[1], bad[0]) in str(e.value)
        if other:
            assert "(row %d, wire %d)" % (other[1], other[0]) in str(e.value)
    assert not dm.read().any()
    dm.free()
    data.close()


def test_a_call_inside_a_proof_in_flight_changes_nothing(gpu_ctx, big):
    """lcp2_commit_wires, then a fill on another buffer (which builds the class table of a fresh handle), then the rest of the staged
    proof: the caps are those of the undisturbed sequence"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, _, class_of, count, _ = big[False]
    rng = np.random.default_rng(9)
    betas, gammas = rng.integers(1, wc.P, size=2, dtype=np.uint64), rng.integers(1, wc.P, size=2, dtype=np.uint64)
    alphas = rng.integers(1, wc.P, size=2, dtype=np.uint64)
    pi_hash = np.array(m.poseidon_py.hash_no_pad([int(v) for v in pis]), dtype=np.uint64)
    cells = fc.one_per_class(circ, wires, class_of, count, rng)
    caps = []
    for disturb in (False, True):
        data = m.CircuitData.build(gpu_ctx, circ)
        wires_cap = data.commit_wires(wires)
        if disturb:
            dm = DeviceMatrix(gpu_ctx, np.zeros_like(wires))
            assert not data.fill_copies(cells, dm.ptr).unsat
            assert (dm.read() == wires).all()
            dm.free()
        caps.append((wires_cap, data.perm_zs(betas, gammas), data.quotient(alphas, pi_hash)))
        data.close()
    for a, b in zip(*caps):
        assert (a == b).all()
