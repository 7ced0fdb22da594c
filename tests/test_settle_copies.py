"""lcp2_witness_settle_copies on the GPU: word for word what lcp2_witness_fill_copies does from the list of the values gathered from
the matrix, the round trip from a scrambled witness to the witness and its proof, conflicts and owners against the numpy model,
refusals, a call in the middle of a proof in flight, and the class table shared with the other two calls.  Every comparison is
exact.  The circuits: 2^5 rows (2560 routed cells: 10 blocks of the broadcast) and 2^10 rows (320 blocks; tens of blocks of the list
passes)."""
import ctypes

import numpy as np
import pytest

import fill_copies_cases as fc
import settle_copies_cases as sc
import witness_check_cases as wc
from rows_lib import TAG, DeviceMatrix, upload

pytestmark = pytest.mark.gpu


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


def fields(report):
    return {k: getattr(report, k) for k in sc.REPORT_FIELDS}


def settle(gpu_ctx, data, sources, ptr, device):
    """settle_copies from a host list or from its upload"""
    import eth_lc_plonky2_amd as m
    if not device:
        return data.settle_copies(sources, ptr)
    up = upload(gpu_ctx, sources)
    try:
        return data.settle_copies(up, ptr, mem=m.binding.MEM_DEVICE, nsources=sources.size)
    finally:
        gpu_ctx.buffer_free(up)


@pytest.mark.parametrize("device", [False, True], ids=["host-list", "device-list"])
@pytest.mark.parametrize("mix", [False, True])
def test_equals_fill_copies_from_the_gathered_values(gpu_ctx, big, mix, device):
    """a matrix of garbage, one source in three quarters of the classes and a second and third source in some of them (conflicts):
    settle_copies on one copy, fill_copies with the values gathered from the matrix on another - the same matrix and the same report"""
    import eth_lc_plonky2_amd as m
    circ, wires, _, data, class_of, count, _ = big[mix]
    rng = np.random.default_rng(12)
    start = sc.garbage(wires.shape, rng)
    chosen = rng.permutation(count)[:3 * count // 4]
    one = sc.refs_of(fc.one_per_class(circ, start, class_of, count, rng, classes=chosen))
    again = sc.refs_of(fc.one_per_class(circ, start, class_of, count, rng, classes=chosen[:count // 8]))
    nowhere = sc.sources_of([(circ.params.num_wires - 1, circ.n - 1), (fc.NR, 0)])
    sources = np.concatenate([one, again, one[:5], nowhere])
    sources = sources[rng.permutation(sources.size)]
    assert sources.size > 4 * 256
    cells = sc.gathered(sources, start)
    a, b = DeviceMatrix(gpu_ctx, start), DeviceMatrix(gpu_ctx, start)
    got = settle(gpu_ctx, data, sources, a.ptr, device)
    if device:
        up = upload(gpu_ctx, cells)
        want = data.fill_copies(up, b.ptr, mem=m.binding.MEM_DEVICE, ncells=cells.size)
        gpu_ctx.buffer_free(up)
    else:
        want = data.fill_copies(cells, b.ptr)
    got_matrix, want_matrix = a.read(), b.read()
    a.free()
    b.free()
    assert fields(got) == fields(want) and got.unsat and want.unsat and got.conflicts > 0 and got.classes_set == chosen.size
    assert got.message == want.message.replace("fill copies", "settle copies")
    assert (got_matrix == want_matrix).all()
    assert (got_matrix != start).sum() > chosen.size // 2


@pytest.mark.parametrize("mix", [False, True])
def test_round_trip_gives_the_witness_and_its_proof(gpu_ctx, big, mix):
    """the witness with every cell of every class but one random source scrambled: settled, it is the witness word for word, the proof
    from it the proof word for word, and no constraint is violated; the same from a device list"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, data, class_of, count, proof = big[mix]
    rng = np.random.default_rng(7)
    sources = sc.refs_of(fc.one_per_class(circ, wires, class_of, count, rng, classes=np.arange(count)))
    sources = sources[rng.permutation(sources.size)]
    start = sc.scrambled(circ, wires, class_of, sources, rng)
    in_classes = int((class_of != sc.NO_CLASS).sum())
    assert (start != wires).sum() == in_classes - count
    dm = DeviceMatrix(gpu_ctx, start)
    for device in (False, True):
        gpu_ctx.buffer_write(dm.ptr, start)
        report = settle(gpu_ctx, data, sources, dm.ptr, device)
        assert not report.unsat and fields(report) == dict(num_classes=count, classes_set=count, cells_filled=in_classes - count, conflicts=0,
                                                            conflict_index=sc.NOBODY, owner_index=sc.NOBODY)
        assert (dm.read() == wires).all()
        assert (data.prove(dm.ptr, pis, mem=m.binding.MEM_DEVICE) == proof).all()
        assert data.check_witness(dm.ptr, pis, mem=m.binding.MEM_DEVICE).ok
    dm.free()


@pytest.mark.parametrize("label", ["owner-is-smallest-index", "owner-is-smallest-index-other-order", "three-listed-two-wrong",
                                   "canonical-equal-is-no-conflict", "no-class-sources-do-nothing", "same-cell-twice"])
def test_conflicts_and_owners_equal_the_model(gpu_ctx, small, label):
    """two sources of a class with different words, in both list orders: LCP2_E_UNSAT, both list indices and both cells in the message,
    the owner's word in every cell of the class; three sources, two of them wrong; v and v + p agree and the raw word is kept; sources in
    no class; one cell listed twice"""
    circ, _, _, data, class_of, count = small
    cases, _, _ = sc.semantics(circ, class_of, count)
    sources, host_list, start, expect = cases[label]
    want_matrix, want = sc.model(circ, sources, host_list, start, class_of)
    assert {k: want[k] for k in expect} == expect
    for device in (False, True):
        dm = DeviceMatrix(gpu_ctx, start)
        report = settle(gpu_ctx, data, sources, dm.ptr, device)
        got = dm.read()
        dm.free()
        assert report.unsat == (want["status"] == -5)
        assert fields(report) == {k: want[k] for k in sc.REPORT_FIELDS}
        assert (got == want_matrix).all()
        if label.startswith("owner-is-smallest-index"):
            loser, owner = sources[2], sources[0]
            assert report.message.startswith("settle copies: cell 2 (row %d, wire %d) differs from cell 0 (row %d, wire %d), which gave"
                                             % (loser["row"], loser["col"], owner["row"], owner["col"]))
        if label == "three-listed-two-wrong":
            assert "cell 2 " in report.message and "cell 1 " in report.message and "(2 such cells" in report.message


def test_refusals(gpu_ctx, small):
    import eth_lc_plonky2_amd as m
    circ, wires, pis, data, class_of, count = small
    cases, _, _ = sc.semantics(circ, class_of, count)
    # a host list with row == n: refused as a whole
    sources, _, start, _ = cases["row-out-of-range-host"]
    dm = DeviceMatrix(gpu_ctx, start)
    with pytest.raises(m.Lcp2Error) as e:
        data.settle_copies(sources, dm.ptr)
    assert e.value.status == -1 and "settle copies: cell 1: row out of range" in str(e.value)
    assert (dm.read() == start).all()
    # a device list with bad entries: the classes of the others are filled, the first refused entry is named
    sources, host_list, start, _ = cases["column-out-of-range-device"]
    want_matrix, want = sc.model(circ, sources, host_list, start, class_of)
    assert want["refused"] == 1 and (want_matrix != start).any()
    gpu_ctx.buffer_write(dm.ptr, start)
    ptr = upload(gpu_ctx, sources)
    report = m.binding.FillReport()
    rc = data.lib.lcp2_witness_settle_copies(data.handle, ctypes.c_void_p(ptr), sources.size, m.binding.MEM_DEVICE, ctypes.c_void_p(dm.ptr), ctypes.byref(report))
    gpu_ctx.buffer_free(ptr)
    assert rc == -1 and "settle copies: cell 1: column out of range" in data.lib.lcp2_last_error(gpu_ctx.handle).decode()
    assert fields(report) == {k: want[k] for k in sc.REPORT_FIELDS}
    assert (dm.read() == want_matrix).all()
    table, _ = data.copy_classes()
    assert (table == class_of).all()   # no mark is left in the table
    # nothing listed
    gpu_ctx.buffer_write(dm.ptr, start)
    report = data.settle_copies(np.zeros(0, dtype=m.binding.CELL_REF_DTYPE), dm.ptr)
    assert not report.unsat and fields(report) == dict(num_classes=0, classes_set=0, cells_filled=0, conflicts=0, conflict_index=sc.NOBODY, owner_index=sc.NOBODY)
    assert (dm.read() == start).all()
    with pytest.raises(m.Lcp2Error):
        data.settle_copies(fc.cells_of([(0, 0, 5)]), dm.ptr)   # records of the other call's type
    # arguments
    lib, good = data.lib, cases["same-cell-twice"][0]
    gp = good.ctypes.data_as(ctypes.c_void_p)
    assert lib.lcp2_witness_settle_copies(None, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -1
    assert lib.lcp2_witness_settle_copies(data.handle, gp, good.size, 0, None, None) == -1
    assert lib.lcp2_witness_settle_copies(data.handle, None, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -1
    assert lib.lcp2_witness_settle_copies(data.handle, gp, good.size, 2, ctypes.c_void_p(dm.ptr), None) == -1
    assert (dm.read() == start).all()
    # a verifier-only handle, a sharded handle
    digest, cap = data.digest()
    verifier = m.CircuitData.verifier_only(circ, digest, cap)
    assert lib.lcp2_witness_settle_copies(verifier.handle, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -2
    verifier.close()
    shard = m.CircuitData.build_sharded(gpu_ctx, circ, 0, 4)
    assert lib.lcp2_witness_settle_copies(shard.handle, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == -6
    shard.close()
    assert (dm.read() == start).all()
    assert lib.lcp2_witness_settle_copies(data.handle, gp, good.size, 0, ctypes.c_void_p(dm.ptr), None) == 0   # (the list was a good one)
    dm.free()


@pytest.mark.parametrize("kind,reason", [("no-id", "is the id of no cell"), ("shared", "have the same image")])
def test_malformed_sigma_columns_are_refused(gpu_ctx, kind, reason):
    """the reasons lcp2_witness_fill_copies gives, from either call, and the matrix is not touched"""
    import eth_lc_plonky2_amd as m
    circ, bad, other = fc.malformed(kind)
    data = m.CircuitData.build(gpu_ctx, circ)
    start = np.full((circ.params.num_wires, circ.n), TAG, dtype=np.uint64)
    dm = DeviceMatrix(gpu_ctx, start)
    messages = []
    for call in (lambda: data.settle_copies(sc.sources_of([(0, 0)]), dm.ptr), lambda: data.fill_copies(fc.cells_of([(0, 0, TAG)]), dm.ptr)):
        with pytest.raises(m.Lcp2Error) as e:
            call()
        assert e.value.status == -1 and reason in str(e.value) and "(row %d, wire %d)" % (bad[1], bad[0]) in str(e.value)
        if other:
            assert "(row %d, wire %d)" % (other[1], other[0]) in str(e.value)
        messages.append(str(e.value))
    assert messages[0] == messages[1]
    assert (dm.read() == start).all()
    dm.free()
    data.close()


def test_a_call_inside_a_proof_in_flight_changes_nothing(gpu_ctx, big):
    """lcp2_commit_wires, then a settle on another buffer (which builds the class table of a fresh handle), then the rest of the staged
    proof: the caps are those of the undisturbed sequence, and the settled matrix is the witness"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis, _, class_of, count, _ = big[False]
    rng = np.random.default_rng(9)
    betas, gammas = rng.integers(1, wc.P, size=2, dtype=np.uint64), rng.integers(1, wc.P, size=2, dtype=np.uint64)
    alphas = rng.integers(1, wc.P, size=2, dtype=np.uint64)
    pi_hash = np.array(m.poseidon_py.hash_no_pad([int(v) for v in pis]), dtype=np.uint64)
    sources = sc.refs_of(fc.one_per_class(circ, wires, class_of, count, rng, classes=np.arange(count)))
    start = sc.scrambled(circ, wires, class_of, sources, rng)
    caps = []
    for disturb in (False, True):
        data = m.CircuitData.build(gpu_ctx, circ)
        wires_cap = data.commit_wires(wires)
        if disturb:
            dm = DeviceMatrix(gpu_ctx, start)
            assert not data.settle_copies(sources, dm.ptr).unsat
            assert (dm.read() == wires).all()
            dm.free()
        caps.append((wires_cap, data.perm_zs(betas, gammas), data.quotient(alphas, pi_hash)))
        data.close()
    for a, b in zip(*caps):
        assert (a == b).all()


@pytest.mark.parametrize("first", ["settle", "fill", "classes"])
def test_the_three_calls_share_one_class_table(gpu_ctx, small, first):
    """whichever of settle_copies, fill_copies and copy_classes builds the table of a fresh handle, the other two work from it: the
    table is the model's and both calls give what they give on the handle that has had its table all along"""
    import eth_lc_plonky2_amd as m
    circ, wires, _, warm, class_of, count = small
    rng = np.random.default_rng(14)
    sources = sc.refs_of(fc.one_per_class(circ, wires, class_of, count, rng, classes=np.arange(count)))
    start = sc.scrambled(circ, wires, class_of, sources, rng)
    cells = sc.gathered(sources, start)
    fresh = m.CircuitData.build(gpu_ctx, circ)
    dm = DeviceMatrix(gpu_ctx, start)

    def run(what, data):
        gpu_ctx.buffer_write(dm.ptr, start)
        if what == "classes":
            table, got_count = data.copy_classes()
            return table, got_count
        report = data.settle_copies(sources, dm.ptr) if what == "settle" else data.fill_copies(cells, dm.ptr)
        return dm.read(), fields(report)

    order = [first] + [w for w in ("settle", "fill", "classes") if w != first]
    for what in order:
        got, want = run(what, fresh), run(what, warm)
        assert (got[0] == want[0]).all() and got[1] == want[1], what
        if what == "classes":
            assert (got[0] == class_of).all() and got[1] == count
        else:
            assert (got[0] == wires).all() and got[1]["classes_set"] == count
    dm.free()
    fresh.close()
