"""lcp2_witness_settle_copies without a GPU: csrc/witness_settle.hpp compiled for the CPU (tests/emu/emu_settle.cpp), its three passes -
owner, conflicts, broadcast - held to circuit.settle_copies_model, matrix and report, under several tilings.  Every comparison is
exact."""
import ctypes

import numpy as np
import pytest

import fill_copies_cases as fc
import settle_copies_cases as sc
import witness_check_cases as wc
from rows_lib import NONE, build_emu, vp

# (lanes per block, blocks and lanes from the last to the first).  With one lane per block every two entries of a list are in
# different blocks - an owner and the source that conflicts with it too -, and so are a class's owner cell and its other cells
TILINGS = [(256, 0), (1, 0), (64, 1), (7, 0)]


@pytest.fixture(scope="module")
def emus():
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_settle", (("emu_settle_copies", None, [V, U, U, c.c_uint, c.c_uint, V, U, c.c_int, V, V, V, U, c.c_int]),))


def emu_settle(E, circ, class_of, num_classes, sources, host_list, start, tile=256, reverse=0):
    """(matrix, report dict in the model's form) of an emulated call on a copy of `start`"""
    got, table = start.copy(), class_of.copy()
    report, flag = np.zeros(6, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    E.emu_settle_copies(vp(table), num_classes, circ.n, circ.params.num_wires, circ.params.num_routed_wires, vp(sources) if sources.size else None,
                        sources.size, int(host_list), vp(got), vp(report), vp(flag), tile, reverse)
    assert (table == class_of).all()   # the marks of the sources are taken off again
    refused = None if int(flag[0]) == NONE else int(flag[0]) >> 8
    out = {k: int(v) for k, v in zip(sc.REPORT_FIELDS, report)}
    out["refused"] = refused
    out["status"] = -1 if refused is not None else (-5 if out["conflicts"] else 0)
    return got, out


def settle_under_every_tiling(E, circ, class_of, num_classes, sources, host_list, start):
    """the emulated call under every tiling: one (matrix, report), the same word for word under all of them"""
    first = None
    for tile, reverse in TILINGS:
        got = emu_settle(E, circ, class_of, num_classes, sources, host_list, start, tile, reverse)
        if first is None:
            first = got
        assert got[1] == first[1] and (got[0] == first[0]).all(), (tile, reverse)
    return first


def check_against_model(E, circ, class_of, num_classes, sources, host_list, start):
    want_matrix, want = sc.model(circ, sources, host_list, start, class_of)
    got_matrix, got = settle_under_every_tiling(E, circ, class_of, num_classes, sources, host_list, start)
    assert got == want
    assert (got_matrix == want_matrix).all()
    return got_matrix, got


@pytest.fixture(scope="module")
def small():
    import eth_lc_plonky2_amd as m
    circ, wires, _ = wc.circuit(fc.DB, False)
    class_of, count = m.circuit.copy_classes_model(circ)
    return circ, wires, class_of, count


def test_the_model_is_fill_copies_on_the_gathered_list(small):
    """settle_copies_model = fill_copies_model on the values read from the matrix before anything changes, conflicts included"""
    import eth_lc_plonky2_amd as m
    circ, _, class_of, count = small
    cases, _, _ = sc.semantics(circ, class_of, count)
    for label, (sources, _, start, _) in cases.items():
        a, b = start.copy(), start.copy()
        got = m.circuit.settle_copies_model(circ, sources, a, class_of)
        want = m.circuit.fill_copies_model(circ, sc.gathered(sources, start), b, class_of)
        assert got == want and (a == b).all(), label


@pytest.mark.parametrize("label", list(fc.hand_cycles()))
def test_hand_made_permutations(emus, label):
    """every hand-made permutation on the 2^5-row circuit, garbage in every cell: one random source per class, then two further sources
    of every class (conflicts, as no two words agree) - matrix and report are the model's under every tiling"""
    circ = fc.hand_circuit(label)
    class_of, count = fc.hand_classes(label)
    rng = np.random.default_rng(31)
    start = sc.garbage((circ.params.num_wires, circ.n), rng)
    one = sc.refs_of(fc.one_per_class(circ, start, class_of, count, rng, classes=np.arange(count)))
    got_matrix, got = check_against_model(emus, circ, class_of, count, one, True, start)
    assert got["status"] == 0 and got["classes_set"] == count and got["cells_filled"] == int((class_of != sc.NO_CLASS).sum()) - count
    for cyc in fc.hand_cycles()[label]:
        assert len({int(got_matrix[j, r]) for j, r in cyc}) == 1
    more = [cyc[k] for cyc in fc.hand_cycles()[label] for k in (0, len(cyc) - 1)] + [(0, 1), (fc.NR - 1, 0), (fc.NR, 3)]
    sources = np.concatenate([sc.sources_of(more), one])[rng.permutation(len(more) + one.size)]
    _, got = check_against_model(emus, circ, class_of, count, sources, False, start)
    assert got["conflicts"] >= count and got["classes_set"] == count


@pytest.mark.parametrize("label,degree_bits,mix,base", fc.table_circuits(gpu=False))
def test_one_source_per_class_gives_the_witness_back(emus, label, degree_bits, mix, base):
    """one random member of every class as its source (and the free non-zero cells, which do nothing), every other cell of every class
    first overwritten with garbage: the result is the original witness and the model's, in any list order, under every tiling"""
    import eth_lc_plonky2_amd as m
    circ, wires, _ = wc.circuit(degree_bits, mix, base)
    class_of, count = m.circuit.copy_classes_model(circ)
    rng = np.random.default_rng(3)
    sources = sc.refs_of(fc.one_per_class(circ, wires, class_of, count, rng))
    start = sc.scrambled(circ, wires, class_of, sources, rng)
    assert (start != wires).sum() == int((class_of != sc.NO_CLASS).sum()) - count
    for order in (np.arange(sources.size), rng.permutation(sources.size)):
        got, report = check_against_model(emus, circ, class_of, count, sources[order], True, start)
        assert (got == wires).all()
        assert report["status"] == 0 and report["classes_set"] == count and report["conflicts"] == 0
        assert report["cells_filled"] == int((class_of != sc.NO_CLASS).sum()) - count


def test_partial_list_leaves_the_other_classes_their_garbage(emus, small):
    """half of the classes have a source: their cells hold the witness, every other word of the scrambled matrix is as it was"""
    circ, wires, class_of, count = small
    rng = np.random.default_rng(8)
    chosen = rng.permutation(count)[:count // 2]
    sources = sc.refs_of(fc.one_per_class(circ, wires, class_of, count, rng, classes=chosen))
    start = sc.scrambled(circ, wires, class_of, sources, rng)
    got, report = check_against_model(emus, circ, class_of, count, sources, True, start)
    mine = np.zeros(wires.shape, dtype=bool)
    mine[:circ.params.num_routed_wires] = np.isin(class_of, chosen)
    assert report["classes_set"] == chosen.size and report["cells_filled"] == int(mine.sum()) - chosen.size
    assert (got[mine] == wires[mine]).all() and (got[~mine] == start[~mine]).all()
    assert (start[~mine] != wires[~mine]).sum() > count // 4   # (there was garbage to keep)


@pytest.mark.parametrize("label", ["owner-is-smallest-index", "owner-is-smallest-index-other-order", "three-listed-two-wrong",
                                   "canonical-equal-is-no-conflict", "no-class-sources-do-nothing", "same-cell-twice", "row-out-of-range-host",
                                   "column-out-of-range-device", "empty-list"])
def test_settle_semantics_equal_the_model(emus, small, label):
    """owner = smallest list index in both list orders, the class ends with the owner's raw word, conflicts on canonical values only,
    sources in no class and a cell listed twice, entries out of range (a host list as a whole, a device list entry by entry), nothing
    listed: the model's matrix and report under every tiling, and each case is what its name says"""
    circ, _, class_of, count = small
    cases, A, B = sc.semantics(circ, class_of, count)
    sources, host_list, start, expect = cases[label]
    got_matrix, got = check_against_model(emus, circ, class_of, count, sources, host_list, start)
    assert {k: got[k] for k in expect} == expect
    in_b = class_of == class_of[B[0]]
    if label.startswith("owner-is-smallest-index"):
        owner = sources[0]
        assert (got_matrix[:fc.NR][in_b] == start[owner["col"], owner["row"]]).all()
        assert int(start[owner["col"], owner["row"]]) == (77 if label == "owner-is-smallest-index" else 78)
    if label == "canonical-equal-is-no-conflict":
        assert (got_matrix[:fc.NR][class_of == class_of[A[0]]] == np.uint64(0x1234 + sc.P)).all() and (got_matrix[:fc.NR][in_b] == np.uint64(sc.P + 1)).all()
    if label in ("no-class-sources-do-nothing", "row-out-of-range-host", "empty-list"):
        assert (got_matrix == start).all()
    if label == "same-cell-twice":
        assert (got_matrix[:fc.NR][in_b] == sc.TAG).all() and got["cells_filled"] == (int(in_b.sum()) - 1) + (2 - 1)
    # nothing outside the owned classes changes
    owned = np.zeros(start.shape, dtype=bool)
    if not (host_list and got["refused"] is not None):
        for s in sources:
            if s["row"] < circ.n and s["col"] < fc.NR and class_of[s["col"], s["row"]] != sc.NO_CLASS:
                owned[:fc.NR][class_of == class_of[s["col"], s["row"]]] = True
    assert (got_matrix[~owned] == start[~owned]).all()


def test_an_owner_and_its_conflicting_source_in_different_blocks(emus, small):
    """tiles of one and of two lanes put the owner (index 0) and the conflicting source (index 2) of a class into different blocks of
    the list passes, a tile of 256 into one: the same matrix and the same report, whichever block runs first"""
    circ, _, class_of, count = small
    cases, _, _ = sc.semantics(circ, class_of, count)
    sources, host_list, start, expect = cases["owner-is-smallest-index"]
    results = [emu_settle(emus, circ, class_of, count, sources, host_list, start, tile, reverse) for tile in (1, 2, 256) for reverse in (0, 1)]
    for got_matrix, got in results:
        assert got == results[0][1] and (got_matrix == results[0][0]).all()
        assert {k: got[k] for k in expect} == expect
