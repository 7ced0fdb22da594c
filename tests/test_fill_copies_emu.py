"""lcp2_witness_fill_copies without a GPU: csrc/witness_fill.hpp compiled for the CPU (tests/emu/emu_fill.cpp).  The class table - decode,
permutation check, pointer-jumping rounds, numbering - is held to circuit.copy_classes_model and to hand-made cycles, a call - owner,
broadcast, conflicts - to circuit.fill_copies_model."""
import ctypes

import numpy as np
import pytest

import fill_copies_cases as fc
import witness_check_cases as wc
from rows_lib import NONE, TAG, build_emu, vp

NO_ID, SHARED = 1, 2   # FILL_SIGMA_*


@pytest.fixture(scope="module")
def emuf():
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_fill", (("emu_fill_classes", c.c_int, [V, V, V, c.c_int]),
                                  ("emu_fill_copies", None, [V, U, U, c.c_uint, c.c_uint, V, U, c.c_int, V, V, V, c.c_int])))


def emu_classes(E, circ, reverse=0):
    """(status, class_of, num_classes, rounds, refused cell, other cell) of the emulated table construction"""
    import eth_lc_plonky2_amd as m
    desc, keep = m.binding._describe(circ)
    class_of = np.zeros((circ.params.num_routed_wires, circ.n), dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint64)
    rc = E.emu_fill_classes(ctypes.byref(desc), vp(class_of), vp(out), reverse)
    return rc, class_of, int(out[0]), int(out[1]), int(out[2]), int(out[3])


def emu_fill(E, circ, class_of, num_classes, cells, host_list, start, reverse=0):
    """(matrix, report dict in the model's form) of an emulated call on a copy of `start`"""
    got, table = start.copy(), class_of.copy()
    report, flag = np.zeros(6, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    E.emu_fill_copies(vp(table), num_classes, circ.n, circ.params.num_wires, circ.params.num_routed_wires, vp(cells), cells.size, int(host_list),
                      vp(got), vp(report), vp(flag), reverse)
    assert (table == class_of).all()   # the marks of the listed cells are taken off again
    refused = None if int(flag[0]) == NONE else int(flag[0]) >> 8
    names = ("num_classes", "classes_set", "cells_filled", "conflicts", "conflict_index", "owner_index")
    out = {k: int(v) for k, v in zip(names, report)}
    out["refused"] = refused
    out["status"] = -1 if refused is not None else (-5 if out["conflicts"] else 0)
    return got, out


@pytest.mark.parametrize("label,degree_bits,mix,base", fc.table_circuits(gpu=False))
def test_class_table_equals_the_model(emuf, label, degree_bits, mix, base):
    """synthetic circuit at 2^5 and 2^7 rows, the reference gate mix at 2^8, a coset shift base other than 7: the table of the portable
    text is the union-find model's, cell for cell, whichever way the lanes run"""
    import eth_lc_plonky2_amd as m
    circ, _, _ = wc.circuit(degree_bits, mix, base)
    want, count = m.circuit.copy_classes_model(circ)
    assert count > 2
    for reverse in (0, 1):
        rc, got, got_count, rounds, _, _ = emu_classes(emuf, circ, reverse)
        assert rc == 0 and got_count == count and 1 <= rounds <= 32
        assert (got == want).all()


@pytest.mark.parametrize("label", list(fc.hand_cycles()))
def test_hand_made_permutations(emuf, label):
    """the identity, a 2-cycle, a 3- and a 5-cycle, one cycle through all 2560 cells, a cycle with cell 0 and the last cell, a cycle
    inside one column and one across all 80: the table is what the cycles say, and the model agrees"""
    import eth_lc_plonky2_amd as m
    circ = fc.hand_circuit(label)
    want, count = fc.hand_classes(label)
    rc, got, got_count, rounds, _, _ = emu_classes(emuf, circ)
    assert rc == 0 and got_count == count and (got == want).all()
    model, model_count = m.circuit.copy_classes_model(circ)
    assert model_count == count and (model == want).all()
    longest = max([len(c) for c in fc.hand_cycles()[label]] + [1])
    assert rounds <= max(int(np.ceil(np.log2(longest))), 0)   # 2^rounds cells are enough to see the whole cycle
    if label == "every-cell":
        assert rounds == 12   # 2^11 < 2559 cells between cell 0's successor and cell 0


@pytest.mark.parametrize("kind,code", [("no-id", NO_ID), ("shared", SHARED)])
def test_malformed_sigma_columns_are_refused(emuf, kind, code):
    """a sigma value that is no cell id, and two cells with one image: each refused with its own reason and the cell it was found at,
    without a single jumping round"""
    import eth_lc_plonky2_amd as m
    circ, bad, other = fc.malformed(kind)
    rc, _, _, rounds, cell, second = emu_classes(emuf, circ)
    assert rc == code and rounds == 0
    assert cell == bad[0] * circ.n + bad[1]
    if other is not None:
        assert second == other[0] * circ.n + other[1]
    with pytest.raises(ValueError):
        m.circuit.copy_classes_model(circ)


@pytest.fixture(scope="module")
def small():
    import eth_lc_plonky2_amd as m
    circ, wires, _ = wc.circuit(fc.DB, False)
    class_of, count = m.circuit.copy_classes_model(circ)
    return circ, wires, class_of, count


def tagged(circ):
    """a matrix no call has written: TAG everywhere, and circuit.tag_witness's mark in the free cells of the last row"""
    import eth_lc_plonky2_amd as m
    return m.circuit.tag_witness(np.full((circ.params.num_wires, circ.n), TAG, dtype=np.uint64), 0xABCDEF)


@pytest.mark.parametrize("label", ["owner-is-smallest-index", "raw-value-kept", "canonical-equal-is-no-conflict", "three-listed-two-wrong",
                                   "row-out-of-range-host", "column-out-of-range-device"])
def test_fill_semantics_equal_the_model(emuf, small, label):
    """owner = smallest list index, raw values kept, conflicts on canonical values only, classes nobody lists keep their tags, entries
    out of range refused (a host list as a whole, a device list entry by entry)"""
    import eth_lc_plonky2_amd as m
    circ, _, class_of, count = small
    cells, host_list = fc.semantics_lists(circ, class_of, count)[label]
    start = tagged(circ)
    want_matrix = start.copy()
    want = m.circuit.fill_copies_model(circ, cells, want_matrix, class_of)
    if host_list and want["refused"] is not None:   # nothing runs
        want_matrix = start
        want.update(classes_set=0, cells_filled=0, conflicts=0, conflict_index=NONE, owner_index=NONE)
    for reverse in (0, 1):
        got_matrix, got = emu_fill(emuf, circ, class_of, count, cells, host_list, start, reverse)
        assert got == want, label
        assert (got_matrix == want_matrix).all(), label
    # the cases are what they say
    expect = {"owner-is-smallest-index": dict(status=-5, conflicts=1, conflict_index=2, owner_index=0),
              "raw-value-kept": dict(status=0, classes_set=2), "canonical-equal-is-no-conflict": dict(status=0, conflicts=0, classes_set=2),
              "three-listed-two-wrong": dict(status=-5, conflicts=2, conflict_index=2, owner_index=1),
              "row-out-of-range-host": dict(status=-1, refused=1), "column-out-of-range-device": dict(status=-1, refused=1, classes_set=2)}[label]
    assert {k: want[k] for k in expect} == expect
    untouched = np.ones(start.shape, dtype=bool)
    for c in cells:
        if c["row"] < circ.n and c["col"] < circ.params.num_wires:
            untouched[c["col"], c["row"]] = False
            if c["col"] < fc.NR and class_of[c["col"], c["row"]] != 0xFFFFFFFF:
                untouched[:fc.NR][class_of == class_of[c["col"], c["row"]]] = False
    assert (got_matrix[untouched] == start[untouched]).all() and untouched.sum() > start.size // 2


def test_one_cell_per_class_gives_the_whole_witness_back(emuf, small):
    """one random member of every class and the free non-zero cells, into a zero matrix: the witness, word for word, in any list order"""
    circ, wires, class_of, count = small
    rng = np.random.default_rng(3)
    cells = fc.one_per_class(circ, wires, class_of, count, rng)
    for order in (np.arange(cells.size), rng.permutation(cells.size)):
        got, report = emu_fill(emuf, circ, class_of, count, cells[order], True, np.zeros_like(wires))
        assert (got == wires).all()
        assert report["status"] == 0 and report["classes_set"] == count
        assert report["cells_filled"] == int((class_of != 0xFFFFFFFF).sum()) - count
