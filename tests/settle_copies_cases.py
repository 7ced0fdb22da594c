"""What tests/test_settle_copies_emu.py (CPU) and tests/test_settle_copies.py (GPU) share (test harness only): source lists from the
cell lists of fill_copies_cases, matrices with scrambled class cells, and the lists and start matrices of the semantics cases with
what each must report.  The expected matrices come from circuit.settle_copies_model."""
import numpy as np

import fill_copies_cases as fc
from rows_lib import MAX, TAG

P = fc.P
NO_CLASS = 0xFFFFFFFF
NOBODY = (1 << 64) - 1
REPORT_FIELDS = ("num_classes", "classes_set", "cells_filled", "conflicts", "conflict_index", "owner_index")


def ref_dtype():
    import eth_lc_plonky2_amd as m
    return m.binding.CELL_REF_DTYPE


def refs_of(cells):
    """the sources of a list of cells: row and col, the value dropped"""
    out = np.zeros(cells.size, dtype=ref_dtype())
    out["row"], out["col"] = cells["row"], cells["col"]
    return out


def sources_of(entries):
    """CELL_REF_DTYPE records from (col, row) pairs, the order of fill_copies_cases.members"""
    out = np.zeros(len(entries), dtype=ref_dtype())
    for i, (col, row) in enumerate(entries):
        out[i] = (row, col)
    return out


def gathered(sources, wires):
    """the CELL_DTYPE list fill_copies takes to do what settle_copies does from `sources` on `wires`: the values read from the matrix
    (an entry out of range keeps the value 0; both calls refuse it)"""
    out = np.zeros(sources.size, dtype=fc.cell_dtype())
    out["row"], out["col"] = sources["row"], sources["col"]
    ok = (out["row"] < wires.shape[1]) & (out["col"] < wires.shape[0])
    out["value"][ok] = wires[out["col"][ok], out["row"][ok]]
    return out


def garbage(shape, rng):
    """a matrix of words from the whole 64-bit range: no two cells agree, many are not canonical"""
    return rng.integers(0, MAX, size=shape, dtype=np.uint64, endpoint=True)


def scrambled(circ, wires, class_of, sources, rng):
    """the witness with every cell of every class overwritten with garbage, the cells of `sources` excepted"""
    nr = circ.params.num_routed_wires
    hit = np.zeros(wires.shape, dtype=bool)
    hit[:nr] = class_of != NO_CLASS
    ok = (sources["row"] < circ.n) & (sources["col"] < circ.params.num_wires)
    hit[sources["col"][ok], sources["row"][ok]] = False
    out = wires.copy()
    out[hit] = garbage(int(hit.sum()), rng)
    return out


def semantics(circ, class_of, num_classes):
    """{label: (sources, host_list, start matrix, what the report must say)} on the synthetic 2^5-row circuit.  Class A has two cells,
    class B is the longest; `free` is a routed cell that is its own image, (100, 3) a cell of a non-routed wire."""
    sizes = np.bincount(class_of[class_of != NO_CLASS], minlength=num_classes)
    a, b = int(np.nonzero(sizes == 2)[0][0]), int(np.argmax(sizes))
    assert sizes[b] > 2 and a != b
    A, B = fc.members(class_of, a), fc.members(class_of, b)
    free = next((j, r) for j in range(fc.NR) for r in range(fc.N) if class_of[j, r] == NO_CLASS)
    base = garbage((circ.params.num_wires, circ.n), np.random.default_rng(21))
    v = 0x1234

    def start(values):
        out = base.copy()
        for (col, row), value in values.items():
            out[col, row] = value
        return out

    return {
        "owner-is-smallest-index": (sources_of([B[2], free, B[0]]), True, start({B[2]: 77, B[0]: 78}),
                                    dict(status=-5, classes_set=1, conflicts=1, conflict_index=2, owner_index=0)),
        "owner-is-smallest-index-other-order": (sources_of([B[0], free, B[2]]), True, start({B[2]: 77, B[0]: 78}),
                                                dict(status=-5, classes_set=1, conflicts=1, conflict_index=2, owner_index=0)),
        "three-listed-two-wrong": (sources_of([free, B[1], B[0], B[2]]), True, start({B[1]: 40, B[0]: 41, B[2]: 42}),
                                   dict(status=-5, conflicts=2, conflict_index=2, owner_index=1)),
        "canonical-equal-is-no-conflict": (sources_of([A[1], A[0], B[0], B[1]]), True, start({A[0]: v, A[1]: v + P, B[0]: P + 1, B[1]: 1}),
                                           dict(status=0, conflicts=0, classes_set=2, conflict_index=NOBODY)),
        "no-class-sources-do-nothing": (sources_of([(100, 3), free, (circ.params.num_wires - 1, circ.n - 1)]), True, start({}),
                                        dict(status=0, classes_set=0, cells_filled=0)),
        "same-cell-twice": (sources_of([B[1], B[1], A[0], B[1]]), True, start({B[1]: TAG}), dict(status=0, conflicts=0, classes_set=2)),
        "row-out-of-range-host": (sources_of([A[0], (2, fc.N), B[0]]), True, start({}), dict(status=-1, refused=1)),
        "column-out-of-range-device": (sources_of([A[0], (135, 0), B[0], (1, fc.N + 5)]), False, start({}), dict(status=-1, refused=1, classes_set=2)),
        "empty-list": (sources_of([]), True, start({}), dict(status=0, classes_set=0, cells_filled=0)),
    }, A, B


def model(circ, sources, host_list, start, class_of):
    """(matrix, report dict) lcp2_witness_settle_copies must leave: circuit.settle_copies_model, and nothing at all for a host list
    with a refused entry"""
    import eth_lc_plonky2_amd as m
    want_matrix = start.copy()
    want = m.circuit.settle_copies_model(circ, sources, want_matrix, class_of)
    if host_list and want["refused"] is not None:
        want_matrix = start.copy()
        want.update(classes_set=0, cells_filled=0, conflicts=0, conflict_index=NOBODY, owner_index=NOBODY)
    return want_matrix, want
