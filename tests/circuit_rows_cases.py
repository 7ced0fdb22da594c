"""What tests/test_circuit_rows_emu.py (CPU) and tests/test_circuit_rows.py (GPU) share (test harness only): the circuits whose matrix
must come back word for word from circuit.circuit_rows_of, the edge lists on a 2^5-row circuit with 80 routed wires, and the refused
lists with the index and reason lcp2_last_error must name.  The tile of the device's sort is 256 lanes x 8 entries = 2048."""
import functools

import numpy as np

import witness_check_cases as wc

NR, DB, N = 80, 5, 32   # the edge lists: 80 routed wires, 2^5 rows, 2560 cells
TILE = 2048             # csrc/circuit_rows.hip ROWS_THREADS * ROWS_RUN
NONE = (1 << 64) - 1
BIND_ROW, BIND_COLUMN, BIND_CLASS, BIND_TWICE, GATE = 1, 2, 3, 4, 5   # ROWS_* of csrc/circuit_rows.hpp


def whole_circuits():
    """(label, degree_bits, mix): circuits whose own matrix the expansion of circuit_rows_of must equal"""
    return [("synthetic-5", 5, False), ("synthetic-8", 8, False), ("mix-10", 10, True)]


@functools.lru_cache(maxsize=None)
def whole(degree_bits, mix):
    """(circuit, its Rows)"""
    import eth_lc_plonky2_amd as m
    circ, _, _ = wc.circuit(degree_bits, mix)
    return circ, m.circuit.circuit_rows_of(circ)


def base():
    """the synthetic 2^5-row circuit whose parameters, gate set and coset shifts the edge lists use, with its own rows and constants"""
    return whole(DB, False)


def with_bindings(entries, num_classes):
    """the Rows of base() with its binding list replaced by `entries`: (row, col, cls) triples or a BINDING_DTYPE array"""
    import eth_lc_plonky2_amd as m
    _, rows = base()
    b = entries if isinstance(entries, np.ndarray) else m.circuit.bindings_of(entries)
    return m.circuit.Rows(rows.gate_of_row, rows.pad_gate, rows.row_constants, b, num_classes)


def all_cells(rng=None):
    """every routed cell as (row, col), column by column, or shuffled"""
    cells = [(r, j) for j in range(NR) for r in range(N)]
    if rng is not None:
        cells = [cells[i] for i in rng.permutation(len(cells))]
    return cells


@functools.lru_cache(maxsize=None)
def edge_lists():
    """{label: Rows}"""
    rng = np.random.default_rng(21)
    shuffled = all_cells(rng)
    big = (1 << 20) + 3
    sparse_ids = (0, 1 << 19, (1 << 20) + 2)
    return {
        "no-binding": with_bindings([], 1),
        "no-binding-no-classes": with_bindings([], 0),
        # 2 560 entries: two tiles of the device, and one class so no pass sorts anything (num_classes = 1: no key bit)
        "every-cell-one-class": with_bindings([(r, j, 0) for r, j in shuffled], 1),
        # the same list under a class id that needs every key bit of a 2^12 range
        "every-cell-one-high-class": with_bindings([(r, j, 4095) for r, j in shuffled], 4096),
        "only-singletons": with_bindings([(r, j, i) for i, (r, j) in enumerate(shuffled[:300])], 300),
        # two classes strictly interleaved, rows descending: the successor follows the LIST, not the cell order
        "interleaved-descending": with_bindings([(N - 1 - i // 2, 3 + (i % 2), i % 2) for i in range(2 * N)], 2),
        # three ids in use out of 2^20 + 3: 21 key bits, six passes, each with more than one digit in use
        "sparse-ids": with_bindings([(r, j, sparse_ids[i % 3]) for i, (r, j) in enumerate(shuffled[:1000])], big),
        "tile-minus-one": with_bindings([(r, j, (7 * i) % 5) for i, (r, j) in enumerate(shuffled[:TILE - 1])], 5),
        "tile": with_bindings([(r, j, (7 * i) % 5) for i, (r, j) in enumerate(shuffled[:TILE])], 5),
        "tile-plus-one": with_bindings([(r, j, (7 * i) % 5) for i, (r, j) in enumerate(shuffled[:TILE + 1])], 5),
        # many classes of random sizes over every cell, ids spread over 16 bits
        "random-classes": with_bindings([(r, j, int(c)) for (r, j), c in zip(shuffled, rng.integers(0, 700, size=len(shuffled)) * 93)], 65536),
    }


def without_constants():
    """base() with row_constants = NULL and fewer rows than n: zeros in the constant columns, pad_gate behind num_rows"""
    import eth_lc_plonky2_amd as m
    _, rows = base()
    return m.circuit.Rows(rows.gate_of_row[:7], 0, None, rows.bindings, rows.num_classes)


def refused_lists():
    """{label: (Rows, status, what lcp2_last_error / the model's ValueError must contain, (refusal word: index, reason) or None)}"""
    import eth_lc_plonky2_amd as m
    _, rows = base()
    good = [(1, 2, 0), (3, 4, 0), (5, 6, 1)]
    num_gates = len(base()[0].gateset.gates)
    bad_gate = rows.gate_of_row.copy()
    bad_gate[[4, 9]] = num_gates
    many = all_cells(np.random.default_rng(22))
    twice = [(r, j, i % 3) for i, (r, j) in enumerate(many[:2100])]
    twice[2077] = twice[40][:2] + (1,)      # group A: entries 40 and 2077 (in the second tile)
    twice[900] = twice[77][:2] + (2,)       # group B: entries 77 and 900
    twice[1500] = twice[40][:2] + (0,)      # a third binding of A's cell: 1500 is the one named
    return {
        "row-out-of-range": (with_bindings(good + [(N, 0, 0), (N + 1, 0, 0)], 2), -1, "binding 3: row out of range", (3, BIND_ROW)),
        "column-not-routed": (with_bindings([(0, NR, 0)] + good, 2), -1, "binding 0: column is no routed wire", (0, BIND_COLUMN)),
        "class-out-of-range": (with_bindings(good + [(7, 7, 2)], 2), -1, "binding 3: class out of range", (3, BIND_CLASS)),
        "class-with-no-classes": (with_bindings(good[:1], 0), -1, "binding 0: class out of range", (0, BIND_CLASS)),
        "range-before-twice": (with_bindings([(1, 2, 0), (1, 2, 1), (N, 0, 0)], 2), -1, "binding 2: row out of range", (2, BIND_ROW)),
        "bound-twice": (with_bindings(twice, 3), -1, "binding 1500: cell bound twice", None),
        "bound-twice-adjacent": (with_bindings([(9, 9, 0), (9, 9, 0)], 1), -1, "binding 1: cell bound twice", None),
        "gate-out-of-range": (m.circuit.Rows(bad_gate, rows.pad_gate, rows.row_constants, rows.bindings, rows.num_classes), -1,
                              "row 4: gate index out of range", (4, GATE)),
    }


def twice_pair(label):
    """(first, second) list indices of the double binding a refused list names"""
    return {"bound-twice": (40, 1500), "bound-twice-adjacent": (0, 1)}[label]


def argument_cases():
    """{label: (change to the lcp2_circuit_rows struct as a dict of fields, status, reason)}: refused before anything runs"""
    return {
        "num-rows-above-n": (dict(num_rows=N + 1), -1, "num_rows > n"),
        "pad-gate": (dict(pad_gate=1000), -1, "pad_gate out of range"),
        "null-list": (dict(bindings=None), -1, "the binding list is null"),
        "null-gate-of-row": (dict(gate_of_row=None), -1, "gate_of_row is null"),
        "bad-mem": (dict(bindings_mem=2), -1, "bad lcp2_mem"),
        "too-many-bindings": (dict(num_bindings=1 << 32), -6, "2^32 bindings or more"),
    }
