"""What tests/test_fill_copies_emu.py (CPU) and tests/test_fill_copies.py (GPU) share (test harness only): the circuits whose class
table is held to the model, hand-made permutations on a 2^5-row circuit, the two malformed sigma columns, and the cell lists of the
fill tests with their expected matrices from circuit.fill_copies_model."""
import functools

import numpy as np

import witness_check_cases as wc
from rows_lib import MAX, TAG

P = wc.P
NR, DB, N = 80, 5, 32   # the hand-made permutations: 80 routed wires, 2^5 rows, 2560 cells


def cell_dtype():
    import eth_lc_plonky2_amd as m
    return m.binding.CELL_DTYPE


def table_circuits(gpu):
    """(label, degree_bits, mix, coset_shift_base) of the circuits whose class table is compared with the model"""
    cases = [("synthetic-5", 5, False, 7), ("synthetic-7", 7, False, 7), ("mix-8", 8, True, 7), ("base-11", 6, False, 11)]
    if gpu:
        cases += [("synthetic-10", 10, False, 7), ("mix-10", 10, True, 7)]
    return cases


def hand_cycles():
    """{label: list of cycles, each a list of (wire, row)} on the 2^5-row circuit"""
    rng = np.random.default_rng(5)
    everything = [(int(c) // N, int(c) % N) for c in rng.permutation(NR * N)]
    return {
        "identity": [],
        "two-cycle": [[(3, 5), (40, 17)]],
        "three-and-five": [[(2, 1), (70, 30), (2, 2)], [(9, 9), (8, 9), (7, 9), (6, 9), (50, 0)]],
        "every-cell": [everything],                                      # 2560 cells: 12 rounds
        "first-and-last": [[(0, 0), (NR - 1, N - 1), (5, 7)]],
        "one-column-and-all-columns": [[(7, 1), (7, 4), (7, 9), (7, 30)], [(j, (3 * j + 2) % N) for j in range(NR)]],
    }


@functools.lru_cache(maxsize=None)
def hand_circuit(label, base=7):
    """the synthetic 2^5-row circuit with its sigma columns replaced by the permutation `label` names (circuit.sigma_values)"""
    import eth_lc_plonky2_amd as m
    circ, _, _ = wc.circuit(DB, False, base)
    sig_row = np.tile(np.arange(N), (NR, 1))
    sig_col = np.tile(np.arange(NR)[:, None], (1, N))
    for cyc in hand_cycles()[label]:
        for (j, r), (j2, r2) in zip(cyc, cyc[1:] + cyc[:1]):
            sig_row[j, r], sig_col[j, r] = r2, j2
    NC = circ.params.num_constants
    cs = circ.constants_sigmas.copy()
    cs[NC:NC + NR] = m.circuit.sigma_values(sig_row, sig_col, circ.k_is, DB)
    return m.circuit.Circuit(circ.params, circ.gateset, cs, circ.k_is, circ.num_public_inputs)


def hand_classes(label):
    """what the table of hand_circuit(label) must be, from the cycles themselves"""
    cycles = sorted(hand_cycles()[label], key=lambda cyc: min(j * N + r for j, r in cyc))
    want = np.full((NR, N), 0xFFFFFFFF, dtype=np.uint32)
    for k, cyc in enumerate(cycles):
        for j, r in cyc:
            want[j, r] = k
    return want, len(cycles)


def malformed(kind):
    """(circuit, refused cell (wire, row), the other cell or None): the synthetic 2^5-row circuit with one sigma value changed to
    "no-id" (a value in none of the 80 cosets) or "shared" (the id of a cell that another cell already has as its image)"""
    import eth_lc_plonky2_amd as m
    circ, _, _ = wc.circuit(DB, False)
    NC = circ.params.num_constants
    cs = circ.constants_sigmas.copy()
    if kind == "no-id":
        cs[NC + 3, 9] = np.uint64(pow(7, NR, P))
        bad, other = (3, 9), None
    else:
        # the last row is NoopGate padding: (12, 31) is its own image, which the assert holds it to
        assert cs[NC + 12, N - 1] == np.uint64(int(circ.k_is[12]) * pow(wc.root_of_unity(DB), N - 1, P) % P)
        cs[NC + 30, N - 1] = cs[NC + 12, N - 1]   # (30, 31) now points at (12, 31), which also points at itself
        bad, other = (30, N - 1), (12, N - 1)
    return m.circuit.Circuit(circ.params, circ.gateset, cs, circ.k_is, circ.num_public_inputs), bad, other


def cells_of(entries):
    out = np.zeros(len(entries), dtype=cell_dtype())
    for i, (col, row, value) in enumerate(entries):
        out[i] = (row, col, value)
    return out


def members(class_of, cls):
    """the cells (wire, row) of a class, ascending"""
    return [(int(j), int(r)) for j, r in zip(*np.nonzero(class_of == cls))]


def one_per_class(circ, wires, class_of, num_classes, rng, classes=None):
    """one randomly chosen member of every class (or of `classes`), plus - with all classes - every non-zero cell that is in no class
    or on a non-routed wire: the list from which the whole witness comes back"""
    nr = circ.params.num_routed_wires
    flat = class_of.ravel()
    order = rng.permutation(flat.size)
    order = order[flat[order] != 0xFFFFFFFF]
    _, first = np.unique(flat[order], return_index=True)
    picks = order[first]
    if classes is not None:
        picks = picks[np.isin(flat[picks], classes)]
    col, row = picks // circ.n, picks % circ.n
    if classes is None:
        free = np.ones(wires.shape, dtype=bool)
        free[:nr] = class_of == 0xFFFFFFFF
        fc, fr = np.nonzero(free & (wires != 0))
        col, row = np.concatenate([col, fc]), np.concatenate([row, fr])
    out = np.zeros(col.size, dtype=cell_dtype())
    out["row"], out["col"], out["value"] = row, col, wires[col, row]
    return out


def semantics_lists(circ, class_of, num_classes):
    """{label: (cells, host_list)} on the synthetic 2^5-row circuit: what the fill tests run through the emulation / the device and
    through the model.  Class A has two cells, class B is the longest."""
    sizes = np.bincount(class_of[class_of != 0xFFFFFFFF], minlength=num_classes)
    a, b = int(np.nonzero(sizes == 2)[0][0]), int(np.argmax(sizes))
    assert sizes[b] > 2 and a != b
    A, B = members(class_of, a), members(class_of, b)
    free = next((j, r) for j in range(NR) for r in range(N) if class_of[j, r] == 0xFFFFFFFF)
    v = 0x1234
    return {
        "owner-is-smallest-index": (cells_of([B[2] + (77,), free + (5,), B[0] + (78,), A[1] + (9,), B[1] + (77,)]), True),
        "raw-value-kept": (cells_of([A[0] + (v + P,), B[1] + (MAX,), (100, 3, TAG)]), True),
        "canonical-equal-is-no-conflict": (cells_of([A[0] + (v,), A[1] + (v + P,), B[0] + (P + 1,), B[1] + (1,)]), True),
        "three-listed-two-wrong": (cells_of([free + (1,), B[1] + (40,), B[0] + (41,), B[2] + (42,)]), True),
        "row-out-of-range-host": (cells_of([A[0] + (v,), (2, N, 7), B[0] + (3,)]), True),
        "column-out-of-range-device": (cells_of([A[0] + (v,), (135, 0, 7), B[0] + (3,), (1, N + 5, 8)]), False),
    }
