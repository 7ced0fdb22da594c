"""What tests/test_witness_check_emu.py (CPU) and tests/test_witness_check.py (GPU) share (test harness only): the circuits, the
corruptions of a witness, the row -> gate map read back from the selector columns, and the numpy reference of the copy check - a
dict from id value k_j w^r to cell over all routed cells, so it does not depend on the logarithm under test."""
import functools

import numpy as np

P = 0xFFFFFFFF00000001
ROOT_2_32 = 1753635133440165772
NO_WIRE = 0xFFFFFFFF
NONE = (1 << 64) - 1


def root_of_unity(bits):
    return pow(ROOT_2_32, 1 << (32 - bits), P)


@functools.lru_cache(maxsize=None)
def circuit(degree_bits, mix=False, coset_shift_base=7, seed=11):
    """(Circuit, wires, public inputs): the synthetic circuit, or the reference gate mix"""
    import eth_lc_plonky2_amd as m
    extra = m.u32_gates.ReferenceMix() if mix else None
    params = m.standard_params(degree_bits, 5 if mix else 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=seed, extra=extra, coset_shift_base=coset_shift_base)
    wires.setflags(write=False)
    return circ, wires, pis


def gate_of_row(circ):
    """the gate each row holds, as the check decides it: constants[selector_index][r] == selector_value (-1: none)"""
    n = circ.n
    out = np.full(n, -1, dtype=np.int64)
    for g, G in enumerate(circ.gateset.gates):
        out[circ.constants_sigmas[G.selector_index, :n] == np.uint64(G.selector_value)] = g
    return out


# the cell to change in a row of each gate: a wire the gate's constraints read.  BaseSumGate: a limb (the sum and the limb's range
# product break: two constraints, listed last to first); PoseidonGate: an S-box input of a partial round (listed first to last)
CELL_OF_GATE = {"BaseSumGate": 5, "PoseidonGate": 70}


def corrupt(wires, cells):
    """a copy of the witness with 1 added to every (wire, row) of `cells`"""
    w = wires.copy()
    for wire, row in cells:
        w[wire, row] = np.uint64((int(w[wire, row]) + 1) % P)
    return w


def gate_cases(circ):
    """{label: [(wire, row), ...]}: one cell in one row of each gate type that has constraints; row 0; row n - 1; two rows at once"""
    names, gor, n = circ.gateset.names, gate_of_row(circ), circ.n
    cases = {}
    for g, name in enumerate(names):
        rows = np.nonzero(gor == g)[0]
        if rows.size and circ.gateset.gates[g].num_constraints:
            cases[name] = [(CELL_OF_GATE.get(name, 0), int(rows[rows.size // 2]))]
    arith = np.nonzero(gor == names.index("ArithmeticGate"))[0]
    cases["row 0"] = [(0, 0)]
    cases["row n-1"] = [(0, n - 1)]   # NoopGate padding: nothing to violate
    cases["two rows"] = [(3, int(arith[-1])), (3, int(arith[0]))]
    return cases


def copy_reference(circ, wires):
    """(violations, first (row, wire) or None, its partner (row, wire) - wire NO_WIRE when the sigma value is no id) by table lookup"""
    n, NR, NC = circ.n, circ.params.num_routed_wires, circ.params.num_constants
    w, sub = root_of_unity(circ.params.degree_bits), [1] * n
    for r in range(1, n):
        sub[r] = sub[r - 1] * w % P
    cell_of = {int(circ.k_is[j]) % P * sub[r] % P: (r, j) for j in range(NR) for r in range(n)}
    sig = circ.constants_sigmas[NC:NC + NR]
    canon = wires[:NR] % np.uint64(P)
    bad = []
    for j in range(NR):
        for r in range(n):
            to = cell_of.get(int(sig[j, r]) % P)
            if to is None:
                bad.append(((r, j), (NONE, NO_WIRE)))
            elif to != (r, j) and canon[j, r] != canon[to[1], to[0]]:
                bad.append(((r, j), to))
    bad.sort()
    return (len(bad),) + (bad[0] if bad else (None, None))


def cycles(circ):
    """the copy cycles with more than one cell, longest last: lists of (row, wire)"""
    n, NR, NC = circ.n, circ.params.num_routed_wires, circ.params.num_constants
    w, sub = root_of_unity(circ.params.degree_bits), [1] * n
    for r in range(1, n):
        sub[r] = sub[r - 1] * w % P
    cell_of = {int(circ.k_is[j]) % P * sub[r] % P: (r, j) for j in range(NR) for r in range(n)}
    sig = circ.constants_sigmas[NC:NC + NR]
    seen, out = set(), []
    for j in range(NR):
        for r in range(n):
            if (r, j) in seen or cell_of[int(sig[j, r])] == (r, j):
                continue
            cyc, at = [], (r, j)
            while at not in seen:
                seen.add(at)
                cyc.append(at)
                at = cell_of[int(sig[at[1], at[0]])]
            out.append(cyc)
    return sorted(out, key=len)
