"""lcp2_check_witness without a GPU: csrc/witness_check.hpp compiled for the CPU (tests/emu/emu_check.cpp).  The walk of the staged
gate programs with the counting sink is held to orc_check_witness - count, first row, first constraint - and the cell-id decode to
the ids themselves."""
import ctypes

import numpy as np
import pytest

import oracle_lib
import witness_check_cases as wc
from rows_lib import build_emu, vp


@pytest.fixture(scope="module")
def emuc():
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_check", (("emu_check_gates", c.c_int, [V, V, V, c.c_uint, V, V]),
                                   ("emu_decode_cells", None, [V, c.c_uint, c.c_uint, V, U, V, V]),
                                   ("emu_check_copies", None, [V, V, V])))


def emu_gates(E, circ, wires, pis, threads=64):
    """(violations, first row, gate, constraint, per-gate counters) of the emulated k_witness_gates"""
    import eth_lc_plonky2_amd as m
    desc, keep = m.binding._describe(circ)
    h = np.array(m.poseidon_py.hash_no_pad([int(v) for v in pis]), dtype=np.uint64)
    out, per_gate = np.zeros(2, dtype=np.uint64), np.zeros(len(circ.gateset.gates), dtype=np.uint64)
    assert E.emu_check_gates(ctypes.byref(desc), vp(np.ascontiguousarray(wires)), vp(h), threads, vp(out), vp(per_gate)) == 0
    key = int(out[1])
    first = None if key == wc.NONE else (key >> 32, (key >> 16) & 0xFFFF, key & 0xFFFF)
    return int(out[0]), first, per_gate


@pytest.mark.parametrize("degree_bits,mix", [(5, False), (8, False), (5, True), (8, True)])
def test_counting_sink_equals_the_oracle(emuc, oracle, degree_bits, mix):
    """every gate of standard_gateset() / ReferenceMix through the staged walk: the clean witness has no violation; one changed cell
    in a row of each gate type (PoseidonGate emits first to last, BaseSumGate last to first: both index conventions), in row 0, in
    row n - 1 and in two rows at once (the first is the lower) give the oracle's count, row and plonky2 constraint index, the gate
    the row holds, and per-gate counters that are non-zero only there"""
    circ, wires, pis = wc.circuit(degree_bits, mix)
    oc = oracle_lib.OracleCircuit(oracle, circ)
    gor = wc.gate_of_row(circ)
    assert emu_gates(emuc, circ, wires, pis)[:2] == (0, None) and oc.check_witness(wires, pis)[0] == 0
    cases = wc.gate_cases(circ)
    assert {"PoseidonGate", "BaseSumGate", "ArithmeticGate"} <= set(cases) and (not mix or "ComparisonGate" in cases)
    for label, cells in cases.items():
        bad = wc.corrupt(wires, cells)
        want, first = oc.check_witness(bad, pis)
        assert (want > 0) == (label != "row n-1"), label   # the case is what it says
        for threads in (64, 24):   # 24: blocks that do not tile the rows evenly, duplicated tail lanes
            got, got_first, per_gate = emu_gates(emuc, circ, bad, pis, threads)
            assert got == want, label
            assert int(per_gate.sum()) == want
            if want:
                row, gate, constraint = got_first
                assert (row, constraint) == (int(first[0]), int(first[1])), label
                assert gate == gor[row] and (per_gate != 0).sum() <= len(cells) and per_gate[gate] != 0
                assert row == min(r for _, r in cells), label
    # the two conventions were really hit: PoseidonGate's first index lies inside its 123 constraints (counted from the front), and
    # BaseSumGate's is the sum constraint, plonky2's index 0, which its program emits LAST
    _, first, _ = emu_gates(emuc, circ, wc.corrupt(wires, cases["PoseidonGate"]), pis)
    assert circ.gateset.gates[first[1]].num_constraints == 123 and 0 < first[2] < 122
    _, first, _ = emu_gates(emuc, circ, wc.corrupt(wires, cases["BaseSumGate"]), pis)
    assert first[2] == 0 and not circ.gateset.gates[first[1]].flags & 1
    oc.close()


def ids(k_is, degree_bits, cells):
    w = wc.root_of_unity(degree_bits)
    return np.array([int(k_is[j]) * pow(w, r, wc.P) % wc.P for j, r in cells], dtype=np.uint64)


@pytest.mark.parametrize("base", [7, 11])
@pytest.mark.parametrize("degree_bits", [1, 2, 5, 10, 16, 28])
def test_cell_ids_decode_to_their_cells(emuc, degree_bits, base):
    """every id k_j w^r decodes to (j, r) - all cells at the small sizes, 2^4 sampled ones (with the corners) at the large - for
    plonky2's shifts 7^j and for another base; a value in none of the cosets, and 0, are refused"""
    import eth_lc_plonky2_amd as m
    NR, n = 80, 1 << degree_bits
    k_is = m.gl_np.powers(base, NR)
    if degree_bits <= 5:
        cells = [(j, r) for j in range(NR) for r in range(n)]
    else:
        rng = np.random.default_rng(degree_bits)
        cells = [(0, 0), (NR - 1, n - 1), (0, n - 1), (NR - 1, 0), (1, 1), (NR - 2, n // 2)]
        cells += [(int(rng.integers(NR)), int(rng.integers(n))) for _ in range(10)]
    s = ids(k_is, degree_bits, cells)
    lifted = s.copy()
    lifted[s < np.uint64(2 ** 32 - 1)] += np.uint64(wc.P)   # a non-canonical word names the same cell
    for values in (s, lifted):
        wire, row = np.zeros(len(cells), dtype=np.uint32), np.zeros(len(cells), dtype=np.uint64)
        emuc.emu_decode_cells(vp(k_is), NR, degree_bits, vp(values), len(cells), vp(wire), vp(row))
        assert [(int(j), int(r)) for j, r in zip(wire, row)] == cells
    # outside the 80 cosets: the shift base^80 (times anything in H), and 0
    outside = np.array([pow(base, NR, wc.P), pow(base, NR, wc.P) * wc.root_of_unity(degree_bits) % wc.P, 0], dtype=np.uint64)
    wire, row = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint64)
    emuc.emu_decode_cells(vp(k_is), NR, degree_bits, vp(outside), 3, vp(wire), vp(row))
    assert (wire == wc.NO_WIRE).all()


@pytest.mark.parametrize("base", [7, 11])
def test_copy_check_equals_the_table_reference(emuc, base):
    """the per-cell copy check over a whole circuit against the dict reference: clean, one cell of a 2-cycle, one cell of the long
    fan-out cycle, a sigma value that is no cell id"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(6, False, base)
    desc, keep = m.binding._describe(circ)

    def run(c, w):
        d, k = m.binding._describe(c)
        out = np.zeros(4, dtype=np.uint64)
        emuc.emu_check_copies(ctypes.byref(d), vp(np.ascontiguousarray(w)), vp(out))
        key = int(out[1])
        return int(out[0]), (None if key == wc.NONE else (key >> 32, key & 0xFFFFFFFF)), (None if key == wc.NONE else (int(out[3]), int(out[2])))

    assert run(circ, wires) == (0, None, None) == wc.copy_reference(circ, wires)
    cyc = wc.cycles(circ)
    assert len(cyc[0]) == 2 and len(cyc[-1]) > 2
    for r, j in (cyc[0][1], cyc[-1][len(cyc[-1]) // 2]):
        bad = wc.corrupt(wires, [(j, r)])
        want = wc.copy_reference(circ, bad)
        assert want[0] == 2 and run(circ, bad) == want
    NC = circ.params.num_constants
    cs = circ.constants_sigmas.copy()
    cs[NC + 3, 9] = np.uint64(pow(base, 80, wc.P))
    broken = m.circuit.Circuit(circ.params, circ.gateset, cs, circ.k_is, circ.num_public_inputs)
    want = wc.copy_reference(broken, wires)
    assert want[1] == (9, 3) and want[2] == (wc.NONE, wc.NO_WIRE) and run(broken, wires) == want
