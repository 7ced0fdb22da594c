"""lcp2_check_witness on the GPU: the gate pass against orc_check_witness, the copy pass against a table reference written here
(witness_check_cases.copy_reference), and the handle's proving state left alone (the proof made afterwards equals the oracle's).
Sizes: 2^4 (the smallest circuit the generator makes: one partial wave), 2^5 (the first BaseSumGate row), 2^8 (four waves),
2^10 of the reference gate mix (several workgroups, every gate kind)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib
import witness_check_cases as wc
from rows_lib import DeviceMatrix

pytestmark = pytest.mark.gpu

SIZES = [(4, False), (5, False), (8, False), (10, True)]
FIELDS = ("gate_violations", "gate_row", "gate_index", "gate_constraint", "copy_violations", "copy_row", "copy_wire", "copy_to_row",
          "copy_to_wire", "noncanonical_cells")


def fields(report):
    return {f: getattr(report, f) for f in FIELDS}


@functools.lru_cache(maxsize=None)
def oracle_circuit(degree_bits, mix=False, base=7):
    return oracle_lib.OracleCircuit(oracle_lib.load(), wc.circuit(degree_bits, mix, base)[0])


@functools.lru_cache(maxsize=None)
def oracle_proof(degree_bits, mix=False, base=7):
    circ, wires, pis = wc.circuit(degree_bits, mix, base)
    return oracle_circuit(degree_bits, mix, base).prove(wires, pis)


@pytest.fixture(scope="module")
def built(gpu_ctx):
    """CircuitData per circuit, built once"""
    import eth_lc_plonky2_amd as m
    cache = {}

    def get(degree_bits, mix=False, base=7):
        key = (degree_bits, mix, base)
        if key not in cache:
            cache[key] = m.CircuitData.build(gpu_ctx, wc.circuit(*key)[0])
        return cache[key]
    yield get
    for d in cache.values():
        d.close()


def assert_gates_equal_oracle(report, oc, circ, wires, pis):
    want, first = oc.check_witness(wires, pis)
    assert report.gate_violations == want
    if want:
        assert (report.gate_row, report.gate_constraint) == (int(first[0]), int(first[1]))
        assert report.gate_index == wc.gate_of_row(circ)[report.gate_row]
    else:
        assert report.gate_row == wc.NONE
    if report.per_gate is not None:
        assert int(report.per_gate.sum()) == want
    return want


def assert_copies_equal_reference(report, circ, wires):
    count, first, to = wc.copy_reference(circ, wires)
    assert report.copy_violations == count
    if count:
        assert (report.copy_row, report.copy_wire) == first and (report.copy_to_row, report.copy_to_wire) == to
    else:
        assert report.copy_row == wc.NONE and report.copy_to_wire == wc.NO_WIRE
    return count


@pytest.mark.parametrize("degree_bits,mix", SIZES)
def test_clean_witness_is_ok_and_the_handle_is_left_alone(built, degree_bits, mix):
    """all counts 0, ok; the proof made right after the call equals the oracle's word for word"""
    circ, wires, pis = wc.circuit(degree_bits, mix)
    data = built(degree_bits, mix)
    report = data.check_witness(wires, pis, per_gate=True)
    assert report.ok and not report.per_gate.any()
    assert fields(report) == dict(gate_violations=0, gate_row=wc.NONE, gate_index=0, gate_constraint=0, copy_violations=0, copy_row=wc.NONE,
                                  copy_wire=0, copy_to_row=wc.NONE, copy_to_wire=wc.NO_WIRE, noncanonical_cells=0)
    assert (data.prove(wires, pis) == oracle_proof(degree_bits, mix)).all()


@pytest.mark.parametrize("degree_bits,mix", SIZES)
def test_gate_violations_equal_the_oracle(built, degree_bits, mix):
    """one changed cell in a row of each gate type, in row 0, in row n - 1, in two rows at once: count, first row and plonky2
    constraint index are orc_check_witness's, the gate is the row's, per_gate sums to the total and is non-zero only at the gates
    of the changed rows; the copy constraints that break with the cell are the table reference's"""
    circ, wires, pis = wc.circuit(degree_bits, mix)
    data, oc, gor = built(degree_bits, mix), oracle_circuit(degree_bits, mix), wc.gate_of_row(circ)
    cases = wc.gate_cases(circ)
    assert "ArithmeticGate" in cases and ("BaseSumGate" in cases) == (degree_bits >= 5)
    for label, cells in cases.items():
        bad = wc.corrupt(wires, cells)
        report = data.check_witness(bad, pis, per_gate=True)
        want = assert_gates_equal_oracle(report, oc, circ, bad, pis)
        assert (want > 0) == (label != "row n-1"), label
        assert set(np.nonzero(report.per_gate)[0]) <= {gor[r] for _, r in cells}, label
        if want:
            assert report.gate_row == min(r for _, r in cells) and not report.ok, label
        assert_copies_equal_reference(report, circ, bad)


def test_last_row_of_a_partial_wave_counts_once(gpu_ctx, oracle):
    """2^4 rows are a quarter of a wave: 48 lanes repeat row 15 so that the wave's votes are complete.  With row 15 made an
    ArithmeticGate row of random cells its violations are counted once, not 49 times"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(4)
    cs = circ.constants_sigmas.copy()
    g = circ.gateset.index("ArithmeticGate")
    G = circ.gateset.gates[g]
    assert circ.gateset.num_selectors == 2 and G.selector_index == 0
    cs[0, 15] = G.selector_value
    changed = m.circuit.Circuit(circ.params, circ.gateset, cs, circ.k_is, circ.num_public_inputs)
    oc = oracle_lib.OracleCircuit(oracle, changed)
    data = m.CircuitData.build(gpu_ctx, changed)
    report = data.check_witness(wires, pis, per_gate=True)
    want = assert_gates_equal_oracle(report, oc, changed, wires, pis)
    assert 0 < want <= G.num_constraints and report.gate_row == 15 and report.gate_index == g and report.per_gate[g] == want
    data.close()
    oc.close()


@pytest.mark.parametrize("base", [7, 11])
def test_copy_violations_equal_the_table_reference(built, base):
    """one cell of a 2-cycle (both cells, the lower row first), one cell of the long fan-out cycle, a cell that is its own sigma
    image (nothing), each with plonky2's coset shifts and with powers of 11; the gate constraints that break with the cell are the
    oracle's"""
    circ, wires, pis = wc.circuit(5, False, base)
    data, oc = built(5, False, base), oracle_circuit(5, False, base)
    cyc = wc.cycles(circ)
    assert len(cyc[0]) == 2 and len(cyc[-1]) > 4
    NC = circ.params.num_constants
    own = [(r, j) for r, j in ((circ.n - 1, 50), (circ.n - 2, 79)) if int(circ.constants_sigmas[NC + j, r]) == int(circ.k_is[j]) * pow(wc.root_of_unity(5), r, wc.P) % wc.P]
    assert own
    for (r, j), count in ((cyc[0][1], 2), (cyc[0][0], 2), (cyc[-1][len(cyc[-1]) // 2], 2), (own[0], 0)):
        bad = wc.corrupt(wires, [(j, r)])
        report = data.check_witness(bad, pis)
        assert assert_copies_equal_reference(report, circ, bad) == count
        if (r, j) in cyc[0]:
            assert {(report.copy_row, report.copy_wire), (report.copy_to_row, report.copy_to_wire)} == set(cyc[0])
            assert (report.copy_row, report.copy_wire) == min(cyc[0])
        assert_gates_equal_oracle(report, oc, circ, bad, pis)
        assert report.ok == (count == 0 and report.gate_violations == 0)


def test_sigma_value_that_is_no_cell_id(gpu_ctx):
    """a sigma value outside the 80 cosets is a violation of its cell, with no partner"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(5)
    cs = circ.constants_sigmas.copy()
    cs[circ.params.num_constants + 3, 9] = np.uint64(pow(7, 80, wc.P))
    broken = m.circuit.Circuit(circ.params, circ.gateset, cs, circ.k_is, circ.num_public_inputs)
    data = m.CircuitData.build(gpu_ctx, broken)
    report = data.check_witness(wires, pis)
    assert assert_copies_equal_reference(report, broken, wires) == 1
    assert (report.copy_row, report.copy_wire, report.copy_to_row, report.copy_to_wire) == (9, 3, wc.NONE, wc.NO_WIRE)
    data.close()


def test_non_canonical_words_are_counted_and_compared_by_value(gpu_ctx, oracle):
    """p added to 600 cells of a witness of small values: noncanonical_cells says so and nothing is violated; a real violation on
    top of them is found"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = m.circuit.synthetic_circuit(m.standard_params(8, 4), seed=21, small_values=True)
    data, oc = m.CircuitData.build(gpu_ctx, circ), oracle_lib.OracleCircuit(oracle, circ)
    rng = np.random.default_rng(5)
    P = np.uint64(wc.P)
    lifted = wires.copy()
    room = np.argwhere(lifted < np.uint64(2 ** 32 - 1))          # x + p < 2^64  <=>  x < 2^32 - 1
    for r, c in room[rng.choice(len(room), size=600, replace=False)]:
        lifted[r, c] += P
    assert (lifted >= P).sum() == 600 and ((lifted % P) == wires).all()
    report = data.check_witness(lifted, pis)
    assert report.ok and report.noncanonical_cells == 600
    cells = wc.gate_cases(circ)["ArithmeticGate"]
    bad = wc.corrupt(lifted, cells)
    report = data.check_witness(bad, pis)
    assert assert_gates_equal_oracle(report, oc, circ, bad, pis) > 0 and report.gate_row == cells[0][1]
    assert report.noncanonical_cells == int((bad >= P).sum())
    assert_copies_equal_reference(report, circ, bad)
    data.close()
    oc.close()


def test_host_and_device_wires_give_the_same_report(gpu_ctx, built):
    """a witness in HBM is read in place and not written"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(8)
    data = built(8)
    for w in (wires, wc.corrupt(wires, wc.gate_cases(circ)["two rows"])):
        dev = DeviceMatrix(gpu_ctx, w)
        on_device = data.check_witness(dev.ptr, pis, per_gate=True, mem=m.MEM_DEVICE)
        on_host = data.check_witness(w, pis, per_gate=True)
        assert fields(on_device) == fields(on_host) and (on_device.per_gate == on_host.per_gate).all()
        assert (dev.read() == w).all()
        dev.free()
    assert not on_host.ok


def test_return_codes(gpu_ctx, built):
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(5)
    data = built(5)
    with pytest.raises(m.Lcp2Error) as e:
        data.check_witness(wires, pis[:-1])
    assert e.value.status == -1      # LCP2_E_INVALID: a wrong public-input count
    report, counts, p = m.WitnessReport(), np.zeros(len(circ.gateset.gates) + 1, dtype=np.uint64), np.ascontiguousarray(pis, dtype=np.uint64)
    args = (data.handle, wires.ctypes.data_as(ctypes.c_void_p), m.MEM_HOST, p.ctypes.data_as(ctypes.c_void_p), p.size, ctypes.byref(report),
            counts.ctypes.data_as(ctypes.c_void_p))
    assert data.lib.lcp2_check_witness(*args, len(circ.gateset.gates) + 1) == -1   # LCP2_E_INVALID: per_gate with a wrong num_gates
    assert data.lib.lcp2_check_witness(*args, len(circ.gateset.gates)) == 0 and not counts.any()
    digest, cap = data.digest()
    verifier = m.CircuitData.verifier_only(circ, digest, cap)
    with pytest.raises(m.Lcp2Error) as e:
        verifier.check_witness(wires, pis)
    assert e.value.status == -2      # LCP2_E_NODEVICE
    verifier.close()
    sharded = m.CircuitData.build_sharded(gpu_ctx, circ, 0, 4)
    with pytest.raises(m.Lcp2Error) as e:
        sharded.check_witness(wires, pis)
    assert e.value.status == -6      # LCP2_E_UNSUPPORTED: it holds only its own blocks
    sharded.close()
    assert data.check_witness(wires, pis).ok   # the refusals left the context usable


def test_check_after_a_bad_witness_then_prove(built):
    """corrupt -> check -> restore -> prove: the proof equals the oracle's"""
    circ, wires, pis = wc.circuit(8)
    data = built(8)
    bad = wc.corrupt(wires, wc.gate_cases(circ)["PoseidonGate"])
    assert not data.check_witness(bad, pis).ok
    assert (data.prove(wires, pis) == oracle_proof(8)).all()
    assert data.check_witness(wires, pis).ok


def test_check_between_the_seams_of_a_proof_in_flight(built):
    """lcp2_commit_wires -> check -> lcp2_perm_zs -> check (of ANOTHER, broken witness) -> lcp2_quotient -> check -> lcp2_fri_open,
    the transcript run by the caller: the proof equals the oracle's word for word, and every check in between reports its own
    witness"""
    import eth_lc_plonky2_amd as m
    circ, wires, pis = wc.circuit(8)
    data = built(8)
    bad = wc.corrupt(wires, wc.gate_cases(circ)["ArithmeticGate"])
    capw = 4 << circ.params.cap_height
    proof = np.zeros(data.proof_words, dtype=np.uint64)
    pi_hash = np.array(m.poseidon_py.hash_no_pad([int(v) for v in pis]), dtype=np.uint64)
    t = m.binding.Challenger()
    t.observe(data.digest()[0])
    t.observe(pi_hash)
    proof[0:capw] = data.commit_wires(wires).ravel()
    assert data.check_witness(wires, pis).ok
    t.observe(proof[0:capw])
    betas, gammas = t.get(2), t.get(2)
    proof[capw:2 * capw] = data.perm_zs(betas, gammas).ravel()
    assert data.check_witness(bad, pis, per_gate=True).gate_violations > 0
    t.observe(proof[capw:2 * capw])
    alphas = t.get(2)
    proof[2 * capw:3 * capw] = data.quotient(alphas, pi_hash).ravel()
    assert data.check_witness(wires, pis).ok
    t.observe(proof[2 * capw:3 * capw])
    data.fri_open(t.get(2), t.state, proof)
    assert (proof == oracle_proof(8)).all()
