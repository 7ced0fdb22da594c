"""The C-ABI library builds, loads and exports every symbol include/lcp2.h declares (no GPU needed),
and refuses to compute without a device instead of falling back to the CPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "lcp2.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(lcp2_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"liblcp2.so does not export {n}"
    assert lib.lcp2_abi_version() == 2


def test_standard_params_match_standard_recursion_config():
    import eth_lc_plonky2_amd as m
    p = m.standard_params(22, 5)
    assert (p.num_wires, p.num_routed_wires, p.rate_bits, p.cap_height, p.num_challenges) == (135, 80, 3, 4, 2)
    assert (p.quotient_degree_factor, p.proof_of_work_bits, p.num_query_rounds) == (8, 16, 28)
    assert p.num_fri_layers == 5 and list(p.fri_arity_bits)[:5] == [4] * 5  # 22 -> 18 -> 14 -> 10 -> 6 -> 2
    p = m.standard_params(12, 5)
    assert p.num_fri_layers == 2  # 12 -> 8 -> 4
    p = m.standard_params(5, 5)
    assert p.num_fri_layers == 0


def test_no_cpu_fallback_without_device():
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    if lib.lcp2_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(m.Lcp2Error) as e:
        m.Context(0)
    assert e.value.status == -2
    assert lib.lcp2_status_str(-5) == b"witness does not satisfy the circuit"


def test_proof_layout_is_consistent_and_refuses_bad_parameters():
    """lcp2_proof_layout_of: the offsets tile the proof without gaps, agree with lcp2_proof_words, and bad parameters are refused"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    for db in (5, 12, 19, 22):
        p = m.standard_params(db, 4)
        L = m.proof_layout(p)
        capw = 4 << p.cap_height
        assert L.total == lib.lcp2_proof_words(ctypes.byref(p)) and L.cap_words == capw
        assert (L.wires_cap, L.zs_cap, L.quot_cap, L.op_constants) == (0, capw, 2 * capw, 3 * capw)
        npp = (p.num_routed_wires + p.quotient_degree_factor - 1) // p.quotient_degree_factor - 1
        ch = p.num_challenges
        assert L.op_sigmas == L.op_constants + 2 * p.num_constants and L.op_wires == L.op_sigmas + 2 * p.num_routed_wires
        assert L.op_zs == L.op_wires + 2 * p.num_wires and L.op_zs_next == L.op_zs + 2 * ch
        assert L.op_partial_products == L.op_zs_next + 2 * ch and L.op_quotient == L.op_partial_products + 2 * ch * npp
        assert L.fri_caps == L.op_quotient + 2 * ch * p.quotient_degree_factor and L.queries == L.fri_caps + p.num_fri_layers * capw
        # one query round: four initial-tree openings, then the FRI layers
        lg = p.degree_bits + p.rate_bits
        pos = 0
        for o, cols in enumerate((p.num_constants + p.num_routed_wires, p.num_wires, ch * (1 + npp), ch * p.quotient_degree_factor)):
            assert (L.q_init_off[o], L.q_init_cols[o]) == (pos, cols)
            pos += cols + 4 * (lg - p.cap_height)
        assert L.q_init_sib == lg - p.cap_height
        for l in range(p.num_fri_layers):
            lg -= p.fri_arity_bits[l]
            assert (L.q_step_off[l], L.q_step_sib[l]) == (pos, lg - p.cap_height)
            pos += (2 << p.fri_arity_bits[l]) + 4 * (lg - p.cap_height)
        assert L.query_words == pos and L.final_poly == L.queries + p.num_query_rounds * pos
        assert L.pow_witness == L.final_poly + 2 * L.final_len and L.total == L.pow_witness + 1
    bad = m.standard_params(10, 4)
    bad.quotient_degree_factor = 0
    with pytest.raises(m.Lcp2Error):
        m.proof_layout(bad)
    bad = m.standard_params(10, 4)
    bad.cap_height = 40
    with pytest.raises(m.Lcp2Error):
        m.proof_layout(bad)
    assert lib.lcp2_proof_layout_of(None, None) != 0


def test_integration_stub_block_binds_every_header_function():
    """INTEGRATION.md section 1 is the binding a plonky2 fork would add: every function include/lcp2.h declares appears in its
    `extern "C"` block (round 3 had 27 of 68 missing)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lcp2.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    start = doc.index('extern "C" {')
    stub = doc[start:doc.index("```", start)]
    declared = list(dict.fromkeys(re.findall(r"\b(lcp2_[a-z0-9_]+)\s*\(", header)))
    missing = [f for f in declared if "fn %s(" % f not in stub]
    assert not missing, missing


def _prover_entry_points(lib):
    """(function, arguments after the handle, positions among them of the pointers the entry point requires), for every prover entry
    point of include/lcp2.h that takes an lcp2_circuit *.  Every argument is valid: non-null buffers, a fresh challenger state."""
    import numpy as np
    import eth_lc_plonky2_amd as m
    buf = np.zeros(4096, dtype=np.uint64)
    b = buf.ctypes.data_as(ctypes.c_void_p)
    ch = m.binding.ChallengerState()
    lib.lcp2_challenger_init(ctypes.byref(ch))
    chp = ctypes.byref(ch)
    dptr, words = ctypes.byref(ctypes.c_void_p()), ctypes.byref(ctypes.c_size_t())
    return [
        (lib.lcp2_prove, [b, 0, b, 4, b, 4096], [0, 2, 4]),
        (lib.lcp2_witness_stage, [b, 0], [0]),
        (lib.lcp2_prove_staged, [0, b, 4, b, 4096], []),  # the buffers are lcp2_prove's to check, once a device handle got that far
        (lib.lcp2_commit_wires, [b, 0, b], [0, 2]),
        (lib.lcp2_commit_wires_coeffs, [b, b, b], [0, 1, 2]),
        (lib.lcp2_commit_wires_rows, [b, b, b], [0, 1, 2]),
        (lib.lcp2_commit_wires_rows_begin, [b], [0]),
        (lib.lcp2_commit_wires_chunk, [b, 0, 8], [0]),
        (lib.lcp2_commit_wires_rows_finish, [b], [0]),
        (lib.lcp2_perm_zs, [b, b, b], [0, 1, 2]),
        (lib.lcp2_perm_zs_rows_begin, [b, b, b], [0, 1, 2]),
        (lib.lcp2_perm_zs_rows_finish, [b, dptr, words], [0, 1, 2]),
        (lib.lcp2_perm_zs_commit, [b], [0]),
        (lib.lcp2_quotient, [b, b, b], [0, 1, 2]),
        (lib.lcp2_quotient_values, [b, b], [0, 1]),
        (lib.lcp2_quotient_buffer, [dptr, words], [0, 1]),
        (lib.lcp2_quotient_commit, [b], [0]),
        (lib.lcp2_fri_open, [b, chp, b], [0, 1, 2]),
        (lib.lcp2_fri_open_begin, [b, chp, b], [0, 1, 2]),
        (lib.lcp2_fri_open_commit, [b], [0]),
        (lib.lcp2_fri_open_finish, [chp, b], [1]),  # the challenger state is optional here
    ], (buf, ch)


def _broken_challenger_states():
    import eth_lc_plonky2_amd as m
    full_input, long_output = m.binding.ChallengerState(), m.binding.ChallengerState()
    full_input.input_len = 8    # 8 buffered inputs duplex at once: never stored
    long_output.output_len = 9  # the output buffer holds 8
    return full_input, long_output


def test_prover_entry_points_guard_their_arguments():
    """Every prover entry point answers a null handle or a null required pointer with LCP2_E_INVALID and a verifier-only handle with
    LCP2_E_NODEVICE, the null check first; the status is looked at, not only that an error is raised."""
    import numpy as np
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    INVALID, NODEVICE = -1, -2
    circ, _, _ = m.circuit.synthetic_circuit(m.standard_params(5, 4), seed=3)
    assert circ.num_public_inputs > 0  # lcp2_prove requires the public inputs only then
    cap = np.zeros((1 << circ.params.cap_height, 4), dtype=np.uint64)
    data = m.CircuitData.verifier_only(circ, np.arange(1, 5, dtype=np.uint64), cap)  # = lcp2_verifier_create
    entries, keep = _prover_entry_points(lib)
    assert len(entries) == 21
    for fn, args, required in entries:
        assert fn(data.handle, *args) == NODEVICE, fn.__name__
        assert fn(None, *args) == INVALID, fn.__name__
        for i in required:
            holed = list(args)
            holed[i] = None
            assert fn(data.handle, *holed) == INVALID, (fn.__name__, i)
    assert lib.lcp2_witness_stage(data.handle, entries[1][1][0], 2) == INVALID  # slots 0 and 1
    assert lib.lcp2_prove_staged(data.handle, 2, *entries[2][1][1:]) == INVALID
    # a challenger state that no lcp2_challenger_* call can have produced
    buf = keep[0].ctypes.data_as(ctypes.c_void_p)
    for bad in _broken_challenger_states():
        assert lib.lcp2_challenger_observe(ctypes.byref(bad), buf, 4) == INVALID
        assert lib.lcp2_challenger_get(ctypes.byref(bad), buf, 4) == INVALID
        # the opening looks at the state after the handle (with a device handle: test_fri_open_refuses_a_broken_challenger_state)
        assert lib.lcp2_fri_open(data.handle, buf, ctypes.byref(bad), buf) == NODEVICE
        assert lib.lcp2_fri_open_begin(data.handle, buf, ctypes.byref(bad), buf) == NODEVICE
    # what a verifier-only handle does serve
    first, count = ctypes.c_size_t(), ctypes.c_size_t()
    layout = m.proof_layout(circ.params)
    for section, want in ((m.binding.SECTION_OPENINGS, (layout.op_constants, layout.fri_caps - layout.op_constants)),
                          (m.binding.SECTION_FRI_CAP0, (layout.fri_caps, layout.cap_words if circ.params.num_fri_layers else 0)),
                          (m.binding.SECTION_AFTER_CAPS, (layout.op_constants, layout.total - layout.op_constants))):
        assert lib.lcp2_proof_section(data.handle, section, ctypes.byref(first), ctypes.byref(count)) == 0
        assert (first.value, count.value) == want
    assert lib.lcp2_proof_section(data.handle, 3, ctypes.byref(first), ctypes.byref(count)) == INVALID
    assert lib.lcp2_proof_section(None, 0, ctypes.byref(first), ctypes.byref(count)) == INVALID
    digest, got_cap = data.digest()
    assert list(digest) == [1, 2, 3, 4] and (got_cap == cap).all()
    assert lib.lcp2_circuit_digest(None, buf, None) == INVALID
    data.close()


@pytest.mark.gpu
def test_fri_open_refuses_a_broken_challenger_state(gpu_ctx):
    """lcp2_fri_open / _begin on a device handle: LCP2_E_INVALID for a challenger state with 8 buffered inputs or 9 outputs, decided
    before the stage is looked at (that refusal would leave its reason in lcp2_last_error)"""
    import numpy as np
    import eth_lc_plonky2_amd as m
    lib = gpu_ctx.lib
    circ, _, _ = m.circuit.synthetic_circuit(m.standard_params(5, 4), seed=3)
    data = m.CircuitData.build(gpu_ctx, circ)
    words = np.zeros(data.proof_words, dtype=np.uint64)
    buf = words.ctypes.data_as(ctypes.c_void_p)
    before = lib.lcp2_last_error(gpu_ctx.handle)
    for bad in _broken_challenger_states():
        assert lib.lcp2_fri_open(data.handle, buf, ctypes.byref(bad), buf) == -1
        assert lib.lcp2_fri_open_begin(data.handle, buf, ctypes.byref(bad), buf) == -1
    assert lib.lcp2_last_error(gpu_ctx.handle) == before
    good = m.binding.ChallengerState()
    assert lib.lcp2_fri_open(data.handle, buf, ctypes.byref(good), buf) == -1  # no quotient committed: the same status, with a reason
    assert b"quotient is not committed" in lib.lcp2_last_error(gpu_ctx.handle)
    data.close()
