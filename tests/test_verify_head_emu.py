"""The device head of lcp2_verify_batch_ex without a GPU: csrc/verify_head.hpp compiled for the CPU (tests/emu/emu_verify_head.cpp)
and run in the decomposition of kernels_verify_head.hip - a group-shaped transcript, the identity per (proof, gate slot) with the
registers in the kernel's LDS layout, the finish - next to verify_head(), the host's head over the same text.  Proofs come from the
oracle prover and the expected code of every case is orc_verify's."""
import ctypes

import numpy as np
import pytest

import verify_batch_cases as vc
import verify_head_cases as hc
from rows_lib import build_emu, vp


@pytest.fixture(scope="module")
def emuh():
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_verify_head", (("emu_head_block_bytes", c.c_uint, []),
                                         ("emu_head_batch", c.c_int, [V, V, V, U, U, V, U, V, V, V, V]),
                                         ("emu_head_gate_sums", c.c_int, [V, V, V, V, V, V])))


def run_heads(E, cases):
    """(labels, want, device codes, host codes, device blocks, host blocks) of a batch through both forms of the head"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = cases
    desc, keep = m.binding._describe(circ, 0)
    dg = np.ascontiguousarray(digest, dtype=np.uint64)
    k, nb = proofs.shape[0], E.emu_head_block_bytes()
    dev, host = np.full(k, -9, dtype=np.int32), np.full(k, -9, dtype=np.int32)
    dev_blocks, host_blocks = np.zeros((k, nb), dtype=np.uint8), np.zeros((k, nb), dtype=np.uint8)
    assert E.emu_head_batch(ctypes.byref(desc), vp(dg), vp(proofs), proofs.shape[1], k, vp(pis), pis.shape[1], vp(dev), vp(host), vp(dev_blocks),
                            vp(host_blocks)) == 0
    return labels, want, dev, host, dev_blocks, host_blocks


def check_heads(E, cases):
    """the head's code is the oracle's where the oracle stops in the head (1, 2, 3) and 0 where it goes on to the queries (0, 4..7),
    in both forms; the two challenge blocks are equal byte for byte, and written, for every proof whose head passes"""
    labels, want, dev, host, dev_blocks, host_blocks = run_heads(E, cases)
    expect = np.where(want >= 4, 0, want)
    wrong = [(l, int(d), int(h), int(w)) for l, d, h, w in zip(labels, dev, host, expect) if d != w or h != w]
    assert not wrong, (len(wrong), wrong[:8])
    assert (dev_blocks == host_blocks).all(), [l for l, a, b in zip(labels, dev_blocks, host_blocks) if (a != b).any()][:8]
    passed = expect == 0
    assert dev_blocks[passed].any(axis=1).all() and not dev_blocks[~passed].any()
    return labels, want


def test_the_circuits_execute_the_whole_format():
    hc.assert_format_is_covered()


@pytest.mark.parametrize("name", hc.circuit_names())
def test_emulated_device_head_names_the_oracles_check(emuh, name):
    """every case of the circuit's batch: the kernels' decomposition and verify_head() give the oracle's code and the same block"""
    labels, want = check_heads(emuh, hc.batch(name))
    assert want[0] == 0 and (want[1:] != 0).all()


@pytest.mark.parametrize("name", hc.IDENTITY_CIRCUITS)
def test_emulated_device_head_over_the_identity_stratum(emuh, name):
    """unsatisfied witnesses proved with an honest proof of work - one per gate, a broken copy, alpha = 0: check 3 and nothing else"""
    cases = hc.identity_stratum(name)
    labels, want = check_heads(emuh, cases)
    assert labels[0] == "clean" and want[0] == 0 and (want[1:] == 3).all() and len(labels) >= 4


def test_emulated_device_head_over_the_head_sweep(emuh):
    """every word outside the query section of synthetic_5 changed in one proof each"""
    labels, want = check_heads(emuh, vc.sweep("synthetic_5", "head"))
    assert set(want) <= {2, 3} and 2 in set(want)


@pytest.mark.parametrize("name", ["synthetic_6", hc.MIXED, "pi13_6"])
def test_gate_slots_sum_to_eval_gates_filtered(emuh, name):
    """the per-gate sums of head_gate_slot, registers in the LDS layout and cleared per gate, add up to what the single walk of
    gate_program::eval_gates_filtered gives, on the clean proof and on every proof of the identity stratum"""
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = hc.identity_stratum(name) if name in hc.IDENTITY_CIRCUITS else hc.batch(name)
    desc, keep = m.binding._describe(circ, 0)
    dg = np.ascontiguousarray(digest, dtype=np.uint64)
    CH = circ.params.num_challenges
    for i in np.nonzero((want == 0) | (want == 3))[0]:
        got, ref = np.zeros(2 * CH, dtype=np.uint64), np.ones(2 * CH, dtype=np.uint64)
        pr, pi = np.ascontiguousarray(proofs[i]), np.ascontiguousarray(pis[i])
        assert emuh.emu_head_gate_sums(ctypes.byref(desc), vp(dg), vp(pr), vp(pi), vp(got), vp(ref)) == 0
        assert (got == ref).all() and ref.any(), labels[i]


def test_wrong_lengths_are_refused_before_anything_is_read(emuh):
    import eth_lc_plonky2_amd as m
    circ, digest, cap, labels, proofs, pis, want = hc.batch("synthetic_5")
    desc, keep = m.binding._describe(circ, 0)
    dg = np.ascontiguousarray(digest, dtype=np.uint64)
    codes = np.full(2, -9, dtype=np.int32)
    for words, npi in ((proofs.shape[1] - 1, pis.shape[1]), (proofs.shape[1] + 1, pis.shape[1]), (proofs.shape[1], pis.shape[1] + 1)):
        assert emuh.emu_head_batch(ctypes.byref(desc), vp(dg), vp(proofs), words, 1, vp(pis), npi, vp(codes), vp(codes[1:]), None, None) == -1
        assert (codes == -9).all()
