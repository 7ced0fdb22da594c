"""lcp2_circuit_rows_expand without a GPU: csrc/circuit_rows.hpp compiled for the CPU (tests/emu/emu_rows.cpp) with the kernels' tiling -
threads x run entries per tile, each lane ranking its own run - as parameters, so that short lists cross tile borders.  The matrix is
held to circuit.expand_rows_model (the list-order rule written independently, as a dict of lists) and, for whole circuits, to the
circuit's own constants_sigmas word for word."""
import ctypes

import numpy as np
import pytest

import circuit_rows_cases as rc
from rows_lib import build_emu, vp

TILINGS = [(256, 8), (64, 1), (3, 5), (1, 1)]   # (threads, run): the device's, one entry per lane, odd sizes, one entry per tile


@pytest.fixture(scope="module")
def emur():
    c, V = ctypes, ctypes.c_void_p
    return build_emu("emu_rows", (("emu_rows_args", c.c_int, [V, V, c.POINTER(c.c_char_p)]), ("emu_rows_problem_str", c.c_char_p, [c.c_uint]),
                                  ("emu_rows_passes", c.c_uint, [c.c_uint]),
                                  ("emu_rows_expand", c.c_int, [V, V, c.c_uint, c.c_uint, c.c_int, V, V])))


def structs(circ, rows):
    import eth_lc_plonky2_amd as m
    desc, keep = m.binding._describe(circ, 0)
    r, keep_rows = m.binding._describe_rows(rows)
    return desc, r, (keep, keep_rows)


def emu_expand(E, circ, rows, threads=256, run=8, reverse=0):
    """(status, matrix, info) of the emulated expansion"""
    desc, r, keep = structs(circ, rows)
    out = np.zeros((circ.params.num_constants + circ.params.num_routed_wires, circ.n), dtype=np.uint64)
    info = np.zeros(6, dtype=np.uint64)
    status = E.emu_rows_expand(ctypes.byref(desc), ctypes.byref(r), threads, run, reverse, vp(out), vp(info))
    return status, out, [int(v) for v in info]


def model(circ, rows):
    import eth_lc_plonky2_amd as m
    return m.circuit.expand_rows_model(circ.params, circ.gateset, circ.k_is, rows)


@pytest.mark.parametrize("label,degree_bits,mix", rc.whole_circuits())
def test_whole_circuits_come_back_word_for_word(emur, label, degree_bits, mix):
    """synthetic circuit at 2^5 and 2^8 rows, the reference gate mix at 2^10: rows, constants and walked cycles in, the circuit's own matrix out"""
    circ, rows = rc.whole(degree_bits, mix)
    assert rows.bindings.size > 10 and rows.num_classes > 3
    assert (model(circ, rows) == circ.constants_sigmas).all()
    for threads, run, reverse in ((256, 8, 0), (64, 1, 1), (3, 5, 0)):
        status, got, info = emu_expand(emur, circ, rows, threads, run, reverse)
        assert status == 0 and info[:4] == [rc.NONE] * 4
        assert (got == circ.constants_sigmas).all(), (label, threads, run)


@pytest.mark.parametrize("label", list(rc.edge_lists()))
def test_edge_lists_equal_the_model(emur, label):
    """no binding, one class over all 2560 cells, singletons, interleaved classes with descending rows, sparse class ids, lists of
    tile size - 1, tile size and tile size + 1: the model's matrix under every tiling, whichever way the lanes run"""
    circ, _ = rc.base()
    rows = rc.edge_lists()[label]
    want = model(circ, rows)
    for (threads, run), reverse in zip(TILINGS, (0, 1, 0, 1)):
        status, got, info = emu_expand(emur, circ, rows, threads, run, reverse)
        assert status == 0 and (got == want).all(), (label, threads, run)
        assert info[4] == (emur.emu_rows_passes(rows.num_classes) if rows.bindings.size else 0)
        assert info[5] == -(-rows.bindings.size // (threads * run))
    # the cases are what they say
    NC = circ.params.num_constants
    identity = model(circ, rc.edge_lists()["no-binding"])
    if label in ("no-binding", "no-binding-no-classes", "only-singletons"):
        assert (want == identity).all()
    if label.startswith("every-cell"):
        assert (want[NC:] != identity[NC:]).all()   # one cycle through all cells: nobody is its own image
        assert emur.emu_rows_passes(rows.num_classes) == (0 if label == "every-cell-one-class" else 3)
    if label == "interleaved-descending":
        # class 0 on wire 3: (row 31) -> (row 30) -> ... -> (row 0) -> (row 31)
        assert want[NC + 3, 31] == identity[NC + 3, 30] and want[NC + 3, 0] == identity[NC + 3, 31] and want[NC + 4, 5] == identity[NC + 4, 4]
    if label == "sparse-ids":
        assert emur.emu_rows_passes(rows.num_classes) == 6
        # the first and the last two passes see more than one digit; the three between see one (every entry keeps its place)
        assert [len({(c >> (4 * k)) & 15 for c in (0, 1 << 19, (1 << 20) + 2)}) > 1 for k in range(6)] == [True, False, False, False, True, True]


def test_null_constants_and_padding_rows(emur):
    import eth_lc_plonky2_amd as m
    circ, _ = rc.base()
    rows = rc.without_constants()
    want = model(circ, rows)
    status, got, _ = emu_expand(emur, circ, rows)
    S, NC = circ.gateset.num_selectors, circ.params.num_constants
    assert status == 0 and (got == want).all()
    assert not got[S:NC].any() and (got[circ.gateset.gates[0].selector_index, 7:] == circ.gateset.gates[0].selector_value).all()


@pytest.mark.parametrize("label", list(rc.refused_lists()))
def test_refused_lists_name_the_smallest_index(emur, label):
    """row, column and class out of range, a cell bound twice (both list indices), a gate index out of range: the refusal words name the
    smallest index and the reason, under every tiling and lane order, and the model refuses with the same words"""
    circ, _ = rc.base()
    rows, status, message, word = rc.refused_lists()[label]
    for threads, run, reverse in ((256, 8, 0), (3, 5, 1)):
        got_status, _, info = emu_expand(emur, circ, rows, threads, run, reverse)
        assert got_status == status
        if word is not None:
            index, reason = word
            slot = 1 if reason == rc.GATE else 0
            assert info[slot] == index << 8 | reason and info[1 - slot] == rc.NONE and info[2:4] == [rc.NONE] * 2
            assert message.endswith(emur.emu_rows_problem_str(reason).decode())
        else:
            assert info[:2] == [rc.NONE] * 2 and tuple(info[2:4]) == rc.twice_pair(label)
    with pytest.raises(ValueError) as e:
        model(circ, rows)
    assert str(e.value).startswith(message)
    if word is None:
        assert "also bound by binding %d" % rc.twice_pair(label)[0] in str(e.value)


@pytest.mark.parametrize("label", list(rc.argument_cases()) + ["too-many-cells"])
def test_arguments_refused_before_anything_runs(emur, label):
    circ, rows = rc.base()
    desc, r, keep = structs(circ, rows)
    why = ctypes.c_char_p()
    assert emur.emu_rows_args(ctypes.byref(desc), ctypes.byref(r), ctypes.byref(why)) == 0 and why.value is None
    if label == "too-many-cells":
        desc.params.degree_bits = 26   # 80 x 2^26 >= 2^32
        status, reason = -6, "2^32 routed cells or more"
    else:
        change, status, reason = rc.argument_cases()[label]
        for field, value in change.items():
            setattr(r, field, value)
    assert emur.emu_rows_args(ctypes.byref(desc), ctypes.byref(r), ctypes.byref(why)) == status
    assert reason in why.value.decode()


def test_entry_points_refuse_null_arguments_without_a_device():
    """the null checks come first: LCP2_E_INVALID whatever else the arguments hold, and no handle comes back"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    circ, rows = rc.base()
    desc, r, keep = structs(circ, rows)
    out, handle = np.zeros(8, dtype=np.uint64), ctypes.c_void_p(5)
    assert lib.lcp2_circuit_rows_expand(None, ctypes.byref(desc), ctypes.byref(r), vp(out)) == -1
    assert lib.lcp2_circuit_create_from_rows(None, ctypes.byref(desc), ctypes.byref(r), ctypes.byref(handle)) == -1
    assert not out.any()
