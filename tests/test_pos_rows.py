"""lcp2_poseidon_gate_rows: the rows of PoseidonGate generated on the device, one job per row.

Without a GPU: csrc/pos_rows.hpp - the row function the kernel and the host's poseidon_gate_row run, and the kernel's grid as a
loop - compiled for the CPU (tests/emu/emu_pos.cpp) against poseidon_py.gate_row / permute, and the argument checks of the entry
point.  (The host row generator with its AVX2 MDS layer against the same text: tests/cpp test_poseidon_gate_outputs_match_rows.)
On the GPU: the same through the library, against the emulation's matrix."""
import ctypes

import numpy as np
import pytest

from rows_lib import INVALID, MAX, NW, P, TAG, DeviceMatrix, build_emu, check_null_context, vp


@pytest.fixture(scope="module")
def emup():
    """tests/emu/libemu_pos.so"""
    c, V = ctypes, ctypes.c_void_p
    return build_emu("emu_pos", (("emu_pos_row_bytes", c.c_uint, []), ("emu_pos_gate_wires", c.c_uint, []), ("emu_pos_row_problem", c.c_uint, [V, c.c_uint64]),
                                 ("emu_pos_row_cells", c.c_uint, [V, V, V, c.c_uint]),
                                 ("emu_pos_gate_rows", None, [V, c.c_uint64, V, c.c_uint64, c.c_uint, c.c_uint])))


def make_rows(items):
    """[(row, swap, 12 inputs)] -> the record array"""
    import eth_lc_plonky2_amd as m
    rows = np.zeros(len(items), dtype=m.binding.POSEIDON_ROW_DTYPE)
    for i, (row, swap, ins) in enumerate(items):
        rows[i]["row"], rows[i]["swap"] = row, swap
        rows[i]["in"][:] = np.array(ins, dtype=np.uint64)
    return rows


def edge_inputs():
    """(inputs, swap): all 0, all p - 1, inputs of p and of 2^64 - 1 (non-canonical), the first four equal to the next four with
    swap = 1 (deltas 0)"""
    rng = np.random.default_rng(7)
    same = [int(x) for x in rng.integers(0, P, size=4, dtype=np.uint64)]
    rest = [int(x) for x in rng.integers(0, P, size=4, dtype=np.uint64)]
    cases = []
    for swap in (0, 1):
        cases += [([0] * 12, swap), ([P - 1] * 12, swap), ([P] * 12, swap), ([MAX] * 12, swap),
                  ([P, MAX, 0, P - 1, MAX, P, 1, P + 1, P, MAX, P - 1, 0], swap)]
    cases.append((same + same + rest, 1))
    return cases


def random_inputs(count, seed):
    rng = np.random.default_rng(seed)
    return [([int(x) for x in rng.integers(0, 1 << 64, size=12, dtype=np.uint64)], k & 1) for k in range(count)]


def check_row(E, ins, swap):
    """the three properties of one job through the emulated row function"""
    from eth_lc_plonky2_amd import poseidon_py as pp
    cols, vals = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.uint64)
    k = E.emu_pos_row_cells(vp(make_rows([(0, swap, ins)])), vp(cols), vp(vals), 256)
    assert k == NW and sorted(cols[:k].tolist()) == list(range(NW)), "the stores do not cover every column exactly once"
    got = [0] * NW
    for c, v in zip(cols[:k].tolist(), vals[:k].tolist()):
        got[c] = v
    want = pp.gate_row(ins, swap)
    for c in range(NW):
        assert got[c] == want[c], (ins, swap, c)
    state = [x % P for x in ins]
    if swap:
        state[0:4], state[4:8] = state[4:8], state[0:4]
    assert got[12:24] == pp.permute(state)
    return got


# ------------------------------------------------------------------ without a GPU
def test_row_layout(emup):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import poseidon_py as pp
    assert emup.emu_pos_row_bytes() == 104 == m.binding.POSEIDON_ROW_DTYPE.itemsize
    assert emup.emu_pos_gate_wires() == NW == pp.NUM_WIRES


def test_random_rows_equal_the_python_row(emup):
    for ins, swap in random_inputs(24, 1):
        check_row(emup, ins, swap)


def test_edge_rows_equal_the_python_row(emup):
    cases = edge_inputs()
    for ins, swap in cases:
        row = check_row(emup, ins, swap)
        assert all(v < P for v in row)
    ins, swap = cases[-1]
    assert check_row(emup, ins, swap)[25:29] == [0, 0, 0, 0]
    assert any(check_row(emup, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], 1)[25:29])


def test_refused_rows(emup):
    n = 64
    assert emup.emu_pos_row_problem(vp(make_rows([(n, 0, [0] * 12)])), n) == 1
    assert emup.emu_pos_row_problem(vp(make_rows([(0, 2, [0] * 12)])), n) == 2
    assert emup.emu_pos_row_problem(vp(make_rows([(0xFFFFFFFF, 0, [0] * 12)])), n) == 1
    assert emup.emu_pos_row_problem(vp(make_rows([(n - 1, 1, [MAX] * 12)])), n) == 0


def grid_jobs(count, n, seed):
    """`count` jobs on distinct rows of an n-row matrix in a shuffled order, the edge inputs first"""
    assert count <= n
    rng = np.random.default_rng(seed)
    rows = rng.permutation(n)[:count].tolist()
    inputs = (edge_inputs() + random_inputs(count, seed))[:count]
    return make_rows([(row, swap, ins) for row, (ins, swap) in zip(rows, inputs)])


def emu_matrix(E, jobs, n, threads=64):
    got = np.full((NW, n), TAG, dtype=np.uint64)
    E.emu_pos_gate_rows(vp(jobs), jobs.size, vp(got), n, (jobs.size + threads - 1) // threads, threads)
    return got


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_grid_writes_its_rows_and_nothing_else(emup, count):
    from eth_lc_plonky2_amd import poseidon_py as pp
    n = 128
    jobs = grid_jobs(count, n, count)
    got = emu_matrix(emup, jobs, n)
    mine = np.zeros(n, dtype=bool)
    mine[jobs["row"]] = True
    assert (got[:, ~mine] == TAG).all(), "a cell outside the jobs' rows changed"
    assert (got[:, mine] != TAG).all()
    for j in jobs[:3].tolist() + jobs[-1:].tolist():
        row, swap, ins = j
        assert got[:, row].tolist() == pp.gate_row([int(x) for x in ins], swap)


def test_entry_point_checks_its_pointers_first():
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    good, bad = make_rows([(0, 0, [1] * 12)]), make_rows([(64, 0, [1] * 12)])
    check_null_context(lambda a, mem, w: lib.lcp2_poseidon_gate_rows(None, *a, w, 64), [(vp(good), 1), (vp(bad), 1), (None, 0)])


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_device_rows_equal_the_emulation(gpu_ctx, emup, count):
    """a tagged 135 x 256 matrix (257 jobs: one row twice, with the same inputs): exactly the emulation's matrix"""
    n = 256
    jobs = grid_jobs(min(count, n), n, 100 + count)
    if count > n:
        jobs = np.concatenate([jobs, jobs[:count - n]])
    want = emu_matrix(emup, jobs, n)
    dm = DeviceMatrix(gpu_ctx, np.full((NW, n), TAG, dtype=np.uint64))
    gpu_ctx.poseidon_gate_rows(jobs, dm.ptr, n)
    got = dm.read()
    dm.free()
    assert (got == want).all()


@pytest.mark.gpu
def test_refused_lists_write_nothing(gpu_ctx, emup):
    import eth_lc_plonky2_amd as m
    n = 256
    good = grid_jobs(100, n, 9)
    dm = DeviceMatrix(gpu_ctx, np.full((NW, n), TAG, dtype=np.uint64))
    for bad in (make_rows([(n, 0, [1] * 12)]), make_rows([(0, 2, [1] * 12)])):
        for at in (0, 50, 100):
            mixed = np.concatenate([good[:at], bad, good[at:]])
            with pytest.raises(m.Lcp2Error) as e:
                gpu_ctx.poseidon_gate_rows(mixed, dm.ptr, n)
            assert e.value.status == INVALID
            assert (dm.read() == TAG).all()
    gpu_ctx.poseidon_gate_rows(good, dm.ptr, n)   # the context still works after the refusals
    assert (dm.read() == emu_matrix(emup, good, n)).all()
    dm.free()
