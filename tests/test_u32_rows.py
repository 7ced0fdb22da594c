"""lcp2_u32_gate_rows: the rows of U32ArithmeticGate, U32AddManyGate, U32SubtractionGate, U32RangeCheckGate and ComparisonGate
generated on the device, one job per operation of a row.

Without a GPU: csrc/u32_rows.hpp - the per-job function the kernel runs, and the kernel's grid as a loop - compiled for the CPU
(tests/emu/emu_u32.cpp) against the integer generators and numpy fillers of u32_gates.py, the fixed edge jobs against Python
integers and against the gates' own constraint programs, witness_jobs / job_columns, and the argument checks of the entry point.
On the GPU: the same through the library, and a proof from a device-filled matrix against the host witness' and the oracle's."""
import ctypes

import numpy as np
import pytest

import gate_program_ref as ref
from rows_lib import INVALID, NONE, NW, P, DeviceMatrix, build_emu, check_null_context, upload, vp

M = 0xFFFFFFFF
ARITH, ADD, SUB, RANGE, CMP = range(5)
OPS = {ARITH: 3, ADD: 5, SUB: 6, RANGE: 7, CMP: 1}
GATE = {ARITH: "U32ArithmeticGate", ADD: "U32AddManyGate", SUB: "U32SubtractionGate", RANGE: "U32RangeCheckGate", CMP: "ComparisonGate"}


@pytest.fixture(scope="module")
def emu32():
    """tests/emu/libemu_u32.so"""
    c, V = ctypes, ctypes.c_void_p
    return build_emu("emu_u32", (("emu_u32_job_bytes", c.c_uint, []), ("emu_u32_row_columns", c.c_uint, []), ("emu_u32_kind_ops", c.c_uint, [c.c_uint]),
                                 ("emu_u32_job_problem", c.c_uint, [V, c.c_uint64]), ("emu_u32_job_cells", c.c_uint, [V, V, V, c.c_uint]),
                                 ("emu_u32_no_problem", c.c_uint64, []), ("emu_u32_problem_str", c.c_char_p, [c.c_uint]),
                                 ("emu_u32_gate_rows", None, [V, c.c_uint64, V, c.c_uint64, V, c.c_uint, c.c_uint])))


def make_jobs(items):
    """[(row, kind, op, inputs)] -> the record array"""
    import eth_lc_plonky2_amd as m
    jobs = np.zeros(len(items), dtype=m.binding.U32_JOB_DTYPE)
    for i, (row, kind, op, ins) in enumerate(items):
        jobs[i]["row"], jobs[i]["kind"], jobs[i]["op"] = row, kind, op
        jobs[i]["in"][:len(ins)] = ins
    return jobs


def emu_cells(E, job):
    """{column: value} of one job (a one-element record array) through the emulation; every column at most once"""
    cols, vals = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.uint64)
    k = E.emu_u32_job_cells(vp(job), vp(cols), vp(vals), 256)
    assert k <= 256 and len(set(cols[:k].tolist())) == k
    return {int(c): int(v) for c, v in zip(cols[:k], vals[:k])}


def digits(x, count):
    return [(x >> (2 * j)) & 3 for j in range(count)]


def expected_cells(kind, op, ins):
    """{column: value} in Python integers, from the gates' docstrings in u32_gates.py"""
    out = {}
    if kind == ARITH:
        m0, m1, addend = ins
        v = m0 * m1 + addend
        lo, hi = v & M, v >> 32
        for k, x in enumerate((m0, m1, addend, lo, hi, pow((M - hi) % P, P - 2, P))):
            out[6 * op + k] = x
        for j, d in enumerate(digits(v, 32)):
            out[18 + 32 * op + j] = d
    elif kind == ADD:
        total = sum(ins)
        for k, x in enumerate(list(ins) + [total & M, total >> 32]):
            out[6 * op + k] = x
        for j, d in enumerate(digits(total, 18)):
            out[30 + 18 * op + j] = d
    elif kind == SUB:
        x, y, borrow = ins
        d = x - y - borrow
        ob = 1 if d < 0 else 0
        res = d + (ob << 32)
        for k, v in enumerate((x, y, borrow, res, ob)):
            out[5 * op + k] = v
        for j, dd in enumerate(digits(res, 16)):
            out[30 + 16 * op + j] = dd
    elif kind == RANGE:
        out[op] = ins[0]
        for j, d in enumerate(digits(ins[0], 16)):
            out[7 + 16 * op + j] = d
    else:
        a, b = ins
        out[0], out[1] = a, b
        so_far = 0
        for i in range(16):
            fc, sc = (a >> (2 * i)) & 3, (b >> (2 * i)) & 3
            diff = (sc - fc) % P
            eq = 1 if diff == 0 else 0
            out[4 + i], out[20 + i] = fc, sc
            out[36 + i] = 0 if eq else pow(diff, P - 2, P)
            out[52 + i] = eq
            out[68 + i] = eq * so_far % P
            so_far = (out[68 + i] + (1 - eq) * diff) % P
        out[3] = so_far
        total = (4 + so_far) % P
        for i in range(3):
            out[84 + i] = (total >> i) & 1
        out[2] = (total >> 2) & 1
    return out


# (kind, inputs, {column offset within the operation's routed wires: value the issue names})
EDGE_JOBS = [
    (ARITH, (0, 0, 0), {3: 0, 4: 0, 5: pow(M, P - 2, P)}),
    (ARITH, (M, M, M), {3: 0, 4: M, 5: 0}),            # output_high = 2^32 - 1: no inverse, output_low = 0
    (ARITH, (M, M, 0), {3: 1, 4: M - 1, 5: 1}),
    (ADD, (M, M, M, M), {4: 0xFFFFFFFC, 5: 3}),
    (SUB, (0, M, 1), {3: 0, 4: 1}),
    (SUB, (0, 0, 1), {3: M, 4: 1}),
    (SUB, (5, 5, 0), {3: 0, 4: 0}),
    (RANGE, (0,), {}),
    (RANGE, (M,), {}),
    (CMP, (7, 7), {2: 1, 3: 0}),
    (CMP, (M, 0), {2: 0, 3: P - 3}),
    (CMP, (0, M), {2: 1, 3: 3}),
]


def edge_items():
    """every edge job in every operation slot of its gate, each in a row of its own: (row, kind, op, inputs, named values)"""
    items = []
    for kind, ins, named in EDGE_JOBS:
        for op in range(OPS[kind]):
            items.append((len(items), kind, op, ins, named))
    return items


def named_base(kind, op):
    return {ARITH: 6 * op, ADD: 6 * op, SUB: 5 * op, RANGE: op, CMP: 0}[kind]


def constraints(gs, name, row):
    """the constraints a gate's program (include/lcp2.h instruction set, the arithmetic subset these gates use) emits on one row"""
    g = gs.gates[gs.index(name)]
    code, imm = gs.code[2 * g.code_offset:2 * (g.code_offset + g.code_len)], gs.imm
    for op, _, kinds, _ in ref.decode(code):
        assert op in (ref.OP_ADD, ref.OP_SUB, ref.OP_MUL, ref.OP_EMIT), op
        assert all(k in (ref.KIND_REG, ref.KIND_WIRE, ref.KIND_IMM) for k in kinds[:ref.num_sources(op)]), kinds
    emitted = ref.emitted_constraints(code, imm, row, None, None)
    assert len(emitted) == g.num_constraints
    return emitted


# ------------------------------------------------------------------ without a GPU
def test_job_layout_and_columns(emu32):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import u32_gates as ug
    assert emu32.emu_u32_job_bytes() == 24 == ctypes.sizeof(m.binding.U32Job) == m.binding.U32_JOB_DTYPE.itemsize
    top = 0
    for kind, ops in OPS.items():
        assert emu32.emu_u32_kind_ops(kind) == ops == ug.U32_JOB_KINDS[kind][1]
        owned = [ug.job_columns(kind, op) for op in range(ops)]
        flat = [c for cols in owned for c in cols]
        assert len(set(flat)) == len(flat), "two operations of a row share a column"
        top = max(top, max(flat))
        for op in range(ops):
            assert sorted(expected_cells(kind, op, (1, 1, 1, 1)[:len(ug.U32_JOB_KINDS[kind][2](op))])) == sorted(owned[op])
    assert emu32.emu_u32_kind_ops(5) == 0
    assert top + 1 == emu32.emu_u32_row_columns() == 126


def test_random_jobs_equal_the_fillers_cell_for_cell(emu32):
    """per kind: 200 rows of the numpy filler and 8 rows of the integer generator (the corner flags included), their jobs read
    back with witness_jobs, every job through the emulated per-job function: the cells it writes are its job_columns and equal the
    generator's"""
    from eth_lc_plonky2_amd import u32_gates as ug
    fillers = {ARITH: ug.fill_u32_arithmetic, ADD: ug.fill_u32_add_many, SUB: ug.fill_u32_subtraction, RANGE: ug.fill_u32_range_check,
               CMP: ug.fill_comparison}
    rng = np.random.default_rng(32)
    for kind, name in GATE.items():
        n = 208
        wires = rng.integers(0, P, size=(NW, n), dtype=np.uint64)
        fillers[kind](wires, np.arange(200), rng)
        for r in range(200, n):
            kw = {"force_high_max": True} if kind == ARITH and r % 2 else {"equal": True} if kind == CMP and r % 2 else {}
            wires[:, r] = np.array(ug.ROW_GENERATORS[name](rng, NW, **kw), dtype=np.uint64)
        jobs = ug.witness_jobs(wires, np.zeros(n, dtype=np.int64), {name: 0})
        assert jobs.size == n * OPS[kind] >= 200
        for i in range(jobs.size):
            job = jobs[i:i + 1]
            row, op = int(job["row"][0]), int(job["op"][0])
            assert emu32.emu_u32_job_problem(vp(job), n) == 0
            cells = emu_cells(emu32, job)
            assert sorted(cells) == sorted(ug.job_columns(kind, op))
            for col, v in cells.items():
                assert v == int(wires[col, row]), (name, row, op, col)


def test_edge_jobs_equal_python_integers_and_satisfy_their_gates(emu32):
    from eth_lc_plonky2_amd import u32_gates as ug
    gs = ug.reference_gateset(native=False)
    for _, kind, op, ins, named in edge_items():
        job = make_jobs([(0, kind, op, ins)])
        cells = emu_cells(emu32, job)
        assert cells == expected_cells(kind, op, ins), (GATE[kind], op, ins)
        for off, v in named.items():
            assert cells[named_base(kind, op) + off] == v, (GATE[kind], op, ins, off)
        row = [0] * NW   # every other cell of the row is zero
        for col, v in cells.items():
            row[col] = v
        bad = [i for i, c in enumerate(constraints(gs, GATE[kind], row)) if c]
        assert not bad, (GATE[kind], op, ins, bad)
    # the interpreter does see a wrong cell: the inverse of the (M, M, 0) job must be 1
    row = [0] * NW
    for col, v in expected_cells(ARITH, 0, (M, M, 0)).items():
        row[col] = v
    row[5] = 0
    assert any(constraints(gs, GATE[ARITH], row))
    # and a row of zeros satisfies every gate but the comparison
    for kind, name in GATE.items():
        assert any(constraints(gs, name, [0] * NW)) == (kind == CMP)


def test_witness_jobs_of_a_small_mix_circuit_refill_it_on_the_cpu(emu32):
    """2^6 rows: one job per operation of every u32 / comparison row, sorted by (kind, op, row); the emulated kernel grid (blocks
    of 64 and of 256 lanes, the last one partly idle) rebuilds exactly the cells job_columns names and touches nothing else"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import u32_gates as ug
    circ, wires, _ = ug.reference_mix_circuit(m.standard_params(6, 5), seed=11)
    gate_of_row, G = ug.gate_rows(circ)
    jobs = ug.witness_jobs(wires, gate_of_row, G)
    counts = {kind: int((gate_of_row == G[name]).sum()) for kind, name in GATE.items()}
    assert all(counts.values())
    assert jobs.size == sum(counts[k] * OPS[k] for k in OPS)
    for kind in OPS:
        assert int((jobs["kind"] == kind).sum()) == counts[kind] * OPS[kind]
    key = [(int(j["kind"]), int(j["op"]), int(j["row"])) for j in jobs]
    assert key == sorted(key) and len(set(key)) == len(key)
    n = circ.n
    zeroed, owned = zeroed_and_owned(wires, gate_of_row, G)
    for threads in (64, 256):
        got, flag = zeroed.copy(), np.full(1, NONE, dtype=np.uint64)
        blocks = (jobs.size + threads - 1) // threads
        emu32.emu_u32_gate_rows(vp(jobs), jobs.size, vp(got), n, vp(flag), blocks, threads)
        assert flag[0] == NONE == emu32.emu_u32_no_problem()
        assert (got[owned] == wires[owned]).all() and (got[~owned] == zeroed[~owned]).all()
    # an invalid job in the list: it writes nothing, the others are written, the flag names it and why
    bad = jobs.copy()
    bad[7]["row"] = n
    got, flag = zeroed.copy(), np.full(1, NONE, dtype=np.uint64)
    emu32.emu_u32_gate_rows(vp(bad), bad.size, vp(got), n, vp(flag), (bad.size + 63) // 64, 64)
    assert flag[0] == (7 << 8 | 1)
    skipped = np.zeros_like(owned)
    skipped[ug.job_columns(int(jobs[7]["kind"]), int(jobs[7]["op"])), int(jobs[7]["row"])] = True
    assert (got[owned & ~skipped] == wires[owned & ~skipped]).all() and (got[~owned | skipped] == zeroed[~owned | skipped]).all()
    # two invalid jobs, the later one in another block: the flag names the lower index, neither writes
    assert jobs.size > 70
    bad[70]["kind"] = 9
    for threads in (64, 256):
        got, flag = zeroed.copy(), np.full(1, NONE, dtype=np.uint64)
        emu32.emu_u32_gate_rows(vp(bad), bad.size, vp(got), n, vp(flag), (bad.size + threads - 1) // threads, threads)
        assert flag[0] == (7 << 8 | 1)
        skipped[ug.job_columns(int(jobs[70]["kind"]), int(jobs[70]["op"])), int(jobs[70]["row"])] = True
        assert (got[owned & ~skipped] == wires[owned & ~skipped]).all() and (got[~owned | skipped] == zeroed[~owned | skipped]).all()
    only_later = jobs.copy()
    only_later[70]["kind"] = 9
    flag = np.full(1, NONE, dtype=np.uint64)
    emu32.emu_u32_gate_rows(vp(only_later), only_later.size, vp(zeroed.copy()), n, vp(flag), (jobs.size + 63) // 64, 64)
    assert flag[0] == (70 << 8 | 2)
    # the fold is a minimum: a word that already names a later job is replaced, one that names an earlier job stays
    for before, after in ((100 << 8 | 3, 70 << 8 | 2), (3 << 8 | 4, 3 << 8 | 4)):
        flag = np.full(1, before, dtype=np.uint64)
        emu32.emu_u32_gate_rows(vp(only_later), only_later.size, vp(zeroed.copy()), n, vp(flag), (jobs.size + 63) // 64, 64)
        assert flag[0] == after


def zeroed_and_owned(wires, gate_of_row, G):
    """(the witness with its u32 / comparison rows zeroed, the mask of the cells some job owns)"""
    from eth_lc_plonky2_amd import u32_gates as ug
    zeroed, owned = wires.copy(), np.zeros(wires.shape, dtype=bool)
    for kind, name in GATE.items():
        rows = np.nonzero(gate_of_row == G[name])[0]
        zeroed[:, rows] = 0
        for op in range(OPS[kind]):
            owned[np.ix_(ug.job_columns(kind, op), rows)] = True
    return zeroed, owned


BAD_JOBS = [(64, RANGE, 0, (1,)), (0, 5, 0, (1,)), (0, 0xFFFF, 0, (1,)), (0, ARITH, 3, (1, 1, 1)), (0, ADD, 5, (1, 1, 1, 1)), (0, SUB, 6, (1, 1, 0)),
            (0, RANGE, 7, (1,)), (0, CMP, 1, (1, 1)), (0, SUB, 0, (1, 1, 2))]


def test_refused_jobs(emu32):
    """the validation the host entry point and the kernel share names every refused job (64 rows), and accepts the limits"""
    for k, item in enumerate(BAD_JOBS):
        assert emu32.emu_u32_job_problem(vp(make_jobs([item])), 64) == (1, 2, 2, 3, 3, 3, 3, 3, 4)[k], item
    for item in ((63, RANGE, 6, (M,)), (0, SUB, 5, (0, M, 1)), (0, ADD, 4, (M, M, M, M)), (0, ARITH, 2, (M, M, M)), (0, CMP, 0, (M, M))):
        assert emu32.emu_u32_job_problem(vp(make_jobs([item])), 64) == 0, item


def test_entry_point_checks_its_pointers_first():
    """without a device there is no context, and the null check comes first: LCP2_E_INVALID for a null context whatever the list
    holds (a valid job, a refused one, nothing), never a crash or another status"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    good, bad = make_jobs([(0, RANGE, 0, (1,))]), make_jobs(BAD_JOBS)
    check_null_context(lambda a, mem, w: lib.lcp2_u32_gate_rows(None, *a, mem, w, 64), [(vp(good), 1), (vp(bad), bad.size), (None, 0)],
                       (m.MEM_HOST, m.MEM_DEVICE), null_wires=(None, 1))


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
def test_refill_of_a_mix_circuit(gpu_ctx):
    """256 rows, every gate of the mix at least 16 times: from the witness with its u32 / comparison rows zeroed, one call with the
    host list, and again with the list in HBM, restores every owned cell and changes no other"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import u32_gates as ug
    circ, wires, _ = ug.reference_mix_circuit(m.standard_params(8, 5), seed=21)
    gate_of_row, G = ug.gate_rows(circ)
    assert all(int((gate_of_row == G[name]).sum()) >= 16 for name in GATE.values())
    jobs = ug.witness_jobs(wires, gate_of_row, G)
    zeroed, owned = zeroed_and_owned(wires, gate_of_row, G)
    d_jobs = upload(gpu_ctx, jobs)
    for device_list in (False, True):
        dm = DeviceMatrix(gpu_ctx, zeroed)
        if device_list:
            gpu_ctx.u32_gate_rows(d_jobs, dm.ptr, circ.n, njobs=jobs.size)
        else:
            gpu_ctx.u32_gate_rows(jobs, dm.ptr, circ.n)
        got = dm.read()
        dm.free()
        assert (got[owned] == wires[owned]).all(), "an owned cell differs from the host witness"
        assert (got[~owned] == zeroed[~owned]).all(), "a cell no job owns changed"
        rest = np.ones(circ.n, dtype=bool)
        for name in GATE.values():
            rest[gate_of_row == G[name]] = False
        assert (got[:, rest] == wires[:, rest]).all()
    gpu_ctx.buffer_free(d_jobs)


@pytest.mark.gpu
def test_edge_jobs_on_the_device(gpu_ctx):
    items = edge_items()
    assert len(items) <= 64
    jobs = make_jobs([it[:4] for it in items])
    dm = DeviceMatrix(gpu_ctx, np.zeros((NW, 64), dtype=np.uint64))
    gpu_ctx.u32_gate_rows(jobs, dm.ptr, 64)
    got = dm.read()
    dm.free()
    want = np.zeros((NW, 64), dtype=np.uint64)
    for row, kind, op, ins, named in items:
        for col, v in expected_cells(kind, op, ins).items():
            want[col, row] = v
        for off, v in named.items():
            assert int(got[named_base(kind, op) + off, row]) == v, (GATE[kind], op, ins, off)
    assert (got == want).all()


def range_jobs(count, n, rng):
    """`count` range-check jobs on distinct (row, op) slots of an n-row matrix, in a shuffled order, and the matrix they give"""
    assert count <= 7 * n
    slots = rng.permutation(7 * n)[:count]
    values = rng.integers(0, 1 << 32, size=count, dtype=np.uint64)
    values[:2] = (M, 0)[:count]   # (a list of one job must leave a mark)
    want = np.zeros((NW, n), dtype=np.uint64)
    items = []
    for slot, v in zip(slots.tolist(), values.tolist()):
        row, op = slot // 7, slot % 7
        items.append((row, RANGE, op, (v,)))
        for col, x in expected_cells(RANGE, op, (v,)).items():
            want[col, row] = x
    return make_jobs(items), want


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129, 255, 256, 257])
def test_launch_boundaries(gpu_ctx, count):
    """lists around the wave (64) and the block (256): exact, and no cell outside the owned columns changes"""
    jobs, want = range_jobs(count, 256, np.random.default_rng(count))
    dm = DeviceMatrix(gpu_ctx, np.zeros((NW, 256), dtype=np.uint64))
    gpu_ctx.u32_gate_rows(jobs, dm.ptr, 256)
    got = dm.read()
    dm.free()
    assert (got == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [(4 << 20) // 24 + 1, (1 << 20) + 5])
def test_long_host_lists(gpu_ctx, count):
    """a host list one job too long for the pinned staging buffer, and one that goes up in two pieces (2^20 jobs, then 5): 1792
    jobs fill a 256-row matrix; the list repeats the first 1787 of them (equal jobs for one slot leave that value) and ends with
    the other 5, whose slots nothing earlier in the list writes"""
    base, want = range_jobs(1792, 256, np.random.default_rng(5))
    jobs = np.concatenate([np.resize(base[:1787], count - 5), base[1787:]])
    assert jobs.size == count
    dm = DeviceMatrix(gpu_ctx, np.zeros((NW, 256), dtype=np.uint64))
    gpu_ctx.u32_gate_rows(jobs, dm.ptr, 256)
    got = dm.read()
    dm.free()
    assert (got == want).all()


@pytest.mark.gpu
def test_refusals_on_the_device(gpu_ctx):
    import eth_lc_plonky2_amd as m
    lib = gpu_ctx.lib
    n = 64
    good, want = range_jobs(100, n, np.random.default_rng(9))
    for k, item in enumerate(BAD_JOBS):
        at = (0, 50, 100)[k % 3]
        mixed = np.concatenate([good[:at], make_jobs([item]), good[at:]])
        # a host list: nothing at all is written
        dm = DeviceMatrix(gpu_ctx, np.zeros((NW, n), dtype=np.uint64))
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, vp(mixed), mixed.size, m.MEM_HOST, ctypes.c_void_p(dm.ptr), n) == INVALID
        reason = lib.lcp2_last_error(gpu_ctx.handle)
        assert b"job %d" % at in reason, reason
        assert not dm.read().any()
        with pytest.raises(m.Lcp2Error) as e:
            gpu_ctx.u32_gate_rows(mixed, dm.ptr, n)
        assert e.value.status == INVALID
        # the same list in HBM: refused after the fact, the valid jobs are written and the bad one wrote nothing
        d_jobs = upload(gpu_ctx, mixed)
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, ctypes.c_void_p(d_jobs), mixed.size, m.MEM_DEVICE, ctypes.c_void_p(dm.ptr), n) == INVALID
        assert b"job %d" % at in lib.lcp2_last_error(gpu_ctx.handle)
        assert (dm.read() == want).all()
        gpu_ctx.buffer_free(d_jobs)
        dm.free()
    dm = DeviceMatrix(gpu_ctx, np.zeros((NW, n), dtype=np.uint64))
    wp = ctypes.c_void_p(dm.ptr)
    for mem in (m.MEM_HOST, m.MEM_DEVICE):
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, vp(good), 0, mem, wp, n) == 0
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, None, 0, mem, wp, n) == 0
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, None, 1, mem, wp, n) == INVALID
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, vp(good), 1, mem, None, n) == INVALID
        assert lib.lcp2_u32_gate_rows(None, vp(good), 1, mem, wp, n) == INVALID
    assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, vp(good), 1, 2, wp, n) == INVALID
    assert not dm.read().any()
    gpu_ctx.u32_gate_rows(good, dm.ptr, n)   # the context still works after the refusals
    assert (dm.read() == want).all()
    dm.free()


@pytest.mark.gpu
def test_two_refused_jobs_in_a_device_list(gpu_ctx, emu32):
    """600 jobs in HBM (three blocks of 256 lanes) with two refused ones, the later one in the first wave of the last block, the
    earlier one in the middle block: the call names the lower index and its reason, whichever lane ran first; both write nothing"""
    import eth_lc_plonky2_amd as m
    lib = gpu_ctx.lib
    n = 128
    good, want = range_jobs(598, n, np.random.default_rng(19))
    first, second = make_jobs([BAD_JOBS[8]]), make_jobs([(n, RANGE, 0, (1,))])   # borrow above 1; then row out of range
    for lo, hi in ((300, 513), (0, 599), (255, 256)):
        mixed = np.concatenate([good[:lo], first, good[lo:hi - 1], second, good[hi - 1:]])
        assert mixed.size == 600 and emu32.emu_u32_job_problem(vp(mixed[lo:lo + 1]), n) == 4 and emu32.emu_u32_job_problem(vp(mixed[hi:hi + 1]), n) == 1
        dm = DeviceMatrix(gpu_ctx, np.zeros((NW, n), dtype=np.uint64))
        d_jobs = upload(gpu_ctx, mixed)
        assert lib.lcp2_u32_gate_rows(gpu_ctx.handle, ctypes.c_void_p(d_jobs), mixed.size, m.MEM_DEVICE, ctypes.c_void_p(dm.ptr), n) == INVALID
        reason = lib.lcp2_last_error(gpu_ctx.handle)
        assert b"job %d:" % lo in reason and emu32.emu_u32_problem_str(4) in reason and b"job %d:" % hi not in reason, reason
        assert emu32.emu_u32_problem_str(4) == b"subtraction borrow above 1"
        assert (dm.read() == want).all()
        gpu_ctx.buffer_free(d_jobs)
        dm.free()


@pytest.mark.gpu
def test_proof_from_a_device_filled_matrix(gpu_ctx, oracle):
    """2^10 rows: the u32 / comparison rows of the device matrix are zeroed and refilled with one call; the proof from that matrix
    (LCP2_MEM_DEVICE) equals the proof from the host witness - the same witness with the cells no job owns on those rows at zero,
    which is what a caller that zeroes the matrix has - and the oracle's proof of it, word for word, and verifies"""
    import eth_lc_plonky2_amd as m
    import oracle_lib
    from eth_lc_plonky2_amd import u32_gates as ug
    circ, wires, pis = ug.reference_mix_circuit(m.standard_params(10, 5), seed=31)
    gate_of_row, G = ug.gate_rows(circ)
    jobs = ug.witness_jobs(wires, gate_of_row, G)
    zeroed, owned = zeroed_and_owned(wires, gate_of_row, G)
    host = np.where(owned, wires, zeroed)
    assert not (zeroed == host).all()
    oc = oracle_lib.OracleCircuit(oracle, circ)
    assert oc.check_witness(host, pis)[0] == 0
    want = oc.prove(host, pis)
    oc.close()
    data = m.CircuitData.build(gpu_ctx, circ)
    from_host = data.prove(host, pis)
    dm = DeviceMatrix(gpu_ctx, zeroed)
    with pytest.raises(m.Lcp2Error) as e:   # a zeroed ComparisonGate row is not satisfied: the refill is what makes the proof
        data.prove(dm.ptr, pis, mem=m.MEM_DEVICE)
    assert e.value.status == m.binding.E_UNSAT
    gpu_ctx.u32_gate_rows(jobs, dm.ptr, circ.n)
    got = data.prove(dm.ptr, pis, mem=m.MEM_DEVICE)
    dm.free()
    assert (got == from_host).all(), "the proof from the device-filled matrix differs from the host witness' proof"
    assert (got == want).all(), "the proof differs from the oracle's"
    data.verify(got, pis)
    data.close()
