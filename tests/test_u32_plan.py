"""lcp2_witness_plan_rows_u32 on the GPU: the plans of tests/test_u32_plan_emu.py through the library, with host lists and with lists
in HBM - equal to u32_gates.plan_u32_model cell for cell on a matrix of arbitrary words, equal word for word to what lcp2_u32_gate_rows
writes from immediate jobs resolved level by level on the host, equal to lcp2_witness_plan_rows without u32 jobs; the refusals the
device alone can see; and rows that satisfy their gates under lcp2_check_witness."""
import ctypes

import numpy as np
import pytest

from rows_lib import INVALID, NW, P, DeviceMatrix, upload
from test_u32_plan_emu import (ADD, BAD_ROW, N, REASONS, SOURCE_ROW, SUB, edge_levels, index_of, index_of_rec, mixed_levels, owned_cells, pattern,
                               plan_struct, random_plan, reason_cases, refusal_levels, refusal_start, refused_plan, rg, ug)

LISTS = ("u32_jobs", "rec_jobs", "pos_jobs", "chain_ends", "operands")


def run_on_device(ctx, plan, start, device_lists=False):
    """(the matrix after the call, the Lcp2Error it raised or None)"""
    import eth_lc_plonky2_amd as m
    dm = DeviceMatrix(ctx, start)
    ends = (plan.u32_level_ends, plan.rec_level_ends, plan.pos_level_ends)
    ptrs = [upload(ctx, getattr(plan, name)) for name in LISTS] if device_lists else []
    error = None
    try:
        if device_lists:
            ctx.witness_plan_rows_u32(*ptrs, *ends, dm.ptr, start.shape[0], start.shape[1], nu32=plan.u32_jobs.size, nrec=plan.rec_jobs.size,
                                      npos=plan.pos_jobs.size, nchains=plan.chain_ends.size, noperands=plan.operands.size)
        else:
            ctx.witness_plan_rows_u32(*[getattr(plan, name) for name in LISTS], *ends, dm.ptr, start.shape[0], start.shape[1])
    except m.Lcp2Error as e:
        error = e
    got = dm.read()
    dm.free()
    for ptr in ptrs:
        ctx.buffer_free(ptr)
    return got, error


@pytest.fixture(scope="module")
def random_case():
    """(the random plan of the emulation test, its start matrix, the model's matrix): computed once"""
    plan, start = random_plan(), pattern(N, 1)
    return plan, start, ug().plan_u32_model(start, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("device_lists", [False, True])
def test_random_plan_equals_the_model(gpu_ctx, random_case, device_lists):
    plan, start, want = random_case
    got, error = run_on_device(gpu_ctx, plan, start, device_lists)
    assert error is None and (got == want).all()
    own = owned_cells(plan, N)
    assert (got[~own] == start[~own]).all(), "a cell outside the operations was touched"


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [edge_levels, mixed_levels])
def test_edge_and_mixed_plans_equal_the_model(gpu_ctx, levels):
    plan = ug().pack_u32_plan(levels())
    start = pattern(64, 2)
    want = ug().plan_u32_model(start, plan)
    for device_lists in (False, True):
        got, error = run_on_device(gpu_ctx, plan, start, device_lists)
        assert error is None and (got == want).all(), device_lists


@pytest.mark.gpu
def test_equal_to_u32_gate_rows_level_by_level(gpu_ctx, random_case):
    """the reference is the existing call: per level the test reads the matrix back, resolves every operand on the host and queues
    immediate jobs; the two matrices agree word for word"""
    import eth_lc_plonky2_amd as m
    plan, start, want = random_case
    counts = m.binding.U32_PLAN_OPERANDS
    dm = DeviceMatrix(gpu_ctx, start)
    begin = 0
    for end in plan.u32_level_ends.tolist():
        now = dm.read()
        jobs = np.zeros(end - begin, dtype=m.binding.U32_JOB_DTYPE)
        for k, j in enumerate(plan.u32_jobs[begin:end]):
            first = int(j["first_operand"])
            vals = [int(now[int(o["col"]), int(o["v"])]) % P if o["src"] == 1 else int(o["v"]) % P for o in plan.operands[first:first + counts[int(j["kind"])]]]
            jobs[k] = (j["row"], j["kind"], j["op"], vals + [0] * (4 - len(vals)))
        if jobs.size:
            gpu_ctx.u32_gate_rows(jobs, dm.ptr, N)
        begin = end
    reference = dm.read()
    dm.free()
    got, error = run_on_device(gpu_ctx, plan, start, device_lists=True)
    assert error is None and (got == reference).all() and (reference == want).all()


@pytest.mark.gpu
def test_without_u32_jobs_it_is_witness_plan_rows(gpu_ctx):
    u = ug()
    base = u.pack_u32_plan([([], rec, chains) for _, rec, chains in mixed_levels()])
    start = pattern(64, 4)
    start[2, 10] = 1   # the swap bit the chain reads
    dm = DeviceMatrix(gpu_ctx, start)
    gpu_ctx.witness_plan_rows(base.rec_jobs, base.pos_jobs, base.chain_ends, base.operands, base.rec_level_ends, base.pos_level_ends, dm.ptr, NW, 64)
    reference = dm.read()
    dm.free()
    assert not (reference == start).all()
    for device_lists in (False, True):
        got, error = run_on_device(gpu_ctx, base, start, device_lists)
        assert error is None and (got == reference).all()


@pytest.mark.gpu
def test_refusals_by_cell_value_are_found_on_the_device(gpu_ctx):
    """a cell holding 2^32, a borrow cell holding 2: refused in the kernel from host and device lists - the refused job writes nothing,
    its level and the earlier ones are written, later levels are not, the job is named; a cell holding v + p is accepted.  Then all
    three families in one level, every structural reason from a device list, and the context still works"""
    u, g = ug(), rg()
    start = refusal_start()
    for code in (9, 4):
        plan, at, kept = refused_plan(code, by_cell=True)
        want = u.plan_u32_model(start, kept)
        for device_lists in (False, True):
            got, error = run_on_device(gpu_ctx, plan, start, device_lists)
            assert error is not None and error.status == INVALID and "plan rows: u32 job %d: " % at in str(error) and REASONS[code] in str(error), str(error)
            assert (got == want).all() and not got[:, [BAD_ROW, 7, 43, 52]].any() and got[:, [3, 4, 41, 51]].any(axis=0).all()
    levels, _ = refusal_levels((BAD_ROW, ADD, 3, [g.CELL(SOURCE_ROW, 2), g.IMM(41 + P), g.IMM(0), g.IMM(0)]))
    plan = u.pack_u32_plan(levels)
    got, error = run_on_device(gpu_ctx, plan, start, True)
    assert error is None and (got == u.plan_u32_model(start, plan)).all() and got[18:24, BAD_ROW].tolist() == [41, 41, 0, 0, 82, 0]
    bad = reason_cases(by_cell=True)[4][0]
    for bad_rec, bad_u32, bad_swap, family in ((True, True, True, "rec"), (False, True, True, "u32"), (False, False, True, "poseidon")):
        levels, kept = refusal_levels(bad if bad_u32 else None, bad_rec=bad_rec, bad_swap=bad_swap)
        plan = u.pack_u32_plan(levels)
        text = {"rec": "plan rows: rec job %d: random-access index" % (index_of_rec(plan, 30) if bad_rec else 0),
                "u32": "plan rows: u32 job %d: subtraction borrow above 1" % (index_of(plan, BAD_ROW) if bad_u32 else 0),
                "poseidon": "plan rows: poseidon job 1: swap value not 0 or 1"}[family]
        for device_lists in (False, True):
            got, error = run_on_device(gpu_ctx, plan, start, device_lists)
            assert error is not None and error.status == INVALID and text in str(error), str(error)
            assert (got == u.plan_u32_model(start, u.pack_u32_plan(kept))).all(), (family, device_lists)
    for code in REASONS:
        for bad_level in ((1,) if code % 3 else (0, 2)):
            plan, at, kept = refused_plan(code, bad_level=bad_level)
            got, error = run_on_device(gpu_ctx, plan, start)
            assert error is not None and error.status == INVALID and "plan rows: u32 job %d: " % at in str(error) and REASONS[code] in str(error)
            assert (got == start).all(), "a refused host list wrote something"
            got, error = run_on_device(gpu_ctx, plan, start, device_lists=True)
            assert error is not None and error.status == INVALID and "plan rows: u32 job %d: " % at in str(error) and REASONS[code] in str(error)
            assert (got == u.plan_u32_model(start, kept)).all(), (code, bad_level)
    good = u.pack_u32_plan(refusal_levels()[0])
    got, error = run_on_device(gpu_ctx, good, start)
    assert error is None and (got == u.plan_u32_model(start, good)).all()


@pytest.mark.gpu
def test_argument_checks(gpu_ctx):
    import eth_lc_plonky2_amd as m
    u = ug()
    lib, n = gpu_ctx.lib, 64
    good = u.pack_u32_plan(refusal_levels()[0])
    start = refusal_start()
    dm = DeviceMatrix(gpu_ctx, start)
    wp, h = ctypes.c_void_p(dm.ptr), gpu_ctx.handle
    call = lambda s, mem=m.MEM_HOST, w=wp, ncols=NW: lib.lcp2_witness_plan_rows_u32(h, ctypes.byref(s) if s is not None else None, mem, w, ncols, n)   # noqa: E731
    s, keep = plan_struct(m, good)
    assert call(None) == INVALID and call(s, w=None) == INVALID and call(s, mem=2) == INVALID and call(s, ncols=134) == INVALID
    assert b"135 columns" in lib.lcp2_last_error(h)
    for field in ("u32_jobs", "u32_level_ends"):
        s, keep = plan_struct(m, good)
        setattr(s, field, None)
        assert call(s) == INVALID and call(s, mem=m.MEM_DEVICE) == INVALID and b"null" in lib.lcp2_last_error(h), field
    for field in ("rec_jobs", "pos_jobs", "chain_ends", "operands", "rec_level_ends", "pos_level_ends"):
        s, keep = plan_struct(m, good)
        setattr(s.base, field, None)
        assert call(s) == INVALID and call(s, mem=m.MEM_DEVICE) == INVALID, field
    for field, values in (("u32_level_ends", [3, 7, 6]), ("u32_level_ends", [3, 2, 7]), ("rec_level_ends", [1, 3, 2]), ("pos_level_ends", [1, 2, 2])):
        broken = type(good)(**vars(good))
        setattr(broken, field, np.array(values, dtype=np.uint32))
        s, keep = plan_struct(m, broken)
        assert call(s) == INVALID and field.encode() in lib.lcp2_last_error(h), (field, values)
    s, keep = plan_struct(m, good, {"nu32": 1 << 32})
    assert call(s, mem=m.MEM_DEVICE) == INVALID and b"2^32 - 1" in lib.lcp2_last_error(h)
    s, keep = plan_struct(m, good, {"nlevels": 0})
    assert call(s) == INVALID
    s, keep = plan_struct(m, u.pack_u32_plan([([], [], []), ([], [], [[]])]))   # empty levels, an empty chain: nothing to do
    assert call(s) == 0 and call(s, mem=m.MEM_DEVICE) == 0
    s, keep = plan_struct(m, good, {"nu32": 0, "nrec": 0, "npos": 0})
    assert call(s) == 0
    assert (dm.read() == start).all()
    s, keep = plan_struct(m, good)
    assert call(s) == 0 and (dm.read() == u.plan_u32_model(start, good)).all()
    dm.free()


@pytest.mark.gpu
def test_rows_satisfy_their_gates_under_check_witness(gpu_ctx):
    """a circuit of 2^7 rows from u32_gates.reference_gateset with gate_of_row taken from the plan and no bindings: the rows the
    device fills have no gate violation; after one output cell is overwritten they have"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import gl_np as gl
    u = ug()
    n = 128
    plan = random_plan(seed=11, n=n - 4, counts=[60, 200, 140])
    gs = u.reference_gateset()
    params = m.standard_params(7, gs.num_selectors + 2)
    gate_of_row = np.zeros(n, dtype=np.int64)
    used = np.nonzero(plan.row_kind >= 0)[0]
    gate_of_row[used] = [gs.index(u.U32_JOB_KINDS[int(k)][0]) for k in plan.row_kind[used]]
    circ = m.circuit.Circuit(params, gs, np.zeros((params.num_constants + params.num_routed_wires, n), dtype=np.uint64),
                             gl.powers(7, params.num_routed_wires), 0)
    rows = m.circuit.Rows(gate_of_row, gs.index("NoopGate"), None, m.circuit.bindings_of([]), 0)
    data = m.CircuitData.build_from_rows(gpu_ctx, circ, rows)
    zero = np.zeros((params.num_wires, n), dtype=np.uint64)
    dm = DeviceMatrix(gpu_ctx, zero)
    ends = (plan.u32_level_ends, plan.rec_level_ends, plan.pos_level_ends)
    gpu_ctx.witness_plan_rows_u32(*[getattr(plan, name) for name in LISTS], *ends, dm.ptr, params.num_wires, n)
    none = np.zeros(0, dtype=np.uint64)
    report = data.check_witness(dm.ptr, none, mem=m.MEM_DEVICE)
    assert report.gate_violations == 0 and report.noncanonical_cells == 0, report
    filled = dm.read()
    assert (filled[:, :n - 4] == u.plan_u32_model(zero[:, :n - 4], plan)).all()
    job = plan.u32_jobs[plan.u32_jobs["kind"].tolist().index(SUB)]
    col = (6 * int(job["op"]) + 4) if int(job["kind"]) == ADD else (5 * int(job["op"]) + 3)
    filled[col, int(job["row"])] = (int(filled[col, int(job["row"])]) + 1) % (1 << 32)
    gpu_ctx.buffer_write(dm.ptr, filled)
    report = data.check_witness(dm.ptr, none, mem=m.MEM_DEVICE)
    assert report.gate_violations > 0 and report.gate_row == int(job["row"]), report
    dm.free()
    data.close()
