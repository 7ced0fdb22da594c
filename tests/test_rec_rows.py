"""lcp2_rec_gate_rows: the rows of the ten recursion gates (ArithmeticGate, BaseSumGate, ArithmeticExtensionGate, MulExtensionGate,
ReducingGate, ReducingExtensionGate, PoseidonMdsGate, RandomAccessGate, ExponentiationGate, CosetInterpolationGate) generated on the
device from a recorded plan: jobs whose operands are immediates or cells of the witness matrix, run level by level.

Without a GPU: csrc/rec_rows.hpp - the per-job function the kernel runs and the validation (tests/emu/emu_rec.cpp), and one
level's launch as a loop over lanes (tests/emu/emu_plan.cpp: the launch of a plan without chains) - compiled for the CPU against
the integer generators row_*, against Python integers (recursion_gates.job_cells) and against the gates' own constraint programs
(gate_program_ref), a chained plan level by level, and the argument checks of the entry point.  On the GPU: the same through the library, and a proof from a device-filled matrix
against the host matrix' and the oracle's."""
import ctypes

import numpy as np
import pytest

import rows_lib
from rows_lib import INVALID, MAX, NONE, NW, P, DeviceMatrix, build_emu, check_null_context, gate_constraints, upload, vp

ARITH, BSUM, AEXT, MEXT, RED, REDX, PMDS, RA, EXP, COSET = range(10)
OPS = {ARITH: 20, BSUM: 1, AEXT: 10, MEXT: 13, RED: 1, REDX: 1, PMDS: 1, RA: 5, EXP: 1, COSET: 1}
COUNT = {ARITH: 5, BSUM: 1, AEXT: 8, MEXT: 5, RED: 47, REDX: 68, PMDS: 24, RA: 17, EXP: 3, COSET: 35}   # (RA op 4: 2)


def rg():
    from eth_lc_plonky2_amd import recursion_gates
    return recursion_gates


@pytest.fixture(scope="module")
def emur():
    """tests/emu/libemu_rec.so"""
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_rec", (("emu_rec_job_bytes", c.c_uint, []), ("emu_rec_operand_bytes", c.c_uint, []), ("emu_rec_row_columns", c.c_uint, []),
                            ("emu_rec_kind_ops", c.c_uint, [c.c_uint]), ("emu_rec_kind_operands", c.c_uint, [c.c_uint, c.c_uint]),
                            ("emu_rec_coset_domain", U, [c.c_uint]), ("emu_rec_coset_weight", U, [c.c_uint]),
                            ("emu_rec_job_problem", c.c_uint, [V, V, U, c.c_uint, U]), ("emu_rec_value_problem", c.c_uint, [V, V]),
                            ("emu_rec_job_cells", c.c_uint, [V, V, V, V, c.c_uint])))


@pytest.fixture(scope="module")
def emul():
    """tests/emu/libemu_plan.so: a level's launch"""
    return rows_lib.emu_plan()


def imm_job(kind, op, vals, row=0):
    """(jobs, operands) of one job whose operands are all immediates"""
    g = rg()
    jobs, ops, _ = g.pack_plan([[(row, kind, op, [g.IMM(v) for v in vals])]])
    return jobs, ops


def emu_cells(E, kind, op, vals):
    """{column: value} of one IMM job through the emulation; every column at most once"""
    jobs, ops = imm_job(kind, op, vals)
    assert E.emu_rec_job_problem(vp(jobs), vp(ops), ops.size, NW, 1) == 0 and E.emu_rec_value_problem(vp(jobs), vp(ops)) == 0
    cols, vals_out = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.uint64)
    k = E.emu_rec_job_cells(vp(jobs), vp(ops), vp(cols), vp(vals_out), 256)
    assert k <= 256 and len(set(cols[:k].tolist())) == k
    return {int(c): int(v) for c, v in zip(cols[:k], vals_out[:k])}


def emu_run(E, jobs, ops, ends, n, threads, start=None, order=None):
    """the plan through the emulated launches, one per level, as the witness plan without chains it is: (matrix, flag), the flag
    as the entry point decodes it: NONE, or job << 8 | reason"""
    plan = rows_lib.rec_plan(jobs, ops, ends)
    got, flags = rows_lib.run_levels(E, plan, n, start, order, threads)
    named = rows_lib.refusal(E, flags, plan)
    assert flags[1] == NONE and (named is None or named[0] == "rec")
    return got, NONE if named is None else named[1] << 8 | named[2]


# ------------------------------------------------------------------ the edge jobs (tests 3 and 7)
def output_column(kind, op):
    """a cell the job writes that its gate's constraints pin whatever the constants are"""
    return {ARITH: 4 * op + 3, BSUM: 0, AEXT: 8 * op + 6, MEXT: 6 * op + 4, RED: 0, REDX: 0, PMDS: 24, RA: 72 if op == 4 else 18 * op + 1,
            EXP: 67, COSET: 35}[kind]


def limited(kind, vals, value):
    """vals with the operand that can make the job refusable (BASE_SUM value < 2^63, RANDOM_ACCESS index < 16, EXPONENTIATION high
    word <= 3, COSET_INTERPOLATION shift != 0) set to `value`"""
    at = {BSUM: 0, RA: 0, EXP: 2, COSET: 0}.get(kind)
    out = list(vals)
    if at is not None and value is not None:
        out[at] = value
    return out


def edge_jobs():
    """[(kind, operand values, {column offset from the output column's base: named value} or a check name)].  'Every operand p - 1'
    and the non-canonical operands keep the job VALID: the four value-limited operands take their own largest value (2^63 - 1, 15, 3)
    or a non-canonical spelling of an allowed one (p + 15, p + 3, p + 1) instead."""
    rng = np.random.default_rng(77)

    def f():
        return int(rng.integers(0, P, dtype=np.uint64))

    top = {BSUM: (1 << 63) - 1, RA: 15, EXP: 3, COSET: P - 1}
    spelled = {BSUM: P, RA: P + 15, EXP: P + 3, COSET: P + 1}
    spelled_max = {BSUM: MAX, RA: P + 15, EXP: P + 3, COSET: MAX}
    jobs = []
    for kind in range(10):
        jobs.append((kind, limited(kind, [P - 1] * COUNT[kind], top.get(kind)), "p-1"))
        jobs.append((kind, limited(kind, [P] * COUNT[kind], spelled.get(kind)), "p"))
        jobs.append((kind, limited(kind, [MAX] * COUNT[kind], spelled_max.get(kind)), "max"))
    for kind in (ARITH, AEXT):
        jobs.append((kind, [0, f()] + [f() for _ in range(COUNT[kind] - 2)], "c0=0"))
        jobs.append((kind, [f(), 0] + [f() for _ in range(COUNT[kind] - 2)], "c1=0"))
    for kind in (RED, REDX):
        jobs.append((kind, [0, 0] + [f() for _ in range(COUNT[kind] - 2)], "alpha=0"))
    b = f()
    jobs += [(EXP, [b, 0, 0], "power0"), (EXP, [0, 0, 0], "power0"), (EXP, [0, 1, 0], "zero^1"), (EXP, [b, MAX, 3], "power-max"),
             (EXP, [P - 1, f(), 2], "base-1")]
    jobs += [(RA, [0] + [f() for _ in range(16)], "index0"), (RA, [15] + [f() for _ in range(16)], "index15")]
    jobs += [(BSUM, [0], "zero"), (BSUM, [(1 << 63) - 1], "top")]
    shift = f() or 1
    values = [f() for _ in range(32)]
    from eth_lc_plonky2_amd import u32_gates as ug
    jobs.append((COSET, [shift] + values + [shift * ug._coset_domain()[5] % P, 0], "on-coset"))
    jobs.append((COSET, [1] + values + [f(), f()], "shift1"))
    return jobs


def edge_items():
    """every edge job in every operation slot of its gate: (kind, op, operand values, tag).  RANDOM_ACCESS op 4 takes two constants"""
    items = []
    for kind, vals, tag in edge_jobs():
        for op in range(OPS[kind]):
            items.append((kind, op, vals[:2] if kind == RA and op == 4 else vals, tag))
    return items


def check_named(kind, op, vals, tag, cells):
    """the values the issue names"""
    v = [x % P for x in vals]
    assert all(x < P for x in cells.values()), "a written value is not canonical"
    if tag == "alpha=0":
        count, ext = (32, True) if kind == REDX else (43, False)
        start = 6 + (2 if ext else 1) * count
        for i in range(count):
            coeff = (v[4 + 2 * i], v[5 + 2 * i]) if ext else (v[4 + i], 0)
            at = start + 2 * i if i < count - 1 else 0
            assert (cells[at], cells[at + 1]) == coeff
    elif tag == "power0":
        assert cells[67] == 1
    elif tag == "zero^1":
        assert cells[67] == 0
    elif tag == "power-max":
        assert cells[67] == pow(v[0], (1 << 66) - 1, P) and all(cells[1 + i] == 1 for i in range(66))
    elif tag == "base-1":
        assert cells[67] == pow(P - 1, vals[1] | (2 << 64), P)
    elif tag in ("index0", "index15") and op < 4:
        assert cells[18 * op + 1] == v[1 + v[0]]
    elif tag == "top":
        assert all(cells[1 + i] == 1 for i in range(63))
    elif tag == "on-coset":
        assert (cells[35], cells[36]) == (v[1 + 2 * 5], v[2 + 2 * 5])
    elif tag in ("c0=0", "c1=0") and kind == ARITH:
        assert cells[4 * op + 3] == (v[0] * v[2] * v[3] + v[1] * v[4]) % P


GATE_CONSTS = {ARITH: lambda op, v: (v[0], v[1]), AEXT: lambda op, v: (v[0], v[1]), MEXT: lambda op, v: (v[0], 0),
               RA: lambda op, v: (v[0], v[1]) if op == 4 else (0, 0)}


# ------------------------------------------------------------------ without a GPU
def test_layout_tables_and_columns(emur):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import u32_gates as ug
    g, b = rg(), m.binding
    assert emur.emu_rec_job_bytes() == 16 == ctypes.sizeof(b.RecJob) == b.REC_JOB_DTYPE.itemsize
    assert emur.emu_rec_operand_bytes() == 16 == ctypes.sizeof(b.RecOperand) == b.REC_OPERAND_DTYPE.itemsize
    assert sorted(g.REC_JOB_KINDS) == list(range(10)) and emur.emu_rec_kind_ops(10) == 0
    top = 0
    for kind, (name, ops, count) in g.REC_JOB_KINDS.items():
        assert emur.emu_rec_kind_ops(kind) == ops == OPS[kind]
        owned = [g.job_columns(kind, op) for op in range(ops)]
        flat = [c for cols in owned for c in cols]
        assert len(set(flat)) == len(flat), "two operations of a row share a column"
        top = max(top, max(flat))
        for op in range(ops):
            assert emur.emu_rec_kind_operands(kind, op) == count(op) == (2 if kind == RA and op == 4 else COUNT[kind])
    assert top < 135 == emur.emu_rec_row_columns() == g.REC_ROW_COLUMNS
    domain = ug._coset_domain()
    assert [emur.emu_rec_coset_domain(i) for i in range(16)] == domain
    assert [emur.emu_rec_coset_weight(i) for i in range(16)] == ug._barycentric_weights(domain)


def random_rows(kind, n, rng):
    """(wires [135][n], c0 [n], c1 [n]): n rows of one gate from the integer generators (numpy for Arithmetic and BaseSum)"""
    from eth_lc_plonky2_amd import gl_np as gl
    from eth_lc_plonky2_amd import u32_gates as ug
    g = rg()
    c0, c1 = rng.integers(0, P, size=n, dtype=np.uint64), rng.integers(0, P, size=n, dtype=np.uint64)
    wires = rng.integers(0, P, size=(NW, n), dtype=np.uint64)
    if kind == ARITH:
        for k in range(20):
            wires[4 * k + 3] = gl.add(gl.mul(gl.mul(wires[4 * k], wires[4 * k + 1]), c0), gl.mul(wires[4 * k + 2], c1))
    elif kind == BSUM:
        wires[0] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
        for i in range(63):
            wires[1 + i] = (wires[0] >> np.uint64(i)) & np.uint64(1)
    else:
        gen = {AEXT: lambda r: g.row_arithmetic_extension(rng, int(c0[r]), int(c1[r])), MEXT: lambda r: g.row_mul_extension(rng, int(c0[r])),
               RED: lambda r: g.row_reducing(rng), REDX: lambda r: g.row_reducing_extension(rng), PMDS: lambda r: g.row_poseidon_mds(rng),
               RA: lambda r: g.row_random_access(rng, int(c0[r]), int(c1[r])), EXP: lambda r: g.row_exponentiation(rng),
               COSET: lambda r: ug.row_coset_interpolation(rng)}[kind]
        for r in range(n):
            wires[:, r] = np.array(gen(r), dtype=np.uint64)
    return wires, c0, c1


def test_random_jobs_equal_the_generators_cell_for_cell(emur):
    """per kind 64 rows of the gate's generator: witness_jobs recovers IMM jobs, one per operation; the cells each job writes
    through the emulated per-job function are exactly its job_columns and equal the generator's"""
    g = rg()
    rng = np.random.default_rng(64)
    for kind, (name, ops, count) in g.REC_JOB_KINDS.items():
        n = 64
        wires, c0, c1 = random_rows(kind, n, rng)
        jobs, operands, ends = g.witness_jobs(wires, np.zeros(n, dtype=np.int64), {name: 0}, (c0, c1))
        assert jobs.size == n * ops == ends[-1] and (operands["src"] == 0).all()
        cols, vals = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.uint64)
        for i in range(jobs.size):
            job = jobs[i:i + 1]
            row, op = int(job["row"][0]), int(job["op"][0])
            assert emur.emu_rec_job_problem(vp(job), vp(operands), operands.size, NW, n) == 0
            assert emur.emu_rec_value_problem(vp(job), vp(operands)) == 0
            k = emur.emu_rec_job_cells(vp(job), vp(operands), vp(cols), vp(vals), 256)
            assert sorted(cols[:k].tolist()) == sorted(g.job_columns(kind, op)), (name, op)
            assert (vals[:k] == wires[cols[:k], row]).all(), (name, row, op)


def test_edge_jobs_equal_python_integers_and_satisfy_their_gates(emur):
    """every edge job in every slot: the emulated cells equal recursion_gates.job_cells (Python integers) and the values the issue
    names, are canonical, make every constraint of the gate's own program zero on a row whose other cells are zero, and one
    changed output cell makes a constraint non-zero"""
    g = rg()
    gs = g.chain_gateset(native=False)
    for kind, op, vals, tag in edge_items():
        name = g.REC_JOB_KINDS[kind][0]
        cells = emu_cells(emur, kind, op, vals)
        assert cells == g.job_cells(kind, op, vals), (name, op, tag)
        assert sorted(cells) == sorted(g.job_columns(kind, op))
        check_named(kind, op, vals, tag, cells)
        consts = [c % P for c in GATE_CONSTS.get(kind, lambda op, v: (0, 0))(op, vals)]
        row = [0] * NW
        for col, v in cells.items():
            row[col] = v
        bad = [i for i, c in enumerate(gate_constraints(gs, name, row, consts)) if c]
        assert not bad, (name, op, tag, bad)
        row[output_column(kind, op)] = (row[output_column(kind, op)] + 1) % P
        assert any(gate_constraints(gs, name, row, consts)), (name, op, tag)


def test_chain_plan_level_by_level(emul):
    """chain_plan(64, seed) through the emulated launches from a zero matrix, at 64 and 256 lanes per block: the expected matrix,
    nothing outside the owned cells; the levels in reverse order do NOT give it (a level reads what the level before wrote)"""
    g = rg()
    plan = g.chain_plan(64, seed=4)
    assert len(plan.level_ends) >= 6 and (plan.operands["src"][plan.jobs[plan.level_ends[0]]["first_operand"]:] == 1).any()
    assert set(plan.jobs["kind"][:plan.level_ends[0]].tolist()) == set(range(10))
    assert (plan.operands["src"][:plan.jobs[plan.level_ends[0]]["first_operand"]] == 0).all(), "level 0 is IMM only"
    owned = np.zeros((NW, 64), dtype=bool)
    for j in plan.jobs:
        owned[g.job_columns(int(j["kind"]), int(j["op"])), int(j["row"])] = True
    assert not plan.expected[~owned].any() and (plan.expected < np.uint64(P)).all()
    for threads in (64, 256):
        got, flag = emu_run(emul, plan.jobs, plan.operands, plan.level_ends, 64, threads)
        assert flag == NONE
        assert (got == plan.expected).all()
    got, _ = emu_run(emul, plan.jobs, plan.operands, plan.level_ends, 64, 64, order=list(reversed(range(len(plan.level_ends)))))
    assert not (got == plan.expected).all()
    other = g.chain_plan(64, seed=5)
    assert (other.jobs == plan.jobs).all() and (other.operands[other.operands["src"] == 1] == plan.operands[plan.operands["src"] == 1]).all()
    assert not (other.expected == plan.expected).all()


def test_pack_plan_is_the_witness_plan_without_chains():
    """pack_plan(levels) and pack_witness_plan with empty chain lists give the same rec jobs, operands and level ends byte for
    byte, and no PoseidonGate job, chain or chain level: three levels of 30 ARITHMETIC jobs, and one job of every kind"""
    g = rg()
    good = arithmetic_jobs(90, 64, np.random.default_rng(12))
    every_kind = {kind: (row, kind, 0, [g.IMM(v) for v in vals]) for row, (kind, vals, _) in reversed(list(enumerate(edge_jobs())))}
    assert sorted(every_kind) == list(range(10))
    for levels in ([good[:30], good[30:60], good[60:]], [list(every_kind.values())]):
        jobs, ops, ends = g.pack_plan(levels)
        plan = g.pack_witness_plan([(level, []) for level in levels])
        assert jobs.size == sum(len(level) for level in levels) == ends[-1] and ops.size == sum(len(it[3]) for level in levels for it in level)
        assert (jobs.tobytes(), ops.tobytes(), ends.tobytes()) == (plan.rec_jobs.tobytes(), plan.operands.tobytes(), plan.rec_level_ends.tobytes())
        assert (jobs.dtype, ops.dtype, ends.dtype) == (plan.rec_jobs.dtype, plan.operands.dtype, plan.rec_level_ends.dtype)
        assert plan.pos_jobs.size == 0 and plan.chain_ends.size == 0 and not plan.pos_level_ends.any()
        assert (g.run_plan(jobs, ops, ends, NW, 64) == g.run_witness_plan(plan, NW, 64)).all()


def structural_cases():
    """[(reason code, row, kind, op, operands, noperands override or None)] for a 64-row, 135-column matrix"""
    g = rg()
    ok = [g.IMM(1)] * 5
    return [(1, 64, ARITH, 0, ok, None), (2, 0, 10, 0, ok, None), (2, 0, 0xFFFF, 0, ok, None), (3, 0, ARITH, 20, ok, None),
            (3, 0, BSUM, 1, [g.IMM(1)], None), (3, 0, AEXT, 10, [g.IMM(1)] * 8, None), (3, 0, MEXT, 13, ok, None), (3, 0, RA, 5, [g.IMM(1)] * 2, None),
            (3, 0, COSET, 1, [g.IMM(1)] * 35, None), (4, 0, ARITH, 0, ok, 4), (5, 0, ARITH, 0, ok[:4] + [(1, 0, 2)], None),
            (6, 0, ARITH, 0, ok[:4] + [g.CELL(0, 135)], None), (7, 0, ARITH, 0, ok[:4] + [g.CELL(64, 0)], None)]


def raw_job(row, kind, op, operands):
    import eth_lc_plonky2_amd as m
    jobs = np.zeros(1, dtype=m.binding.REC_JOB_DTYPE)
    ops = np.zeros(len(operands), dtype=m.binding.REC_OPERAND_DTYPE)
    jobs[0] = (row, kind, op, 0, 0)
    for k, o in enumerate(operands):
        ops[k] = o
    return jobs, ops


VALUE_CASES = [(8, BSUM, [1 << 63], [(1 << 63) - 1]), (9, RA, [16] + [1] * 16, [15] + [1] * 16), (10, EXP, [2, 5, 4], [2, MAX, 3]),
               (11, COSET, [0] + [1] * 34, [1] * 35), (11, COSET, [P] + [1] * 34, [P + 1] + [1] * 34)]


def test_refused_jobs(emur, emul):
    """every structural reason and every value reason as IMM through the shared validation; the limits are accepted; as CELL the
    flag names the job, that job's cells stay untouched, the rest of its level is written and later levels are not run"""
    g = rg()
    for code, row, kind, op, operands, nops in structural_cases():
        jobs, ops = raw_job(row, kind, op, operands)
        assert emur.emu_rec_job_problem(vp(jobs), vp(ops), ops.size if nops is None else nops, NW, 64) == code, (code, kind, op)
    for row, kind, op, operands in ((63, ARITH, 19, [g.IMM(MAX)] * 4 + [g.CELL(63, 134)]), (0, RA, 4, [g.IMM(1)] * 2), (0, MEXT, 12, [g.IMM(1)] * 5)):
        jobs, ops = raw_job(row, kind, op, operands)
        assert emur.emu_rec_job_problem(vp(jobs), vp(ops), ops.size, NW, 64) == 0
    for code, kind, bad, good in VALUE_CASES:
        jobs, ops = imm_job(kind, 0, bad)
        assert emur.emu_rec_job_problem(vp(jobs), vp(ops), ops.size, NW, 64) == 0 and emur.emu_rec_value_problem(vp(jobs), vp(ops)) == code
        jobs, ops = imm_job(kind, 0, good)
        assert emur.emu_rec_value_problem(vp(jobs), vp(ops)) == 0
    for code, kind, bad, good in VALUE_CASES[:4]:
        jobs, ops, ends, bad_at = cell_refusal_plan(kind, bad)
        keep = np.ones(jobs.size, dtype=bool)
        keep[bad_at] = False
        want = g.run_plan(jobs[keep], ops, [ends[0], ends[1] - 1], NW, 64)   # the levels up to the refused job's, without it
        got, flag = emu_run(emul, jobs, ops, ends, 64, 64)
        assert flag == (bad_at << 8 | code)
        assert (got == want).all() and not got[:, 10].any() and not got[:, 20].any()


def cell_refusal_plan(kind, bad):
    """three levels: level 0 writes the refusable value into a cell (an ARITHMETIC op: 1 * v * 1 + 0) and more; level 1 holds a job
    of `kind` on row 10 that reads it as a CELL, between two valid ARITHMETIC jobs; level 2 holds one more valid job on row 20.
    Returns (jobs, operands, level_ends, the index of the refusable job)."""
    g = rg()
    at = {BSUM: 0, RA: 0, EXP: 2, COSET: 0}[kind]
    arith = lambda row, op, v: (row, ARITH, op, [g.IMM(1), g.IMM(0), g.IMM(v), g.IMM(1), g.IMM(0)])   # noqa: E731
    operands = [g.IMM(v) for v in bad]
    operands[at] = g.CELL(0, 3)
    levels = [[arith(0, 0, bad[at] % P), arith(1, 1, 7)], [arith(2, 0, 8), (10, kind, 0, operands), arith(3, 0, 9)], [arith(20, 0, 11)]]
    jobs, ops, ends = g.pack_plan(levels)
    bad_at = int(ends[0]) + [int(k) for k in jobs["kind"][ends[0]:ends[1]]].index(kind)
    return jobs, ops, ends, bad_at


def test_entry_point_checks_its_pointers_first():
    """without a device there is no context, and the null check comes first: LCP2_E_INVALID for a null context whatever the lists
    hold (a valid job, refused ones, nothing), for both lists_mem values, never a crash or another status"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    good_jobs, good_ops = imm_job(ARITH, 0, [1, 2, 3, 4, 5])
    bad_jobs, bad_ops = raw_job(64, 10, 99, [(1, 0, 2)])
    one, none = np.array([1], dtype=np.uint32), None
    check_null_context(lambda a, mem, w: lib.lcp2_rec_gate_rows(None, *a, mem, w, NW, 64),
                       [(vp(good_jobs), 1, vp(good_ops), 5, vp(one), 1), (vp(bad_jobs), 1, vp(bad_ops), 1, vp(one), 1), (none, 0, none, 0, none, 0)],
                       (m.MEM_HOST, m.MEM_DEVICE), null_wires=(none, 1, none, 0, none, 1))


# ------------------------------------------------------------------ on the GPU
def run_on_device(ctx, jobs, ops, ends, start, device_lists=False):
    n = start.shape[1]
    dm = DeviceMatrix(ctx, start)
    if device_lists:
        dj, do = upload(ctx, jobs), upload(ctx, ops)
        ctx.rec_gate_rows(dj, do, ends, dm.ptr, NW, n, njobs=jobs.size, noperands=ops.size)
        ctx.buffer_free(dj)
        ctx.buffer_free(do)
    else:
        ctx.rec_gate_rows(jobs, ops, ends, dm.ptr, NW, n)
    got = dm.read()
    dm.free()
    return got


@pytest.mark.gpu
def test_refill_of_256_rows(gpu_ctx):
    """256 rows, every kind at least 16 times: from the witness with its owned cells zeroed, one call with host lists, and again
    with the lists in HBM, restores every owned cell and changes no other"""
    g = rg()
    rng = np.random.default_rng(256)
    n = 256
    wires, c0, c1 = np.zeros((NW, n), dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    gate_of_row = np.arange(n) % 10
    G = {g.REC_JOB_KINDS[kind][0]: kind for kind in range(10)}
    owned = np.zeros((NW, n), dtype=bool)
    for kind in range(10):
        rows = np.nonzero(gate_of_row == kind)[0]
        assert rows.size >= 16
        wires[:, rows], c0[rows], c1[rows] = random_rows(kind, rows.size, rng)
        for op in range(OPS[kind]):
            owned[np.ix_(g.job_columns(kind, op), rows)] = True
    jobs, ops, ends = g.witness_jobs(wires, gate_of_row, G, (c0, c1))
    zeroed = np.where(owned, np.uint64(0), wires)
    assert not (zeroed == wires).all()
    for device_lists in (False, True):
        got = run_on_device(gpu_ctx, jobs, ops, ends, zeroed, device_lists)
        assert (got[owned] == wires[owned]).all(), "an owned cell differs from the host witness"
        assert (got[~owned] == wires[~owned]).all(), "a cell no job owns changed"


@pytest.mark.gpu
def test_edge_jobs_on_the_device(gpu_ctx):
    """the edge jobs of the CPU test, every slot: rows of 64 per call, each job on a row of its own; the matrix equals Python's"""
    g = rg()
    items = edge_items()
    n = 64
    for at in range(0, len(items), n):
        level = [(r, kind, op, [g.IMM(v) for v in vals]) for r, (kind, op, vals, _) in enumerate(items[at:at + n])]
        jobs, ops, ends = g.pack_plan([level])
        want = np.zeros((NW, n), dtype=np.uint64)
        for r, kind, op, operands in level:
            for col, v in g.job_cells(kind, op, [o[0] for o in operands]).items():
                want[col, r] = v
        got = run_on_device(gpu_ctx, jobs, ops, ends, np.zeros((NW, n), dtype=np.uint64))
        assert (got == want).all(), at


@pytest.mark.gpu
def test_chain_on_the_device(gpu_ctx):
    """chain_plan(256, seed) from a zero matrix with host lists and with resident lists; then only level 0's IMM values are
    rewritten in the resident operand buffer and the same plan is replayed: the second seed's expected matrix"""
    g = rg()
    n = 256
    plan, second = g.chain_plan(n, seed=8), g.chain_plan(n, seed=9)
    zero = np.zeros((NW, n), dtype=np.uint64)
    assert (run_on_device(gpu_ctx, plan.jobs, plan.operands, plan.level_ends, zero) == plan.expected).all()
    dj, do = upload(gpu_ctx, plan.jobs), upload(gpu_ctx, plan.operands)
    dm = DeviceMatrix(gpu_ctx, zero)
    gpu_ctx.rec_gate_rows(dj, do, plan.level_ends, dm.ptr, NW, n, njobs=plan.jobs.size, noperands=plan.operands.size)
    assert (dm.read() == plan.expected).all()
    leaves = int(plan.jobs[plan.level_ends[0]]["first_operand"])   # level 0's operands come first
    assert (second.jobs == plan.jobs).all() and (second.operands[leaves:] == plan.operands[leaves:]).all()
    assert not (second.expected == plan.expected).all()
    gpu_ctx.buffer_write(do, np.ascontiguousarray(second.operands[:leaves]).view(np.uint64))
    gpu_ctx.rec_gate_rows(dj, do, plan.level_ends, dm.ptr, NW, n, njobs=plan.jobs.size, noperands=plan.operands.size)
    assert (dm.read() == second.expected).all()
    dm.free()
    gpu_ctx.buffer_free(dj)
    gpu_ctx.buffer_free(do)


def arithmetic_jobs(count, n, rng):
    """`count` IMM ARITHMETIC jobs on distinct (row, op) slots of an n-row matrix, in a shuffled order: [(row, kind, op, operands)]"""
    g = rg()
    assert count <= 20 * n
    slots = rng.permutation(20 * n)[:count]
    return [(int(s) // 20, ARITH, int(s) % 20, [g.IMM(v) for v in rng.integers(1, P, size=5, dtype=np.uint64)]) for s in slots]


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_launch_boundaries(gpu_ctx, count):
    """single-level lists around the wave (64) and the block (256), in shuffled order (pack_plan would sort: the records are
    shuffled after packing): exact, and no cell outside the owned columns changes"""
    g = rg()
    rng = np.random.default_rng(count)
    jobs, ops, ends = g.pack_plan([arithmetic_jobs(count, 64, rng)])
    jobs = jobs[rng.permutation(count)]
    want = g.run_plan(jobs, ops, ends, NW, 64)
    assert want.any()
    assert (run_on_device(gpu_ctx, jobs, ops, ends, np.zeros((NW, 64), dtype=np.uint64)) == want).all()


@pytest.mark.gpu
def test_forty_levels(gpu_ctx):
    """40 levels of one job: ARITHMETIC op 0 of row l squares the output of row l - 1 (c0 = 1, c1 = 0)"""
    g = rg()
    x = 0x123456789ABCDEF0 % P
    levels = [[(lv, ARITH, 0, [g.IMM(1), g.IMM(0)] + ([g.IMM(x)] * 2 if lv == 0 else [g.CELL(lv - 1, 3)] * 2) + [g.IMM(0)])] for lv in range(40)]
    jobs, ops, ends = g.pack_plan(levels)
    assert list(ends) == list(range(1, 41))
    for device_lists in (False, True):
        got = run_on_device(gpu_ctx, jobs, ops, ends, np.zeros((NW, 64), dtype=np.uint64), device_lists)
        assert [int(v) for v in got[3, :40]] == [pow(x, 2 ** (lv + 1), P) for lv in range(40)]


@pytest.mark.gpu
def test_both_entry_points_run_one_plan(gpu_ctx):
    """64 rows, three levels of 30 ARITHMETIC jobs, level 1 reading a cell of level 0: lcp2_rec_gate_rows and lcp2_witness_plan_rows
    with npos = nchains = 0 and pos_level_ends = NULL, from host lists and from device lists, leave run_plan's matrix.  Then one job
    of level 1 becomes a RANDOM_ACCESS job whose index is a CELL holding 16, which only the device can see: both entry points
    return LCP2_E_INVALID, name the same job, and leave levels 0 and 1 without that job written and nothing of level 2"""
    import re
    import eth_lc_plonky2_amd as m
    g = rg()
    lib, h, n = gpu_ctx.lib, gpu_ctx.handle, 64
    good = arithmetic_jobs(90, n, np.random.default_rng(12))
    levels = [list(good[:30]), list(good[30:60]), list(good[60:])]
    src_row, _, src_op, _ = levels[0][0]
    row, kind, op, operands = levels[1][0]
    levels[1][0] = (row, kind, op, operands[:2] + [g.CELL(src_row, 4 * src_op + 3)] + operands[3:])
    zero = np.zeros((NW, n), dtype=np.uint64)

    def both(jobs, ops, ends, device_lists):
        """[(status, last error, matrix)] of lcp2_rec_gate_rows and of lcp2_witness_plan_rows"""
        out = []
        dj, do = (upload(gpu_ctx, jobs), upload(gpu_ctx, ops)) if device_lists else (jobs.ctypes.data, ops.ctypes.data)
        mem = m.MEM_DEVICE if device_lists else m.MEM_HOST
        plan = m.binding.WitnessPlan(dj, jobs.size, ends.ctypes.data, None, 0, None, 0, None, do, ops.size, ends.size)
        for by_plan in (False, True):
            dm = DeviceMatrix(gpu_ctx, zero)
            wp = ctypes.c_void_p(dm.ptr)
            status = (lib.lcp2_witness_plan_rows(h, ctypes.byref(plan), mem, wp, NW, n) if by_plan else
                      lib.lcp2_rec_gate_rows(h, ctypes.c_void_p(dj), jobs.size, ctypes.c_void_p(do), ops.size, vp(ends), ends.size, mem, wp, NW, n))
            out.append((status, lib.lcp2_last_error(h) if status else b"", dm.read()))
            dm.free()
        if device_lists:
            gpu_ctx.buffer_free(dj)
            gpu_ctx.buffer_free(do)
        return out

    jobs, ops, ends = g.pack_plan(levels)
    want = g.run_plan(jobs, ops, ends, NW, n)
    assert list(ends) == [30, 60, 90] and (ops["src"] == 1).sum() == 1 and not (want == g.run_plan(jobs, ops, ends[:1], NW, n)).all()
    for device_lists in (False, True):
        for status, _, got in both(jobs, ops, ends, device_lists):
            assert status == 0 and (got == want).all(), device_lists
    # level 0's first job writes 16 (1 * 16 * 1 + 0), and a job of level 1 reads it as its RANDOM_ACCESS index
    levels[0][0] = (src_row, ARITH, src_op, [g.IMM(1), g.IMM(0), g.IMM(16), g.IMM(1), g.IMM(0)])
    levels[1][1] = (levels[1][1][0], RA, 0, [g.CELL(src_row, 4 * src_op + 3)] + [g.IMM(k) for k in range(16)])
    jobs, ops, ends = g.pack_plan(levels)
    bad_at = 59   # pack_plan sorts a level by kind: the RANDOM_ACCESS job is the last of level 1
    assert list(ends) == [30, 60, 90] and int(jobs["kind"][bad_at]) == RA
    keep = np.ones(jobs.size, dtype=bool)
    keep[bad_at] = False
    want = g.run_plan(jobs[keep], ops, [30, 59], NW, n)
    assert not (want == g.run_plan(jobs[keep], ops, [30], NW, n)).all() and not (want == g.run_plan(jobs[keep], ops, [30, 59, 89], NW, n)).all()
    for device_lists in (False, True):
        (rec_status, rec_error, rec_got), (plan_status, plan_error, plan_got) = both(jobs, ops, ends, device_lists)
        assert rec_status == INVALID == plan_status
        assert b"rec rows: job 59: random-access index" in rec_error and b"plan rows: rec job 59: random-access index" in plan_error
        assert re.search(rb"job (\d+):", rec_error).group(1) == re.search(rb"job (\d+):", plan_error).group(1) == b"%d" % bad_at
        assert (rec_got == want).all() and (plan_got == want).all(), device_lists


@pytest.mark.gpu
def test_long_host_list(gpu_ctx):
    """a host list of 2^18 + 5 jobs: the pinned staging buffer holds 2^18 records, so the upload of the whole list takes it twice;
    that boundary lies inside level 0 (level_ends = [count - 3, count]) and is an upload boundary only - the list is whole in HBM
    before the first launch, and a level is one launch.  Built as test_long_host_lists builds its list: 1280 jobs
    fill a 64-row matrix; the list repeats the first 1275 (equal jobs for one slot leave that value; they share their operands)
    and ends with the other 5, whose slots nothing earlier writes.  The 3 jobs of level 1 read a cell level 0 wrote."""
    g = rg()
    count = (4 << 20) // 16 + 5
    rng = np.random.default_rng(18)
    items = arithmetic_jobs(1280, 64, rng)
    source = items[0]
    for k in (1277, 1278, 1279):   # level 1: the multiplicand is the output of the list's first job
        row, kind, op, operands = items[k]
        items[k] = (row, kind, op, operands[:2] + [g.CELL(source[0], 4 * source[2] + 3)] + operands[3:])
    base, ops, _ = g.pack_plan([items[:1277], items[1277:]])
    jobs = np.concatenate([np.resize(base[:1275], count - 5), base[1275:]])
    ends = np.array([count - 3, count], dtype=np.uint32)
    assert jobs.size == count and jobs.nbytes > 4 << 20
    want = g.run_plan(base, ops, [1277, 1280], NW, 64)
    assert (run_on_device(gpu_ctx, jobs, ops, ends, np.zeros((NW, 64), dtype=np.uint64)) == want).all()


@pytest.mark.gpu
def test_refusals_on_the_device(gpu_ctx):
    """each bad job at position 0, in the middle and at the end of a good three-level list: a host list writes nothing; a device
    list writes the valid jobs of the levels up to and including the failing one and nothing later; lcp2_last_error names the job;
    then the argument checks of the entry point, and the context still works"""
    import eth_lc_plonky2_amd as m
    g = rg()
    lib, n = gpu_ctx.lib, 64
    rng = np.random.default_rng(12)
    good = arithmetic_jobs(90, n, rng)
    bad_items = [(row, kind, op, operands) for _, row, kind, op, operands, nops in structural_cases() if nops is None]
    bad_items += [(0, kind, 0, [g.IMM(v) for v in bad]) for _, kind, bad, _ in VALUE_CASES]
    zero = np.zeros((NW, n), dtype=np.uint64)
    for k, item in enumerate(bad_items):
        position = (0, 45, 90)[k % 3]
        level_of, levels = (0, 1, 2)[k % 3], [list(good[:30]), list(good[30:60]), list(good[60:])]
        # pack_plan sorts a level by (kind, op, row): pack the good list, then splice the bad record in at `position`
        jobs, ops, ends = g.pack_plan(levels)
        bj, bo = raw_job(item[0], item[1], item[2], item[3])
        bj["first_operand"] = ops.size
        mixed = np.concatenate([jobs[:position], bj, jobs[position:]])
        mixed_ops = np.concatenate([ops, bo])
        mixed_ends = np.array([e + (1 if l >= level_of else 0) for l, e in enumerate(ends)], dtype=np.uint32)
        want = g.run_plan(jobs, ops, ends[:level_of + 1], NW, n)
        args = (mixed.size, vp(mixed_ops), mixed_ops.size, vp(mixed_ends), 3)
        dm = DeviceMatrix(gpu_ctx, zero)
        assert lib.lcp2_rec_gate_rows(gpu_ctx.handle, vp(mixed), *args, m.MEM_HOST, ctypes.c_void_p(dm.ptr), NW, n) == INVALID
        reason = lib.lcp2_last_error(gpu_ctx.handle)
        assert b"job %d:" % position in reason, reason
        assert not dm.read().any(), "a refused host list wrote something"
        with pytest.raises(m.Lcp2Error) as e:
            gpu_ctx.rec_gate_rows(mixed, mixed_ops, mixed_ends, dm.ptr, NW, n)
        assert e.value.status == INVALID
        dj, do = upload(gpu_ctx, mixed), upload(gpu_ctx, mixed_ops)
        assert lib.lcp2_rec_gate_rows(gpu_ctx.handle, ctypes.c_void_p(dj), mixed.size, ctypes.c_void_p(do), mixed_ops.size, vp(mixed_ends), 3,
                                      m.MEM_DEVICE, ctypes.c_void_p(dm.ptr), NW, n) == INVALID
        assert b"job %d:" % position in lib.lcp2_last_error(gpu_ctx.handle)
        assert (dm.read() == want).all(), (k, item[:3])
        gpu_ctx.buffer_free(dj)
        gpu_ctx.buffer_free(do)
        dm.free()
    # a value seen only on the device (a CELL operand), from host lists and from device lists
    for code, kind, bad, _ in VALUE_CASES[:4]:
        jobs, ops, ends, bad_at = cell_refusal_plan(kind, bad)
        keep = np.ones(jobs.size, dtype=bool)
        keep[bad_at] = False
        want = g.run_plan(jobs[keep], ops, [ends[0], ends[1] - 1], NW, n)
        for device_lists in (False, True):
            with pytest.raises(m.Lcp2Error) as e:
                run_on_device_keep(gpu_ctx, jobs, ops, ends, zero, device_lists)
            assert e.value.status == INVALID and "job %d:" % bad_at in str(e.value)
            assert (run_on_device_keep.last == want).all()
    jobs, ops, ends = g.pack_plan([good])
    want = g.run_plan(jobs, ops, ends, NW, n)
    dm = DeviceMatrix(gpu_ctx, zero)
    wp, h = ctypes.c_void_p(dm.ptr), gpu_ctx.handle
    two = np.array([45, 90], dtype=np.uint32)
    for mem in (m.MEM_HOST, m.MEM_DEVICE):
        assert lib.lcp2_rec_gate_rows(h, vp(jobs), 0, vp(ops), ops.size, vp(ends), 1, mem, wp, NW, n) == 0
        assert lib.lcp2_rec_gate_rows(h, None, 0, None, 0, None, 0, mem, wp, NW, n) == 0
        assert lib.lcp2_rec_gate_rows(h, None, 1, vp(ops), ops.size, vp(ends), 1, mem, wp, NW, n) == INVALID
        assert lib.lcp2_rec_gate_rows(h, vp(jobs), 1, None, 5, vp(ends), 1, mem, wp, NW, n) == INVALID
        assert lib.lcp2_rec_gate_rows(h, vp(jobs), 1, vp(ops), ops.size, None, 1, mem, wp, NW, n) == INVALID
        assert lib.lcp2_rec_gate_rows(h, vp(jobs), 1, vp(ops), ops.size, vp(ends), 1, mem, None, NW, n) == INVALID
        assert lib.lcp2_rec_gate_rows(None, vp(jobs), 1, vp(ops), ops.size, vp(ends), 1, mem, wp, NW, n) == INVALID
    for bad_ends in ([90, 45], [45, 89], [45, 91], [91, 90]):   # not ascending, not ending at njobs, past the end
        assert lib.lcp2_rec_gate_rows(h, vp(jobs), 90, vp(ops), ops.size, vp(np.array(bad_ends, dtype=np.uint32)), 2, m.MEM_HOST, wp, NW, n) == INVALID
        assert b"level_ends" in lib.lcp2_last_error(h)
    assert lib.lcp2_rec_gate_rows(h, vp(jobs), 90, vp(ops), ops.size, vp(two), 2, m.MEM_HOST, wp, 134, n) == INVALID
    assert lib.lcp2_rec_gate_rows(h, vp(jobs), 90, vp(ops), ops.size, vp(two), 2, 2, wp, NW, n) == INVALID
    assert not dm.read().any()
    gpu_ctx.rec_gate_rows(jobs, ops, two, dm.ptr, NW, n)   # the context still works after the refusals
    assert (dm.read() == want).all()
    dm.free()


def run_on_device_keep(ctx, jobs, ops, ends, start, device_lists):
    """run_on_device for a call that raises: the matrix after the call is left in run_on_device_keep.last"""
    n = start.shape[1]
    dm = DeviceMatrix(ctx, start)
    dj, do = (upload(ctx, jobs), upload(ctx, ops)) if device_lists else (None, None)
    try:
        if device_lists:
            ctx.rec_gate_rows(dj, do, ends, dm.ptr, NW, n, njobs=jobs.size, noperands=ops.size)
        else:
            ctx.rec_gate_rows(jobs, ops, ends, dm.ptr, NW, n)
    finally:
        run_on_device_keep.last = dm.read()
        dm.free()
        if device_lists:
            ctx.buffer_free(dj)
            ctx.buffer_free(do)


@pytest.mark.gpu
def test_proof_from_a_device_filled_matrix(gpu_ctx, oracle):
    """2^10 rows of chain_plan filled on the device from a zero matrix (resident lists).  The zero matrix itself is refused with
    LCP2_E_UNSAT: a zero ExponentiationGate row does not satisfy its gate (its first intermediate must be 1) and a zero
    RandomAccessGate row does not either where the row's constants are non-zero - the plan holds both on every level, so the
    assertion holds for every seed.  The proof from the filled matrix (LCP2_MEM_DEVICE) equals the proof from the Python-computed
    host matrix and the oracle's proof of it, word for word, and verifies."""
    import eth_lc_plonky2_amd as m
    import oracle_lib
    g = rg()
    params = m.standard_params(10, 5)
    plan = g.chain_plan(1 << 10, seed=13)
    circ, pis = g.chain_circuit(params, plan)
    host = np.zeros((params.num_wires, circ.n), dtype=np.uint64)
    host[:NW] = plan.expected
    oc = oracle_lib.OracleCircuit(oracle, circ)
    assert oc.check_witness(host, pis)[0] == 0
    want = oc.prove(host, pis)
    oc.close()
    data = m.CircuitData.build(gpu_ctx, circ)
    from_host = data.prove(host, pis)
    dm = DeviceMatrix(gpu_ctx, np.zeros_like(host))
    with pytest.raises(m.Lcp2Error) as e:
        data.prove(dm.ptr, pis, mem=m.MEM_DEVICE)
    assert e.value.status == m.binding.E_UNSAT
    dj, do = upload(gpu_ctx, plan.jobs), upload(gpu_ctx, plan.operands)
    gpu_ctx.rec_gate_rows(dj, do, plan.level_ends, dm.ptr, params.num_wires, circ.n, njobs=plan.jobs.size, noperands=plan.operands.size)
    got = data.prove(dm.ptr, pis, mem=m.MEM_DEVICE)
    dm.free()
    gpu_ctx.buffer_free(dj)
    gpu_ctx.buffer_free(do)
    assert (got == from_host).all(), "the proof from the device-filled matrix differs from the host matrix' proof"
    assert (got == want).all(), "the proof differs from the oracle's"
    data.verify(got, pis)
    data.close()
