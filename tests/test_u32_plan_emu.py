"""lcp2_witness_plan_rows_u32 without a GPU: csrc/u32_plan.hpp - the validation, the lane text of k_u32_plan_rows and one level's three
launches with the three flag words - compiled for the CPU (tests/emu/emu_plan_u32.cpp) against u32_gates.plan_u32_model cell for
cell, against the gates' own constraint programs, and every refusal: of a host list (named before anything is written) and of the
lane text (the refused job writes nothing, later levels write nothing, the first job is named, rec before u32 before poseidon).
tests/test_u32_plan.py runs the same plans through the library on the GPU and takes its helpers from here."""
import ctypes

import numpy as np
import pytest

import rows_lib
from rows_lib import NONE, NW, P, check_null_context, gate_constraints
from rows_lib import vpn as vp

ARITH, ADD, SUB, RANGE, CMP = range(5)
REC_ARITH, REC_BSUM, REC_RA = 0, 1, 7
N = 70            # not a power of two
THREADS = 256     # the kernel's block: a level of 257 jobs crosses it
COUNTS = [40, 1, 0, 257]
FAMILIES = ("rec", "poseidon", "u32")
REASONS = {1: "row out of range", 2: "unknown kind", 3: "operation slot out of range", 4: "subtraction borrow above 1", 5: "operands run past",
           6: "operand src above 1", 7: "cell operand column", 8: "cell operand row", 9: "operand value of 2^32 or more"}


def ug():
    from eth_lc_plonky2_amd import u32_gates
    return u32_gates


def rg():
    from eth_lc_plonky2_amd import recursion_gates
    return recursion_gates


@pytest.fixture(scope="module")
def emul():
    """tests/emu/libemu_plan_u32.so"""
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return rows_lib.build_emu("emu_plan_u32", (
        ("emu_plan_u32_job_bytes", c.c_uint, []), ("emu_plan_u32_operands", c.c_uint, [c.c_uint]), ("emu_plan_u32_problem_str", c.c_char_p, [c.c_uint]),
        ("emu_plan_u32_lists_problem", c.c_uint, [V, U, V, U, V, V, U, V, U, c.c_uint, U, V, V]),
        ("emu_plan_u32_level", None, [V, U, U, V, U, U, V, U, V, U, U, V, U, V, c.c_uint, U, V, U, c.c_uint]),
        ("emu_plan_u32_refusal", c.c_uint, [V, V, V, U, V, V])))


def emu_run(E, plan, n, start, order=None, threads=THREADS):
    """the plan through the emulated launches, level by level: (matrix, the three flag words)"""
    got = start.copy()
    flags = np.full(3, NONE, dtype=np.uint64)
    ends = [[0] + e.tolist() for e in (plan.rec_level_ends, plan.u32_level_ends, plan.pos_level_ends)]
    for l in (range(len(ends[0]) - 1) if order is None else order):
        E.emu_plan_u32_level(vp(plan.rec_jobs), ends[0][l], ends[0][l + 1], vp(plan.u32_jobs), ends[1][l], ends[1][l + 1], vp(plan.pos_jobs),
                             plan.pos_jobs.size, vp(plan.chain_ends), ends[2][l], ends[2][l + 1], vp(plan.operands), plan.operands.size,
                             rows_lib.vp(got), got.shape[0], n, rows_lib.vp(flags), l, threads)
    return got, [int(f) for f in flags]


def named(E, flags, plan):
    """(family, job, reason code) the three flag words name, as the entry point decodes them; None while nothing is refused"""
    family, job = ctypes.c_uint(0), ctypes.c_uint64(0)
    code = E.emu_plan_u32_refusal(rows_lib.vp(np.array(flags, dtype=np.uint64)), vp(plan.rec_level_ends), vp(plan.u32_level_ends),
                                  plan.u32_level_ends.size, ctypes.byref(family), ctypes.byref(job))
    return (FAMILIES[family.value], job.value, code) if code else None


def lists_problem(E, plan, n, noperands=None):
    """the host validation of the whole plan: None, or (family, job, reason code)"""
    family, job = ctypes.c_uint(0), ctypes.c_uint64(0)
    code = E.emu_plan_u32_lists_problem(vp(plan.rec_jobs), plan.rec_jobs.size, vp(plan.u32_jobs), plan.u32_jobs.size, vp(plan.pos_jobs),
                                        vp(plan.chain_ends), plan.chain_ends.size, vp(plan.operands), plan.operands.size if noperands is None else noperands,
                                        NW, n, ctypes.byref(family), ctypes.byref(job))
    return (FAMILIES[family.value], job.value, code) if code else None


def pattern(n, seed):
    """a matrix of any u64 words: cells a plan does not own must keep them"""
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(NW, n), dtype=np.uint64)


def random_plan(seed=7, n=N, counts=COUNTS):
    return ug().random_u32_plan(np.random.default_rng(seed), n, len(counts), counts)


def owned_cells(plan, n):
    """[NW][n] bool: the cells the u32 jobs of the plan own"""
    own = np.zeros((NW, n), dtype=bool)
    for j in plan.u32_jobs:
        own[ug().job_columns(int(j["kind"]), int(j["op"])), int(j["row"])] = True
    return own


def edge_levels():
    """force_high_max (output_high = 0xFFFFFFFF, inverse 0), a subtraction that borrows and whose borrow feeds the next one, a
    comparison of equal inputs - as IMM jobs in level 0 and again from CELLs in level 1"""
    g = rg()
    M = 0xFFFFFFFF
    level0 = [(0, ARITH, 0, [g.IMM(M), g.IMM(M), g.IMM(M)]), (1, SUB, 0, [g.IMM(5), g.IMM(9), g.IMM(0)]), (2, CMP, 0, [g.IMM(77), g.IMM(77)]),
              (3, ADD, 4, [g.IMM(M), g.IMM(M), g.IMM(M), g.IMM(2)]), (4, RANGE, 6, [g.IMM(M - 1 + P)])]
    level1 = [(5, ARITH, 2, [g.CELL(0, 4), g.CELL(0, 4), g.CELL(0, 4)]), (1, SUB, 5, [g.CELL(0, 3), g.CELL(1, 3), g.CELL(1, 4)]),
              (6, CMP, 0, [g.CELL(1, 3), g.CELL(1, 3)]), (7, SUB, 1, [g.IMM(0), g.IMM(M), g.CELL(2, 2)])]
    return [(level0, [], []), (level1, [], [])]


def mixed_levels():
    """REC_ARITHMETIC and REC_BASE_SUM in level 0; u32 jobs of level 1 read their outputs; level 2: a PoseidonGate chain whose swap bit
    is the result_bool of the comparison and whose inputs are u32 outputs, a rec job that reads an output_result, a u32 job"""
    g = rg()
    rec0 = [(0, REC_ARITH, 0, [g.IMM(1), g.IMM(0), g.IMM(123456789), g.IMM(1), g.IMM(0)]), (1, REC_BSUM, 0, [g.IMM(0x9ABCDEF5)])]
    u1 = [(10, CMP, 0, [g.CELL(0, 3), g.CELL(1, 0)]), (11, ADD, 2, [g.CELL(0, 3), g.CELL(1, 0), g.IMM(4000000000), g.CELL(1, 1)]),
          (12, SUB, 1, [g.CELL(0, 3), g.CELL(1, 0), g.CELL(1, 3)]), (13, ARITH, 1, [g.CELL(1, 0), g.CELL(0, 3), g.CELL(1, 2)])]
    chain = [(20, g.CELL(10, 2), [g.CELL(11, 16), g.CELL(11, 17), g.CELL(12, 8), g.CELL(13, 9), g.CELL(13, 10)] + [g.IMM(k) for k in range(7)]),
             (21, g.IMM(0), [g.PREV(k) for k in range(12)])]
    rec2 = [(0, REC_ARITH, 1, [g.IMM(3), g.IMM(1), g.CELL(11, 16), g.CELL(13, 9), g.CELL(12, 9)])]
    u2 = [(14, RANGE, 3, [g.CELL(13, 10)])]
    return [([], rec0, []), (u1, [], []), (u2, rec2, [chain])]


SOURCE_ROW = 60   # cells the matrix holds before the call: 2^32, 2, a non-canonical u32, 1, 16


def refusal_start(n=64):
    start = np.zeros((NW, n), dtype=np.uint64)
    start[:5, SOURCE_ROW] = [1 << 32, 2, 41 + P, 1, 16]
    return start


def refusal_levels(bad=None, bad_rec=False, bad_swap=False, bad_level=1):
    """three levels over 64 rows, each with u32 jobs, a rec job and a chain.  bad: a u32 item put into level `bad_level` (its row is
    free in every level); bad_rec: a RANDOM_ACCESS job on row 30 of level 1 whose index is the CELL holding 16; bad_swap: the swap of
    level 1's chain is the CELL holding 2.  Returns (levels, the levels as they must come out: without the refused jobs and without
    every level after the first refusal)"""
    g = rg()
    Z = [g.IMM(0)] * 12
    arith = lambda row, op, v: (row, REC_ARITH, op, [g.IMM(1), g.IMM(0), g.IMM(v), g.IMM(1), g.IMM(0)])   # noqa: E731
    u = [[(0, ARITH, 0, [g.IMM(3), g.IMM(5), g.IMM(7)]), (1, SUB, 0, [g.IMM(5), g.IMM(9), g.IMM(0)]), (2, ADD, 0, [g.IMM(1), g.IMM(2), g.IMM(3), g.IMM(2)])],
         [(3, RANGE, 0, [g.CELL(0, 3)]), (4, CMP, 0, [g.CELL(0, 3), g.IMM(21)]), (1, SUB, 3, [g.CELL(SOURCE_ROW, 2), g.IMM(1), g.CELL(1, 4)])],
         [(7, ADD, 1, [g.CELL(3, 0), g.CELL(1, 18), g.IMM(0), g.CELL(4, 2)])]]
    rec = [[arith(50, 0, 11)], [arith(51, 0, 12)], [arith(52, 0, 13)]]
    chains = [[[(40, g.IMM(0), Z)]], [[(41, g.CELL(SOURCE_ROW, 1) if bad_swap else g.CELL(SOURCE_ROW, 3), Z), (42, g.IMM(1), [g.PREV(k) for k in range(12)])]],
              [[(43, g.IMM(1), Z)]]]
    levels = [(list(u[l]), list(rec[l]), [list(c) for c in chains[l]]) for l in range(3)]
    kept = [(list(u[l]), list(rec[l]), [list(c) for c in chains[l]]) for l in range(3)]
    first = None
    if bad is not None:
        levels[bad_level][0].append(bad)
        first = bad_level
    if bad_rec:
        levels[1][1].append((30, REC_RA, 0, [g.CELL(SOURCE_ROW, 4)] + [g.IMM(k) for k in range(16)]))
        first = 1 if first is None else min(first, 1)
    if bad_swap:
        kept[1][2][0] = []
        first = 1 if first is None else min(first, 1)
    return levels, (kept if first is None else kept[:first + 1])


def index_of(plan, row, op=None):
    """the list index of the u32 job on `row` (and operation slot `op`)"""
    hit = [i for i, j in enumerate(plan.u32_jobs) if int(j["row"]) == row and (op is None or int(j["op"]) == op)]
    assert len(hit) == 1
    return hit[0]


BAD_ROW = 33


def reason_cases(n=64, by_cell=False):
    """{reason code: (the u32 item, what to patch in the packed job: {field: value})}; by_cell: the value reasons through CELL operands,
    which only the lane text sees"""
    g = rg()
    one, big, two = (g.CELL(SOURCE_ROW, 3), g.CELL(SOURCE_ROW, 0), g.CELL(SOURCE_ROW, 1)) if by_cell else (g.IMM(1), g.IMM(1 << 32), g.IMM(2))
    ok3 = [g.IMM(1), g.IMM(2), one]
    return {1: ((n, ARITH, 0, ok3), {}), 2: ((BAD_ROW, ARITH, 0, ok3), {"kind": 5}), 3: ((BAD_ROW, ARITH, 3, ok3), {}),
            4: ((BAD_ROW, SUB, 2, [g.IMM(9), g.IMM(2), two]), {}), 5: ((BAD_ROW, ADD, 0, [g.IMM(1)] * 4), {"first_operand": None}),
            6: ((BAD_ROW, CMP, 0, [g.IMM(1), g.PREV(0)]), {}), 7: ((BAD_ROW, RANGE, 2, [g.CELL(0, NW)]), {}),
            8: ((BAD_ROW, SUB, 2, [g.IMM(1), g.CELL(n, 0), g.IMM(0)]), {}), 9: ((BAD_ROW, ADD, 3, [g.IMM(1), one, big, g.IMM(0)]), {})}


def refused_plan(code, n=64, by_cell=False, bad_level=1):
    """(the packed plan with reason `code` in one u32 job of level `bad_level`, that job's index, the plan as it must come out)"""
    item, patch = reason_cases(n, by_cell)[code]
    levels, kept = refusal_levels(item, bad_level=bad_level)
    plan = ug().pack_u32_plan(levels)
    at = index_of(plan, item[0], item[2])
    for field, value in patch.items():
        plan.u32_jobs[at][field] = plan.operands.size - 3 if value is None else value
    return plan, at, ug().pack_u32_plan(kept)


# ------------------------------------------------------------------ without a GPU
def test_layout_counts_and_reason_texts(emul):
    import eth_lc_plonky2_amd as m
    b = m.binding
    assert emul.emu_plan_u32_job_bytes() == 16 == b.U32_PLAN_JOB_DTYPE.itemsize == ctypes.sizeof(b.U32PlanJob)
    assert ctypes.sizeof(b.WitnessPlanU32) == ctypes.sizeof(b.WitnessPlan) + 24
    assert [emul.emu_plan_u32_operands(k) for k in range(6)] == [3, 4, 3, 1, 2, 0] == [b.U32_PLAN_OPERANDS.get(k, 0) for k in range(6)]
    for code, text in REASONS.items():
        assert text.encode() in emul.emu_plan_u32_problem_str(code)


def test_random_plan_equals_the_model(emul):
    """n = 70, four levels of 40, 1, 0 and 257 jobs, every kind and every operation slot, CELL operands from level 1 on; on a matrix
    of arbitrary words, so a store outside the operation shows"""
    plan = random_plan()
    assert plan.u32_level_ends.tolist() == [40, 41, 41, 298]
    slots = set(zip(plan.u32_jobs["kind"].tolist(), plan.u32_jobs["op"].tolist()))
    assert slots == {(k, op) for k, (_, ops, _) in ug().U32_JOB_KINDS.items() for op in range(ops)} and len(slots) == 22
    first = plan.u32_jobs["first_operand"]
    assert (plan.operands["src"][:first[40]] == 0).all() and (plan.operands["src"][first[41]:] == 1).sum() > 200
    assert (plan.operands["v"][plan.operands["src"] == 0] >= np.uint64(P)).any(), "no IMM spelled v + p"
    start = pattern(N, 1)
    want = ug().plan_u32_model(start, plan)
    got, flags = emu_run(emul, plan, N, start)
    assert flags == [NONE] * 3 and (got == want).all()
    own = owned_cells(plan, N)
    assert (got[~own] == start[~own]).all() and (got[own] < np.uint64(P)).all() and own.sum() == sum(
        len(ug().job_columns(int(j["kind"]), int(j["op"]))) for j in plan.u32_jobs)
    # in reverse level order the CELLs are read before they are written
    assert not (emu_run(emul, plan, N, start, order=[3, 2, 1, 0])[0] == want).all()
    # other block sizes: the same cells
    assert (emu_run(emul, plan, N, start, threads=64)[0] == want).all()


def test_rows_of_a_plan_satisfy_their_gates(emul):
    """from a zero matrix every row with a job satisfies its gate's own program; one more on an output cell does not"""
    plan = random_plan(seed=9)
    got, flags = emu_run(emul, plan, N, np.zeros((NW, N), dtype=np.uint64))
    assert flags == [NONE] * 3
    gs = ug().reference_gateset(native=False)
    outputs = {ARITH: 3, ADD: 4, SUB: 3, RANGE: 0, CMP: 2}
    seen = set()
    for r in np.nonzero(plan.row_kind >= 0)[0]:
        kind = int(plan.row_kind[r])
        name = ug().U32_JOB_KINDS[kind][0]
        ops = sorted(int(j["op"]) for j in plan.u32_jobs if int(j["row"]) == r)
        row = [int(x) for x in got[:, r]]
        assert not any(gate_constraints(gs, name, row, [0, 0])), (name, r)
        col = outputs[kind] + {ARITH: 6, ADD: 6, SUB: 5, RANGE: 1, CMP: 0}[kind] * ops[0]
        row[col] = (row[col] + 1) % P
        assert any(gate_constraints(gs, name, row, [0, 0])), (name, r)
        seen.add(kind)
    assert seen == set(range(5))


def test_edge_jobs(emul):
    u = ug()
    plan = u.pack_u32_plan(edge_levels())
    start = pattern(64, 2)
    got, flags = emu_run(emul, plan, 64, start)
    assert flags == [NONE] * 3 and (got == u.plan_u32_model(start, plan)).all()
    M = 0xFFFFFFFF
    assert got[:6, 0].tolist() == [M, M, M, 0, M, 0], "output_high = 0xFFFFFFFF: output_low 0, inverse 0"
    assert got[12:18, 5].tolist() == [M, M, M, 0, M, 0], "the same from CELLs"
    assert got[:5, 1].tolist() == [5, 9, 0, (1 << 32) - 4, 1], "5 - 9 borrows"
    assert got[25:30, 1].tolist() == [0, (1 << 32) - 4, 1, 3, 1], "0 - (2^32 - 4) - 1 borrows again"
    assert got[:4, 2].tolist() == [77, 77, 1, 0] and got[:4, 6].tolist() == [(1 << 32) - 4] * 2 + [1, 0], "equal inputs: first <= second"
    assert got[24:30, 3].tolist() == [M, M, M, 2, M, 2] and got[6, 4] == M - 1, "the largest sum; an IMM spelled v + p"
    assert got[5:10, 7].tolist() == [0, M, 1, 0, 1]
    gs = u.reference_gateset(native=False)
    zero, _ = emu_run(emul, plan, 64, np.zeros((NW, 64), dtype=np.uint64))
    for r, kind in ((0, ARITH), (5, ARITH), (1, SUB), (7, SUB), (2, CMP), (6, CMP), (3, ADD), (4, RANGE)):
        assert not any(gate_constraints(gs, u.U32_JOB_KINDS[kind][0], [int(x) for x in zero[:, r]], [0, 0])), r


def test_mixed_plan_of_three_families(emul):
    u = ug()
    plan = u.pack_u32_plan(mixed_levels())
    assert plan.rec_jobs.size == 3 and plan.pos_jobs.size == 2 and plan.u32_jobs.size == 5 and set(plan.operands["src"].tolist()) == {0, 1, 2}
    start = pattern(64, 3)
    want = u.plan_u32_model(start, plan)
    got, flags = emu_run(emul, plan, 64, start)
    assert flags == [NONE] * 3 and (got == want).all()
    a, b = 123456789, 0x9ABCDEF5
    assert got[:3, 10].tolist() == [a, b, 1] and got[24, 20] == 1, "the swap bit is the comparison's result_bool"
    assert got[16, 11] == (a + b + 4000000000 + 1) & 0xFFFFFFFF and got[17, 11] == (a + b + 4000000001) >> 32
    assert got[8, 12] == a + (1 << 32) - b - 1 and got[9, 12] == 1 and got[9, 13] == (a * b + 0) & 0xFFFFFFFF
    assert got[:4, 20].tolist() == got[[16, 17, 8, 9], [11, 11, 12, 13]].tolist(), "the chain reads u32 outputs"
    assert got[7, 0] == (3 * int(got[16, 11]) * int(got[9, 13]) + 1) % P, "a rec job of level 2 reads u32 outputs"
    assert got[3, 14] == got[10, 13]
    # without its u32 jobs the plan is the one lcp2_witness_plan_rows runs
    base = u.pack_u32_plan([([], rec, chains) for _, rec, chains in mixed_levels()])
    assert base.u32_jobs.size == 0 and (emu_run(emul, base, 64, want)[0] == rg().run_witness_plan(base, NW, 64, start=want)).all()


def test_refusals_of_host_lists_name_the_job_before_anything_is_written(emul):
    """every reason as a structural or IMM case in level 1 of a three-level plan: the host validation names family, job and reason,
    so the entry point returns before its first launch (GPU: test_u32_plan.py checks the matrix)"""
    plan = ug().pack_u32_plan(refusal_levels()[0])
    assert lists_problem(emul, plan, 64) is None
    for code in REASONS:
        plan, at, _ = refused_plan(code)
        assert lists_problem(emul, plan, 64) == ("u32", at, code), code
    for code in (4, 9):   # the same through CELLs: only the device can see the value
        plan, at, _ = refused_plan(code, by_cell=True)
        assert lists_problem(emul, plan, 64) is None
    # accepted neighbours: a value of 2^32 - 1, the same spelled v + p, a borrow of 1, the last row and column
    g = rg()
    ok = [(BAD_ROW, ADD, 4, [g.IMM(0xFFFFFFFF), g.IMM(0xFFFFFFFF + P), g.CELL(63, NW - 1), g.IMM(P)]), (63, SUB, 5, [g.IMM(0), g.IMM(0), g.IMM(1 + P)])]
    assert lists_problem(emul, ug().pack_u32_plan([(ok, [], [])]), 64) is None
    # rec, then u32, then poseidon
    levels, _ = refusal_levels(reason_cases()[9][0])
    levels[2][1].append((31, REC_ARITH, 20, [g.IMM(0)] * 5))
    levels[0][2].append([(44, g.IMM(2), [g.IMM(0)] * 12)])
    plan = ug().pack_u32_plan(levels)
    assert lists_problem(emul, plan, 64) == ("rec", index_of_rec(plan, 31), 3)
    levels[2][1].pop()
    plan = ug().pack_u32_plan(levels)
    assert lists_problem(emul, plan, 64) == ("u32", index_of(plan, BAD_ROW), 9)
    levels[1][0].pop()
    assert lists_problem(emul, ug().pack_u32_plan(levels), 64) == ("poseidon", 1, 9)


def index_of_rec(plan, row):
    return plan.rec_jobs["row"].tolist().index(row)


@pytest.mark.parametrize("bad_level", [0, 1, 2])
def test_refusals_in_the_lane_text(emul, bad_level):
    """every reason in a list the host has not checked (and the two value reasons through CELLs), in level 0, 1 or 2: the refused
    job writes nothing, the other jobs of its level and every earlier level are written, later levels write nothing"""
    u = ug()
    start = refusal_start()
    for code in REASONS:
        plan, at, kept = refused_plan(code, by_cell=code in (4, 9), bad_level=bad_level)
        got, flags = emu_run(emul, plan, 64, start)
        assert named(emul, flags, plan) == ("u32", at, code), code
        assert (got == u.plan_u32_model(start, kept)).all(), code
        assert (got[:, BAD_ROW] == 0).all() and got[:, [0, 1, 2, 40, 50]].any(axis=0).all()
        later = [r for l, rows in enumerate(([3, 4, 41, 51], [7, 43, 52])) if l + 1 > bad_level for r in rows]
        assert not got[:, later].any()


def test_the_first_refused_job_is_named_rec_before_u32_before_poseidon(emul):
    u, g = ug(), rg()
    start = refusal_start()
    bad = reason_cases(by_cell=True)[4][0]
    # two refused u32 jobs in one level: the one that comes first in the list, whatever order the lanes ran in
    levels, kept = refusal_levels(bad)
    levels[1][0].append((34, RANGE, 6, [g.CELL(SOURCE_ROW, 0)]))
    plan = u.pack_u32_plan(levels)
    firsts = sorted(((index_of(plan, BAD_ROW), 4), (index_of(plan, 34), 9)))
    got, flags = emu_run(emul, plan, 64, start)
    assert named(emul, flags, plan) == ("u32",) + firsts[0] and (got == u.plan_u32_model(start, u.pack_u32_plan(kept))).all()
    # all three families refuse in level 1
    for bad_rec, bad_u32, bad_swap, family in ((True, True, True, "rec"), (False, True, True, "u32"), (False, False, True, "poseidon"),
                                               (True, False, True, "rec"), (True, True, False, "rec"), (False, True, False, "u32")):
        levels, kept = refusal_levels(bad if bad_u32 else None, bad_rec=bad_rec, bad_swap=bad_swap)
        plan, kept = u.pack_u32_plan(levels), u.pack_u32_plan(kept)
        got, flags = emu_run(emul, plan, 64, start)
        want = {"rec": ("rec", index_of_rec(plan, 30) if bad_rec else 0, 9), "u32": ("u32", index_of(plan, BAD_ROW) if bad_u32 else 0, 4),
                "poseidon": ("poseidon", 1, 9)}[family]
        assert named(emul, flags, plan) == want, (bad_rec, bad_u32, bad_swap)
        assert (flags[2] != NONE) == bad_u32 and (flags[1] != NONE) == bad_swap
        assert (got == u.plan_u32_model(start, kept)).all()
        assert not got[:, [7, 43, 52, 30, BAD_ROW]].any() and got[:, [3, 4, 51]].any(axis=0).all() and got[:, 41].any() != bad_swap


def test_the_decode_of_hand_built_flag_words(emul):
    """plan_refusal_u32 for rec_level_ends = [4, 4, 7] and u32_level_ends = [0, 5, 9]: flags[2] carries the job index shifted by
    level + 1; flags[0] says which family to read"""
    from types import SimpleNamespace
    plan = SimpleNamespace(rec_level_ends=np.array([4, 4, 7], dtype=np.uint32), u32_level_ends=np.array([0, 5, 9], dtype=np.uint32))
    assert named(emul, [NONE, NONE, NONE], plan) is None
    assert named(emul, [0x6FE, NONE, 0x204], plan) == ("u32", 0, 4)          # level 1: marker 4 + 2, job 0 at index 0 + 2
    assert named(emul, [0x6FE, 0x509, 0x609], plan) == ("u32", 4, 9)         # a chain of the level refused too: the u32 job
    assert named(emul, [0xAFE, NONE, 0xB05], plan) == ("u32", 8, 5)          # level 2: marker 7 + 3, job 8 at index 8 + 3
    assert named(emul, [0x708, 0x509, 0x809], plan) == ("rec", 4, 8)         # a rec job of level 2 before everything
    assert named(emul, [0x6FF, 0x509, NONE], plan) == ("poseidon", 5, 9)


def test_entry_point_checks_its_pointers_first():
    """without a device there is no context, and the null check comes first: LCP2_E_INVALID whatever the lists hold"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    structs = [plan_struct(m, plan) for plan in (ug().pack_u32_plan(refusal_levels()[0]), refused_plan(6)[0], ug().pack_u32_plan([]))]
    check_null_context(lambda a, mem, w: lib.lcp2_witness_plan_rows_u32(None, *a, mem, w, NW, 64), [(ctypes.byref(s),) for s, keep in structs] + [(None,)],
                       (m.MEM_HOST, m.MEM_DEVICE))


def plan_struct(m, plan, counts=None):
    """(the ctypes lcp2_witness_plan_u32 over the host arrays, the arrays kept alive)"""
    names = ("rec_jobs", "pos_jobs", "chain_ends", "operands", "rec_level_ends", "pos_level_ends", "u32_jobs", "u32_level_ends")
    keep = {name: np.ascontiguousarray(getattr(plan, name)) for name in names}
    ptr = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    c = counts or {}
    k = keep
    base = m.binding.WitnessPlan(ptr(k["rec_jobs"]), c.get("nrec", k["rec_jobs"].size), ptr(k["rec_level_ends"]), ptr(k["pos_jobs"]),
                                 c.get("npos", k["pos_jobs"].size), ptr(k["chain_ends"]), c.get("nchains", k["chain_ends"].size), ptr(k["pos_level_ends"]),
                                 ptr(k["operands"]), c.get("noperands", k["operands"].size), c.get("nlevels", k["u32_level_ends"].size))
    return m.binding.WitnessPlanU32(base, ptr(k["u32_jobs"]), c.get("nu32", k["u32_jobs"].size), ptr(k["u32_level_ends"])), keep
