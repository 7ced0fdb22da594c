"""lcp2_witness_plan_rows: a recorded witness plan that holds PoseidonGate rows - rec jobs and PoseidonGate CHAINS (inputs: immediates,
cells, or outputs of the chain's previous row), run level by level on the device without the host in between.

Without a GPU: csrc/pos_plan.hpp - the validation, the portable job and chain texts and one level's two launches - compiled for the
CPU (tests/emu/emu_plan.cpp) against poseidon_py.gate_row, recursion_gates.run_witness_plan and the gates' own constraint programs,
and the null check of the entry point.  On the GPU: the same through the library (k_pos_plan_chains walks a chain with a 16-lane
group), exact equality of whole matrices, the refusals, and a proof from a device-filled matrix."""
import ctypes

import numpy as np
import pytest

import rows_lib
from rows_lib import INVALID, MAX, NONE, NW, P, TAG, DeviceMatrix, check_null_context, gate_constraints, upload
from rows_lib import refusal as named
from rows_lib import run_levels as emu_run
from rows_lib import vpn as vp

ARITH, BSUM, RA = 0, 1, 7
REASONS = {1: "row out of range", 2: "operands run past", 3: "src above 2", 4: "first job of a chain", 5: "PREV as the swap", 6: "column of 12 or more",
           7: "cell operand column", 8: "cell operand row", 9: "swap value not 0 or 1"}


def rg():
    from eth_lc_plonky2_amd import recursion_gates
    return recursion_gates


@pytest.fixture(scope="module")
def emul():
    """tests/emu/libemu_plan.so; emu_run(E, plan, n, ..) runs a plan's levels through it, named(E, flags, plan) decodes its flag words"""
    return rows_lib.emu_plan()


def lists_problem(E, plan, n, noperands=None):
    """the host validation of the whole plan: None, or (family, job, reason code)"""
    family, job = ctypes.c_uint(0), ctypes.c_uint64(0)
    code = E.emu_plan_lists_problem(vp(plan.rec_jobs), plan.rec_jobs.size, vp(plan.pos_jobs), vp(plan.chain_ends), plan.chain_ends.size,
                                    vp(plan.operands), plan.operands.size if noperands is None else noperands, NW, n, ctypes.byref(family), ctypes.byref(job))
    return (("rec", "poseidon")[family.value], job.value, code) if code else None


def arith(row, op, v, c=(1, 0)):
    """an ARITHMETIC job whose output (column 4 op + 3) is c0 * v * 1 + c1 * 0"""
    g = rg()
    return (row, ARITH, op, [g.IMM(c[0]), g.IMM(c[1]), g.IMM(v), g.IMM(1), g.IMM(0)])


def reason_cases(n=64):
    """{reason code: (chain, noperands shortfall)}: a two-job chain whose SECOND job (the first for reasons 1, 2, 4 of a one-job
    chain) is refused for that reason; and the accepted neighbours of the boundaries"""
    g = rg()
    Z = [g.IMM(0)] * 12
    ok = (0, g.IMM(0), Z)
    return {1: [(n, g.IMM(0), Z)], 2: [ok], 3: [ok, (1, g.IMM(0), Z[:5] + [(1, 0, 3)] + Z[6:])], 4: [(0, g.IMM(0), [g.PREV(0)] + Z[1:])],
            5: [ok, (1, g.PREV(0), Z)], 6: [ok, (1, g.IMM(0), Z[:11] + [g.PREV(12)])], 7: [ok, (1, g.IMM(0), [g.CELL(0, NW)] + Z[1:])],
            8: [ok, (1, g.CELL(n, 0), Z)], 9: [ok, (1, g.IMM(2), Z)]}


def accepted_cases(n=64):
    g = rg()
    Z = [g.IMM(0)] * 12
    ok = (0, g.IMM(0), Z)
    return [[(n - 1, g.IMM(0), Z)], [ok, (1, g.IMM(1), [g.CELL(n - 1, NW - 1)] + Z[1:10] + [g.PREV(11), g.IMM(MAX)])], [ok, (1, g.IMM(P + 1), Z)]]


# ------------------------------------------------------------------ without a GPU
def test_layout_and_every_reason(emul):
    import eth_lc_plonky2_amd as m
    g, b = rg(), m.binding
    assert emul.emu_plan_pos_job_bytes() == 8 == b.POS_JOB_DTYPE.itemsize
    assert emul.emu_plan_operand_bytes() == 16 == b.REC_OPERAND_DTYPE.itemsize
    assert emul.emu_plan_pos_operands() == 13 == g.POS_PLAN_OPERANDS and (b.PLAN_IMM, b.PLAN_CELL, b.PLAN_PREV) == (0, 1, 2)
    for code, chain in reason_cases().items():
        plan = g.pack_witness_plan([([], [chain])])
        last = plan.pos_jobs.size - 1
        noperands = plan.operands.size - (1 if code == 2 else 0)
        for k in range(last):
            assert emul.emu_plan_pos_problem(vp(plan.pos_jobs[k:k + 1]), k == 0, vp(plan.operands), noperands, NW, 64) == 0
        assert emul.emu_plan_pos_problem(vp(plan.pos_jobs[last:]), last == 0, vp(plan.operands), noperands, NW, 64) == code
        assert REASONS[code].encode() in emul.emu_plan_problem_str(code)
        assert lists_problem(emul, plan, 64, noperands) == ("poseidon", last, code)
    for chain in accepted_cases():
        assert lists_problem(emul, g.pack_witness_plan([([], [chain])]), 64) is None
    # PREV in a rec job: "operand src above 1"
    plan = g.pack_witness_plan([([(0, ARITH, 0, [g.IMM(1)] * 4 + [g.PREV(0)])], [])])
    assert lists_problem(emul, plan, 64) == ("rec", 0, 5)


def random_chains(seed, n, lengths):
    """chains of the given lengths on distinct rows above row 8 (rows 0..7 hold source cells): operands of all three sources, both
    swap values as IMM (non-canonical spellings too) and as CELL, edge inputs"""
    g = rg()
    rng = np.random.default_rng(seed)
    rows = iter(rng.permutation(np.arange(8, n)).tolist())
    edge = [0, P - 1, MAX, P, 1]
    chains = []
    for length in lengths:
        chain = []
        for k in range(length):
            def operand(i):
                pick = int(rng.integers(0, 4))
                if pick == 0 and k:
                    return g.PREV(int(rng.integers(0, 12)))
                if pick == 1:
                    return g.CELL(int(rng.integers(0, 8)), int(rng.integers(0, NW)))
                return g.IMM(edge[int(rng.integers(0, 5))] if pick == 2 else int(rng.integers(0, 1 << 64, dtype=np.uint64)))
            swap = [g.IMM(0), g.IMM(1), g.IMM(P + 1), g.IMM(P), g.CELL(0, 0), g.CELL(1, 0)][int(rng.integers(0, 6))]
            chain.append((next(rows), swap, [operand(i) for i in range(12)]))
        chains.append(chain)
    return chains


def source_matrix(n, seed, fill=0):
    """rows 0..7 hold what CELL operands read: cells (0, 0) = 0 and (1, 0) = p + 1 (swap flags), the rest any u64 with edge values"""
    rng = np.random.default_rng(seed)
    start = np.full((NW, n), fill, dtype=np.uint64)
    start[:, :8] = rng.integers(0, 1 << 64, size=(NW, 8), dtype=np.uint64)
    start[0, 0], start[0, 1], start[1, 2], start[2, 3], start[3, 4] = 0, P + 1, MAX, P - 1, P
    return start


def expected_rows(chains, start):
    """the chains' rows in Python integers, independently of run_witness_plan: {row: 135 values}"""
    from eth_lc_plonky2_amd import poseidon_py as pp
    out = {}
    for chain in chains:
        prev = None
        for row, swap, inputs in chain:
            vals = [int(start[col, v]) % P if src == 1 else prev[col] if src == 2 else v % P for v, col, src in [swap] + inputs]
            out[row] = pp.gate_row(vals[1:], vals[0])
            if prev is not None:
                for (v, col, src), x in zip(inputs, out[row][:12]):
                    assert src != 2 or x == prev[col], "PREV is not the previous row's output"
            prev = out[row][12:24]
    return out


def test_random_jobs_equal_the_python_row(emul):
    g = rg()
    n = 64
    chains = random_chains(5, n, [1, 2, 7, 3, 1, 5])
    srcs = {src for chain in chains for _, swap, ins in chain for _, _, src in [swap] + ins}
    assert srcs == {0, 1, 2}
    plan = g.pack_witness_plan([([], chains)])
    start = source_matrix(n, 5, TAG)
    got, flags = emu_run(emul, plan, n, start)
    assert flags == [NONE, NONE]
    want = expected_rows(chains, start)
    assert {sw for r in want.values() for sw in [r[24]]} == {0, 1}
    for row, cells in want.items():
        assert got[:, row].tolist() == cells, row
    untouched = np.ones(n, dtype=bool)
    untouched[list(want)] = False
    assert (got[:, untouched] == start[:, untouched]).all()
    assert (got == g.run_witness_plan(plan, NW, n, start=start)).all()


def test_verifier_plan_level_by_level(emul):
    """verifier_plan(64, seed) through the emulated launches equals run_witness_plan; in reverse level order it does not; every
    PoseidonGate row and every rec row satisfies its gate's own program, and a changed output cell does not"""
    g = rg()
    n = 64
    plan = g.verifier_plan(n, seed=4)
    assert len(plan.rec_level_ends) == 5 and plan.chain_ends.size >= 6 and {0, 1, 2} == set(plan.operands["src"].tolist())
    assert (plan.operands["src"][:plan.leaves] == 0).all() and plan.leaves == int(plan.pos_jobs[0]["first_operand"])
    got, flags = emu_run(emul, plan, n)
    assert flags == [NONE, NONE] and (got == plan.expected).all() and (plan.expected < np.uint64(P)).all()
    got, _ = emu_run(emul, plan, n, order=[4, 3, 2, 1, 0])
    assert not (got == plan.expected).all()
    other = g.verifier_plan(n, seed=5)
    assert (other.operands[plan.leaves:] == plan.operands[plan.leaves:]).all() and (other.pos_jobs == plan.pos_jobs).all()
    assert not (other.expected == plan.expected).all()
    gs = g.verifier_gateset(native=False)
    seen = set()
    for r in range(n):
        name = gs.names[int(plan.gate_of_row[r])]
        if name == "NoopGate":
            assert not plan.expected[:, r].any()
            continue
        seen.add(name)
        row, consts = [int(x) for x in plan.expected[:, r]], [int(plan.c0[r]), int(plan.c1[r])]
        assert not any(gate_constraints(gs, name, row, consts)), (name, r)
        out = {"PoseidonGate": 12, "BaseSumGate": 0, "ArithmeticGate": 3, "ArithmeticExtensionGate": 6}[name]
        row[out] = (row[out] + 1) % P
        assert any(gate_constraints(gs, name, row, consts)), (name, r)
    assert seen == {"PoseidonGate", "BaseSumGate", "ArithmeticGate", "ArithmeticExtensionGate"}


def refusal_levels(bad_swap=True, bad_rec=False):
    """three levels over 64 rows.  Level 0 writes 2 into cell (0, 3), 16 into (0, 7), 1 into (0, 11).  Level 1: three ARITHMETIC jobs
    (and, bad_rec, a RANDOM_ACCESS job on row 30 whose index is the CELL holding 16), chain A (rows 10, 11), chain B (rows 12 .. 15;
    bad_swap: the swap flag of row 14 is the CELL holding 2) and chain C (rows 16, 17).  Level 2: one ARITHMETIC job on row 40 and a
    chain on row 41.  Returns (levels, levels as they must come out: without the refused jobs and what follows them)."""
    g = rg()
    Z = [g.IMM(0)] * 12
    ins = lambda k: [g.IMM(100 * k + i) for i in range(12)]   # noqa: E731
    follow = lambda k: [g.PREV(i) for i in range(4)] + [g.IMM(k)] * 4 + [g.PREV(8 + i) for i in range(4)]   # noqa: E731
    level0 = [arith(0, 0, 2), arith(0, 1, 16), arith(0, 2, 1), arith(1, 0, 7)]
    rec1 = [arith(2, 0, 8), arith(3, 0, 9), arith(4, 5, 10)]
    A = [(10, g.CELL(0, 11), ins(1)), (11, g.IMM(0), follow(2))]
    B = [(12, g.IMM(1), ins(3)), (13, g.IMM(0), follow(4)), (14, g.CELL(0, 3) if bad_swap else g.IMM(0), follow(5)), (15, g.IMM(1), follow(6))]
    C = [(16, g.IMM(0), ins(7)), (17, g.CELL(0, 11), follow(8))]
    bad = [(30, RA, 0, [g.CELL(0, 7)] + [g.IMM(k) for k in range(16)])] if bad_rec else []
    level2 = ([arith(40, 0, 11)], [[(41, g.IMM(0), Z)]])
    levels = [(level0, []), (rec1 + bad, [A, B, C]), level2]
    if not (bad_swap or bad_rec):
        return levels, levels
    return levels, [(level0, []), (rec1, [A, B[:2] if bad_swap else B, C])]


def test_refusals_of_host_lists_write_nothing(emul):
    """each reason as an IMM or structural case inside a three-level plan: the host validation names the job, so the entry point
    returns before its first launch (GPU: test_refusals_on_the_device checks the matrix)"""
    g = rg()
    for code, chain in reason_cases().items():
        levels, _ = refusal_levels(False)
        levels[1][1].insert(1, chain)
        plan = g.pack_witness_plan(levels)
        at = 2 + len(chain) - 1
        if code == 2:
            plan.pos_jobs[at]["first_operand"] = plan.operands.size - 12
        assert lists_problem(emul, plan, 64) == ("poseidon", at, code)


def test_a_cell_swap_of_two_stops_its_chain_and_later_levels(emul):
    g = rg()
    levels, kept = refusal_levels()
    plan = g.pack_witness_plan(levels)
    assert lists_problem(emul, plan, 64) is None, "only the device can see the value"
    got, flags = emu_run(emul, plan, 64)
    assert named(emul, flags, plan) == ("poseidon", 4, 9)
    want = g.run_witness_plan(g.pack_witness_plan(kept), NW, 64)
    assert (got == want).all()
    assert want[:, [10, 11, 12, 13, 16, 17]].any(axis=0).all() and not got[:, [14, 15, 40, 41]].any()


def test_both_families_refuse_in_one_level_the_rec_job_is_named(emul):
    g = rg()
    levels, kept = refusal_levels(bad_rec=True)
    plan = g.pack_witness_plan(levels)
    got, flags = emu_run(emul, plan, 64)
    bad_at = int(plan.rec_level_ends[0]) + plan.rec_jobs["kind"][plan.rec_level_ends[0]:plan.rec_level_ends[1]].tolist().index(RA)
    assert named(emul, flags, plan) == ("rec", bad_at, 9) and flags[1] == (4 << 8 | 9)
    assert (got == g.run_witness_plan(g.pack_witness_plan(kept), NW, 64)).all() and not got[:, [14, 15, 30, 40, 41]].any()
    levels, kept = refusal_levels(bad_swap=False, bad_rec=True)   # the rec family alone: the chains of its level run in full
    plan = g.pack_witness_plan(levels)
    got, flags = emu_run(emul, plan, 64)
    assert named(emul, flags, plan) == ("rec", bad_at, 9) and flags[1] == NONE
    assert (got == g.run_witness_plan(g.pack_witness_plan(kept), NW, 64)).all() and got[:, 15].any() and not got[:, [30, 40, 41]].any()


def test_the_decode_of_hand_built_flag_words(emul):
    """plan_refusal (row_flag.hpp), the decode both entry points use, on flag words built by hand for rec_level_ends = [4, 4, 7] -
    level 1 holds no rec job, so its key (6) and level 2's first index (7) are what plan_gate keeps apart.  The expected triples are
    what the Python loop this export replaced returned"""
    plan = rows_lib.rec_plan(None, None, [4, 4, 7])
    assert named(emul, [NONE, NONE], plan) is None
    assert named(emul, [0x101, NONE], plan) == ("rec", 0, 1)        # level 0: index job + 1
    assert named(emul, [0x409, NONE], plan) == ("rec", 3, 9)
    assert named(emul, [0x90B, NONE], plan) == ("rec", 6, 11)       # the last level: index job + 3
    assert named(emul, [0x708, NONE], plan) == ("rec", 4, 8)        # the first job after the empty level: index 7, above level 1's key
    assert named(emul, [0x708, 0x509], plan) == ("rec", 4, 8)       # both families refused in level 2: the rec job
    assert named(emul, [0x6FF, 0x509], plan) == ("poseidon", 5, 9)  # a chain of the empty level (marker 4 + 2): the family bit
    assert named(emul, [0xAFF, 0x004], plan) == ("poseidon", 0, 4)  # a chain of the last level (marker 7 + 3)
    assert named(emul, [0x30A, NONE], rows_lib.rec_plan(None, None, [3])) == ("rec", 2, 10)   # a rec-gate call of one level


def plan_struct(m, plan, counts=None):
    """(the ctypes lcp2_witness_plan over the host arrays, the arrays kept alive)"""
    keep = [np.ascontiguousarray(a) for a in (plan.rec_jobs, plan.pos_jobs, plan.chain_ends, plan.operands, plan.rec_level_ends, plan.pos_level_ends)]
    ptr = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    c = counts or {}
    s = m.binding.WitnessPlan(ptr(keep[0]), c.get("nrec", keep[0].size), ptr(keep[4]), ptr(keep[1]), c.get("npos", keep[1].size), ptr(keep[2]),
                              c.get("nchains", keep[2].size), ptr(keep[5]), ptr(keep[3]), c.get("noperands", keep[3].size), c.get("nlevels", keep[4].size))
    return s, keep


def test_entry_point_checks_its_pointers_first():
    """without a device there is no context, and the null check comes first: LCP2_E_INVALID whatever the lists hold"""
    import eth_lc_plonky2_amd as m
    g = rg()
    lib = m.load_library()
    good = g.pack_witness_plan(refusal_levels(False)[0])
    bad = g.pack_witness_plan([([], [reason_cases()[4]])])
    empty = g.pack_witness_plan([])
    structs = [plan_struct(m, plan) for plan in (good, bad, empty)]
    check_null_context(lambda a, mem, w: lib.lcp2_witness_plan_rows(None, *a, mem, w, NW, 64), [(ctypes.byref(s),) for s, keep in structs] + [(None,)],
                       (m.MEM_HOST, m.MEM_DEVICE))


# ------------------------------------------------------------------ on the GPU
class Resident:
    """the four lists of a plan in HBM"""

    def __init__(self, ctx, plan):
        self.ctx, self.plan = ctx, plan
        self.rec, self.pos, self.chains, self.ops = (upload(ctx, a) for a in (plan.rec_jobs, plan.pos_jobs, plan.chain_ends, plan.operands))

    def run(self, wires_ptr, ncols, n):
        p = self.plan
        self.ctx.witness_plan_rows(self.rec, self.pos, self.chains, self.ops, p.rec_level_ends, p.pos_level_ends, wires_ptr, ncols, n,
                                   nrec=p.rec_jobs.size, npos=p.pos_jobs.size, nchains=p.chain_ends.size, noperands=p.operands.size)

    def free(self):
        for ptr in (self.rec, self.pos, self.chains, self.ops):
            self.ctx.buffer_free(ptr)


def run_on_device(ctx, plan, start, device_lists=False):
    """(the matrix after the call, the Lcp2Error it raised or None)"""
    import eth_lc_plonky2_amd as m
    dm = DeviceMatrix(ctx, start)
    res = Resident(ctx, plan) if device_lists else None
    error = None
    try:
        if device_lists:
            res.run(dm.ptr, start.shape[0], start.shape[1])
        else:
            ctx.witness_plan_rows(plan.rec_jobs, plan.pos_jobs, plan.chain_ends, plan.operands, plan.rec_level_ends, plan.pos_level_ends,
                                  dm.ptr, start.shape[0], start.shape[1])
    except m.Lcp2Error as e:
        error = e
    got = dm.read()
    dm.free()
    if res:
        res.free()
    return got, error


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3, 4, 5, 16, 17])
def test_single_level_chain_shapes(gpu_ctx, count):
    """`count` chains (around the four groups of a wave and the 16 of a block) of lengths 1, 2 and 17 in turn - divergent trip
    counts inside a wave - with an empty chain in the middle, on a matrix filled with a non-zero pattern: host and resident lists"""
    g = rg()
    n = 256
    lengths = [(1, 2, 17)[i % 3] for i in range(count)]
    if count >= 3:
        lengths[count // 2] = 0
    chains = random_chains(count, n, lengths)
    plan = g.pack_witness_plan([([], chains)])
    assert plan.chain_ends.size == count
    start = source_matrix(n, count, TAG)
    want = g.run_witness_plan(plan, NW, n, start=start)
    rows = expected_rows(chains, start)
    assert all(want[:, r].tolist() == cells for r, cells in rows.items())
    for device_lists in (False, True):
        got, error = run_on_device(gpu_ctx, plan, start, device_lists)
        assert error is None and (got == want).all(), device_lists


@pytest.mark.gpu
def test_a_sponge_of_forty_rows(gpu_ctx):
    """20 rows absorb 8 immediates each with the capacity as PREV 8..11, then 20 rows take PREV for every input; the outputs of
    row 19 are hash_no_pad of the 160 absorbed values"""
    from eth_lc_plonky2_amd import poseidon_py as pp
    g = rg()
    n = 64
    rng = np.random.default_rng(40)
    absorbed = [int(x) for x in rng.integers(0, P, size=160, dtype=np.uint64)]
    chain = [(3 + k, g.IMM(0), [g.IMM(v) for v in absorbed[8 * k:8 * k + 8]] + ([g.IMM(0)] * 4 if k == 0 else [g.PREV(8 + i) for i in range(4)]))
             for k in range(20)]
    chain += [(23 + k, g.IMM(0), [g.PREV(i) for i in range(12)]) for k in range(20)]
    plan = g.pack_witness_plan([([], [chain])])
    want = g.run_witness_plan(plan, NW, n)
    assert want[12:16, 22].tolist() == pp.hash_no_pad(absorbed)
    for device_lists in (False, True):
        got, error = run_on_device(gpu_ctx, plan, np.zeros((NW, n), dtype=np.uint64), device_lists)
        assert error is None and (got == want).all()


@pytest.mark.gpu
def test_verifier_plan_on_the_device(gpu_ctx):
    """verifier_plan(256, seed) from a zero matrix with host lists and with resident lists; then only the leaf prefix of the resident
    operand buffer is rewritten and the plan replayed: the second seed's matrix"""
    g = rg()
    n = 256
    plan, second = g.verifier_plan(n, seed=8), g.verifier_plan(n, seed=9)
    zero = np.zeros((NW, n), dtype=np.uint64)
    got, error = run_on_device(gpu_ctx, plan, zero)
    assert error is None and (got == plan.expected).all()
    res, dm = Resident(gpu_ctx, plan), DeviceMatrix(gpu_ctx, zero)
    res.run(dm.ptr, NW, n)
    assert (dm.read() == plan.expected).all()
    assert (second.operands[plan.leaves:] == plan.operands[plan.leaves:]).all() and not (second.expected == plan.expected).all()
    gpu_ctx.buffer_write(res.ops, np.ascontiguousarray(second.operands[:plan.leaves]).view(np.uint64))
    res.run(dm.ptr, NW, n)
    assert (dm.read() == second.expected).all()
    dm.free()
    res.free()


@pytest.mark.gpu
def test_levels_empty_in_one_family(gpu_ctx):
    """rec jobs only: exactly what lcp2_rec_gate_rows writes from the same lists; chains only: exact"""
    g = rg()
    n = 64
    chain = g.chain_plan(n, seed=6)
    empty = g.pack_witness_plan([])
    plan = type(empty)(rec_jobs=chain.jobs, pos_jobs=empty.pos_jobs, chain_ends=empty.chain_ends, operands=chain.operands,
                       rec_level_ends=chain.level_ends, pos_level_ends=np.zeros(chain.level_ends.size, dtype=np.uint32))
    zero = np.zeros((NW, n), dtype=np.uint64)
    dm = DeviceMatrix(gpu_ctx, zero)
    gpu_ctx.rec_gate_rows(chain.jobs, chain.operands, chain.level_ends, dm.ptr, NW, n)
    by_rec = dm.read()
    dm.free()
    assert (by_rec == chain.expected).all()
    for device_lists in (False, True):
        got, error = run_on_device(gpu_ctx, plan, zero, device_lists)
        assert error is None and (got == by_rec).all()
    chains = random_chains(11, n, [2, 3])
    only = g.pack_witness_plan([([], chains[:1]), ([], []), ([], chains[1:])])
    start = source_matrix(n, 11)
    got, error = run_on_device(gpu_ctx, only, start, True)
    assert error is None and (got == g.run_witness_plan(only, NW, n, start=start)).all()


@pytest.mark.gpu
def test_long_host_list(gpu_ctx):
    """2^19 + 3 PoseidonGate records, each a chain of its own: the pinned staging buffer holds 2^19 of them, so the jobs go up in
    two pieces (and chain_ends behind them).  One job repeated 2^19 times - equal jobs for one row leave that value, as
    test_rec_rows.py::test_long_host_list argues - then three distinct ones."""
    g = rg()
    n = 64
    count = (1 << 19) + 3
    chains = [[(5 + k, g.IMM(k & 1), [g.IMM(1000 * k + i) for i in range(12)])] for k in range(4)]
    base = g.pack_witness_plan([([], chains)])
    jobs = np.concatenate([np.resize(base.pos_jobs[:1], count - 3), base.pos_jobs[1:]])
    assert jobs.nbytes > 4 << 20
    plan = type(base)(rec_jobs=base.rec_jobs, pos_jobs=jobs, chain_ends=np.arange(1, count + 1, dtype=np.uint32), operands=base.operands,
                      rec_level_ends=np.zeros(1, dtype=np.uint32), pos_level_ends=np.array([count], dtype=np.uint32))
    got, error = run_on_device(gpu_ctx, plan, np.zeros((NW, n), dtype=np.uint64))
    assert error is None and (got == g.run_witness_plan(base, NW, n)).all()


@pytest.mark.gpu
def test_refusals_on_the_device(gpu_ctx):
    """every structural reason in a device list, in a chain of level 0, 1 and 2 of a three-level plan in turn: the rows before the
    refused one, the other chains and the rec jobs of its level and everything earlier are written, nothing later; a host list writes
    nothing; the error names family and job.  Then the CELL swap case and both families from host and device lists, the argument
    checks, and the context still works.  Refusals by validation: every index is checked before it is used."""
    import eth_lc_plonky2_amd as m
    g = rg()
    lib, n = gpu_ctx.lib, 64
    zero = np.zeros((NW, n), dtype=np.uint64)
    for code, chain in reason_cases().items():
        if code == 9:
            continue   # an IMM value is a host check; the CELL case follows
        level_of = code % 3
        levels, _ = refusal_levels(False)
        levels[0] = (levels[0][0], [[(50, g.IMM(0), [g.IMM(5)] * 12)]])
        moved = [(20 + k if r < 64 else r, sw, ins) for k, (r, sw, ins) in enumerate(chain)]   # rows 20, 21: free in every level
        middle = len(levels[level_of][1]) // 2
        levels[level_of][1].insert(middle, moved)
        plan = g.pack_witness_plan(levels)
        before = sum(len(c) for lv in levels[:level_of] for c in lv[1]) + sum(len(c) for c in levels[level_of][1][:middle])
        at = before + len(moved) - 1
        if code == 2:
            plan.pos_jobs[at]["first_operand"] = plan.operands.size - 12
        kept = [list(lv) for lv in levels[:level_of + 1]]
        kept[level_of][1] = [c[:-1] if c is moved else c for c in kept[level_of][1]]
        want = g.run_witness_plan(g.pack_witness_plan([tuple(lv) for lv in kept]), NW, n)
        got, error = run_on_device(gpu_ctx, plan, zero)
        assert error is not None and error.status == INVALID and "plan rows: poseidon job %d: " % at in str(error) and REASONS[code] in str(error)
        assert not got.any(), "a refused host list wrote something"
        got, error = run_on_device(gpu_ctx, plan, zero, device_lists=True)
        assert error is not None and error.status == INVALID and "plan rows: poseidon job %d: " % at in str(error) and REASONS[code] in str(error)
        assert (got == want).all(), code
    for bad_swap, bad_rec in ((True, False), (True, True), (False, True)):
        levels, kept = refusal_levels(bad_swap, bad_rec)
        plan = g.pack_witness_plan(levels)
        want = g.run_witness_plan(g.pack_witness_plan(kept), NW, n)
        rec_at = int(plan.rec_level_ends[0]) + (plan.rec_jobs["kind"][plan.rec_level_ends[0]:plan.rec_level_ends[1]].tolist().index(RA) if bad_rec else 0)
        text = "plan rows: rec job %d: random-access index" % rec_at if bad_rec else "plan rows: poseidon job 4: swap value not 0 or 1"
        for device_lists in (False, True):
            got, error = run_on_device(gpu_ctx, plan, zero, device_lists)
            assert error is not None and error.status == INVALID and text in str(error), str(error)
            assert (got == want).all(), (bad_swap, bad_rec, device_lists)
    # the argument checks
    good = g.pack_witness_plan(refusal_levels(False)[0])
    want = g.run_witness_plan(good, NW, n)
    dm = DeviceMatrix(gpu_ctx, zero)
    wp, h = ctypes.c_void_p(dm.ptr), gpu_ctx.handle
    call = lambda s, mem=m.MEM_HOST, w=wp, ncols=NW: lib.lcp2_witness_plan_rows(h, ctypes.byref(s) if s is not None else None, mem, w, ncols, n)   # noqa: E731
    s, keep = plan_struct(m, good)
    assert call(None) == INVALID and call(s, w=None) == INVALID and call(s, mem=2) == INVALID and call(s, ncols=134) == INVALID
    assert lib.lcp2_witness_plan_rows(None, ctypes.byref(s), m.MEM_HOST, wp, NW, n) == INVALID
    for field in ("rec_jobs", "pos_jobs", "chain_ends", "operands", "rec_level_ends", "pos_level_ends"):
        s, keep = plan_struct(m, good)
        setattr(s, field, None)
        assert call(s) == INVALID and call(s, mem=m.MEM_DEVICE) == INVALID, field
    for field, values in (("rec_level_ends", [4, 8, 7]), ("rec_level_ends", [4, 3, 8]), ("pos_level_ends", [0, 3, 3]), ("pos_level_ends", [0, 5, 4]),
                          ("chain_ends", [2, 6, 8, 8]), ("chain_ends", [2, 1, 8, 9])):
        broken = type(good)(**vars(good))
        setattr(broken, field, np.array(values, dtype=np.uint32))
        s, keep = plan_struct(m, broken)
        assert call(s) == INVALID and field.encode() in lib.lcp2_last_error(h), (field, values)
    empty = g.pack_witness_plan([([], [[], []]), ([], [])])   # empty chains, empty levels: nothing to do
    s, keep = plan_struct(m, empty)
    assert call(s) == 0 and call(s, mem=m.MEM_DEVICE) == 0
    s, keep = plan_struct(m, good, {"nrec": 0, "npos": 0})
    assert call(s) == 0
    assert not dm.read().any()
    dm.free()
    got, error = run_on_device(gpu_ctx, good, zero)   # the context still works after the refusals
    assert error is None and (got == want).all()


@pytest.mark.gpu
def test_proof_from_a_device_filled_matrix(gpu_ctx, oracle):
    """2^10 rows of verifier_plan filled on the device by ONE call from resident lists.  The zero matrix is LCP2_E_UNSAT (a zero
    PoseidonGate row is not a permutation).  The proof from the filled matrix equals the proof from the Python-computed host matrix
    and the oracle's proof of it, word for word, and verifies."""
    import eth_lc_plonky2_amd as m
    import oracle_lib
    g = rg()
    gs = g.verifier_gateset()
    params = m.standard_params(10, gs.num_selectors + 2)
    plan = g.verifier_plan(1 << 10, seed=13)
    circ, pis = g.verifier_plan_circuit(params, plan)
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
    res = Resident(gpu_ctx, plan)
    res.run(dm.ptr, params.num_wires, circ.n)
    got = data.prove(dm.ptr, pis, mem=m.MEM_DEVICE)
    dm.free()
    res.free()
    assert (got == from_host).all(), "the proof from the device-filled matrix differs from the host matrix' proof"
    assert (got == want).all(), "the proof differs from the oracle's"
    data.verify(got, pis)
    data.close()
