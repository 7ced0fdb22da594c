"""lcp2_witness_plan_rows_sha without a GPU: csrc/sha_plan.hpp - the validation, the one-lane reference of k_sha_plan_jobs and one
level's four launches with the four flag words - compiled for the CPU (tests/emu/emu_plan_sha.cpp) against
sha_plan_cases.plan_sha_model cell for cell, against hashlib, against the SHA gates' own constraint programs, and every refusal: of a
host list (named before anything is written) and of the lane text (the refused job writes nothing, later levels write nothing in any
family, the first job is named, rec before SHA before u32 before poseidon).  tests/test_sha_plan.py runs the same plans through the
library on the GPU."""
import ctypes

import numpy as np
import pytest

import rows_lib
import sha_plan_cases as cases
from rows_lib import NONE, NW, P, check_null_context
from rows_lib import vpn as vp
from sha_plan_cases import BAD_FIRST, FAMILIES, REASONS, REFUSAL_N, ROWS, SHA_FIRST, VALUE_REASON
from test_sha_rows import programs, violated  # noqa: F401  (programs is a fixture)
from test_u32_plan_emu import BAD_ROW, index_of, index_of_rec
from test_u32_plan_emu import reason_cases as u32_reason_cases

THREADS = 256


@pytest.fixture(scope="module")
def emul():
    """tests/emu/libemu_plan_sha.so"""
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return rows_lib.build_emu("emu_plan_sha", (
        ("emu_plan_sha_job_bytes", c.c_uint, []), ("emu_plan_sha_operands", c.c_uint, []), ("emu_plan_sha_problem_str", c.c_char_p, [c.c_uint]),
        ("emu_plan_sha_lists_problem", c.c_uint, [V, U, V, U, V, U, V, V, U, V, U, c.c_uint, U, V, V]),
        ("emu_plan_sha_level", None, [V, U, U, V, U, U, V, U, U, V, U, V, U, U, V, U, V, c.c_uint, U, V, U, c.c_uint]),
        ("emu_plan_sha_refusal", c.c_uint, [V, V, V, V, U, V, V])))


@pytest.fixture(scope="module")
def emu_u32():
    """tests/emu/libemu_plan_u32.so: the level of the existing three-family runner"""
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return rows_lib.build_emu("emu_plan_u32", (("emu_plan_u32_level", None, [V, U, U, V, U, U, V, U, V, U, U, V, U, V, c.c_uint, U, V, U, c.c_uint]),))


def emu_run(E, plan, n, start, order=None, threads=THREADS):
    """the plan through the emulated launches, level by level: (matrix, the four flag words)"""
    got = np.array(start)
    flags = np.full(4, NONE, dtype=np.uint64)
    ends = [[0] + e.tolist() for e in (plan.rec_level_ends, plan.sha_level_ends, plan.u32_level_ends, plan.pos_level_ends)]
    for l in (range(len(ends[0]) - 1) if order is None else order):
        E.emu_plan_sha_level(vp(plan.rec_jobs), ends[0][l], ends[0][l + 1], vp(plan.sha_jobs), ends[1][l], ends[1][l + 1], vp(plan.u32_jobs), ends[2][l],
                             ends[2][l + 1], vp(plan.pos_jobs), plan.pos_jobs.size, vp(plan.chain_ends), ends[3][l], ends[3][l + 1], vp(plan.operands),
                             plan.operands.size, rows_lib.vp(got), got.shape[0], n, rows_lib.vp(flags), l, threads)
    return got, [int(f) for f in flags]


def named(E, flags, plan):
    """(family, job, reason code) the four flag words name, as the entry point decodes them; None while nothing is refused"""
    family, job = ctypes.c_uint(0), ctypes.c_uint64(0)
    code = E.emu_plan_sha_refusal(rows_lib.vp(np.array(flags, dtype=np.uint64)), vp(plan.rec_level_ends), vp(plan.u32_level_ends), vp(plan.sha_level_ends),
                                  plan.sha_level_ends.size, ctypes.byref(family), ctypes.byref(job))
    return (FAMILIES[family.value], job.value, code) if code else None


def lists_problem(E, plan, n, noperands=None):
    """the host validation of the whole plan: None, or (family, job, reason code)"""
    family, job = ctypes.c_uint(0), ctypes.c_uint64(0)
    code = E.emu_plan_sha_lists_problem(vp(plan.rec_jobs), plan.rec_jobs.size, vp(plan.sha_jobs), plan.sha_jobs.size, vp(plan.u32_jobs), plan.u32_jobs.size,
                                        vp(plan.pos_jobs), vp(plan.chain_ends), plan.chain_ends.size, vp(plan.operands),
                                        plan.operands.size if noperands is None else noperands, NW, n, ctypes.byref(family), ctypes.byref(job))
    return (FAMILIES[family.value], job.value, code) if code else None


# ------------------------------------------------------------------ the cases
def test_layout_and_reason_texts(emul):
    import eth_lc_plonky2_amd as m
    b, s = m.binding, m.sha_plan
    assert emul.emu_plan_sha_job_bytes() == 8 == b.SHA_PLAN_JOB_DTYPE.itemsize and emul.emu_plan_sha_operands() == 16 == b.SHA_PLAN_OPERANDS
    assert ctypes.sizeof(b.WitnessPlanSha) == ctypes.sizeof(b.WitnessPlanU32) + 24
    for code, text in REASONS.items():
        assert text.encode() in emul.emu_plan_sha_problem_str(code)
    assert [s.digest_cell(10, i) for i in range(8)] == [(317, 2), (317, 5), (317, 8), (318, 2), (318, 5), (318, 8), (319, 2), (319, 5)]
    assert [s.message_cell(10, t) for t in (0, 15)] == [(58, 5), (88, 5)]
    # the two cells in the model's rows: the digest, and W_t on its round E row
    msg = list(range(100, 116))
    rows = cases.model_rows(msg)
    assert [int(rows[col, row]) for row, col in (s.digest_cell(0, i) for i in range(8))] == cases.ref.digest_words(msg)
    assert [int(rows[col, row]) for row, col in (s.message_cell(0, t) for t in range(16))] == msg


@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases_equal_the_model(emul, name):
    """(a)-(f): cell for cell, and the cells outside the 108 x 310 blocks of a plan of SHA jobs alone untouched"""
    plan, n, start, want = cases.case(name)
    got, flags = emu_run(emul, plan, n, start)
    assert flags == [NONE] * 4 and (got == want).all()
    own = cases.owned_by_sha(plan, n)
    assert own.sum() == 108 * 310 * plan.sha_jobs.size and (got[own] < np.uint64(1 << 32)).all()
    if not plan.u32_jobs.size + plan.rec_jobs.size + plan.pos_jobs.size:
        assert (got[~own] == start[~own]).all() and not (got[own] == start[own]).all()
    assert lists_problem(emul, plan, n) is None


def test_flat_jobs_end_at_the_last_row_and_hold_the_special_messages():
    for name, count in (("flat1", 1), ("flat2", 2), ("flat5", 5)):
        plan, n, start, want = cases.case(name)
        assert plan.sha_jobs.size == count and plan.sha_level_ends.tolist() == [count] and int(plan.sha_jobs["first_row"].max()) + ROWS == n
        assert (plan.operands["src"] == 0).all()
    seen = {tuple(int(o["v"]) for o in cases.case(name)[0].operands[16 * k:16 * k + 16]) for name, count in (("flat1", 1), ("flat2", 2), ("flat5", 5))
            for k in range(count)}
    assert {tuple(msg) for msg in cases.SPECIAL} <= seen


def test_merkle_root_is_hashlib(emul):
    """7 jobs in 3 levels, the parents' words the digest cells of their children: the root's digest cells hold hashlib's root; in
    reverse level order the cells are read before they are written"""
    plan, n, start, want = cases.case("merkle")
    _, rows, root = cases.merkle_parts()
    got, _ = emu_run(emul, plan, n, start)
    assert cases.digest_of(got, rows[6]) == root == cases.digest_of(want, rows[6])
    assert cases.digest_of(emu_run(emul, plan, n, start, order=[2, 1, 0])[0], rows[6]) != root


def test_mixed_plan_passes_values_between_the_four_families(emul):
    plan, n, start, want = cases.case("mixed")
    assert (plan.sha_jobs.size, plan.u32_jobs.size, plan.rec_jobs.size, plan.pos_jobs.size) == (3, 1, 1, 1)
    got, _ = emu_run(emul, plan, n, start)
    d0, d1 = cases.digest_of(got, 0), cases.digest_of(got, ROWS)
    total = d1[0] + d0[7] + 4000000000 + 3
    assert got[16, cases.MIXED_U32_ROW] == total & 0xFFFFFFFF and got[17, cases.MIXED_U32_ROW] == total >> 32, "the u32 job reads digest cells"
    assert got[23, cases.MIXED_REC_ROW] == d0[4], "the rec job's output is a digest word"
    msg = [int(got[col, row]) for row, col in (cases.sp().message_cell(2 * ROWS, t) for t in range(16))]
    assert msg[:2] == [total & 0xFFFFFFFF, d0[4]] and msg[8:] == d1[2:] + [d0[1], d0[3]], "the SHA job of level 2 reads all of them"
    assert got[:12, cases.MIXED_CHAIN_ROW].tolist() == d0 + d1[:4] and got[24, cases.MIXED_CHAIN_ROW] == 1, "the chain reads digest cells"
    assert cases.digest_of(got, 2 * ROWS) == cases.ref.digest_words(msg)


def test_noncanonical_and_own_row_operands(emul):
    plan, n, start, want = cases.case("noncanonical")
    got, _ = emu_run(emul, plan, n, start)
    assert [int(got[col, row]) for row, col in (cases.sp().message_cell(1, t) for t in range(4))] == [5, 7, 0xFFFFFFFE, 0]
    assert got[120, n - 1] == P + 7, "the source cell keeps its spelling"
    plan, n, start, want = cases.case("own_rows")
    got, _ = emu_run(emul, plan, n, start)
    assert [int(got[col, row]) for row, col in (cases.sp().message_cell(2, t) for t in range(3))] == list(cases.OWN_WORDS)
    assert got[5, 2 + 48 + 6] != cases.OWN_WORDS[0], "W_3's own cell now holds W_3, not the word it held before the call"


def test_sha_rows_of_a_plan_satisfy_their_gates(emul, programs):  # noqa: F811
    """the rows the lane text fills satisfy the SHA gates' own programs: the job of level 2 of the mixed plan (words from cells of
    three families) and the job that reads its own rows"""
    for name, first_row in (("mixed", 2 * ROWS), ("own_rows", 2)):
        plan, n, start, want = cases.case(name)
        got, _ = emu_run(emul, plan, n, start)
        rows = [[int(x) for x in got[:108, first_row + lr]] for lr in range(ROWS)]
        assert violated(programs, rows) == [], name


# ------------------------------------------------------------------ refusals
def test_refusals_of_host_lists_name_the_job_before_anything_is_written(emul):
    good = cases.sp().pack_sha_plan(cases.refusal_levels()[0])
    assert lists_problem(emul, good, REFUSAL_N) is None
    for code in REASONS:
        plan, at, _ = cases.refused_plan(code)
        assert lists_problem(emul, plan, REFUSAL_N) == ("sha", at, code), code
    plan, at, _ = cases.refused_plan(VALUE_REASON, by_cell=True)   # only the device can see the value
    assert lists_problem(emul, plan, REFUSAL_N) is None
    # accepted neighbours: the last rows, a value of 2^32 - 2 spelled v + p, the last row and column as a cell
    g = cases.rg()
    ok = [(REFUSAL_N - ROWS, [g.IMM(0xFFFFFFFE + P), g.CELL(REFUSAL_N - 1, NW - 1)] + cases.imms(range(14)))]
    assert lists_problem(emul, cases.sp().pack_sha_plan([(ok, [], [], [])]), REFUSAL_N) is None
    # rec, then SHA, then u32, then poseidon - whatever the level
    bad_sha, bad_u32 = cases.reason_cases()[VALUE_REASON][0], u32_reason_cases()[9][0]
    levels, _ = cases.refusal_levels(bad_sha, bad_level=2, bad_u32=bad_u32)
    levels[2][2].append((31, cases.REC_ARITH, 20, [g.IMM(0)] * 5))
    levels[0][3].append([(44, g.IMM(2), [g.IMM(0)] * 12)])
    plan = cases.sp().pack_sha_plan(levels)
    assert lists_problem(emul, plan, REFUSAL_N) == ("rec", index_of_rec(plan, 31), 3)
    levels[2][2].pop()
    plan = cases.sp().pack_sha_plan(levels)
    assert lists_problem(emul, plan, REFUSAL_N) == ("sha", cases.index_of_sha(plan, BAD_FIRST), VALUE_REASON)
    levels[2][0].pop()
    plan = cases.sp().pack_sha_plan(levels)
    assert lists_problem(emul, plan, REFUSAL_N) == ("u32", index_of(plan, BAD_ROW), 9)
    levels[1][1].pop()
    assert lists_problem(emul, cases.sp().pack_sha_plan(levels), REFUSAL_N) == ("poseidon", 1, 9)


LATER = ([3, 4, 41, 51], [7, 43, 52])   # rows the u32 jobs, the chain and the rec job of levels 1 and 2 write


@pytest.mark.parametrize("bad_level", [0, 1, 2])
def test_refusals_in_the_lane_text(emul, bad_level):
    """every reason in a list the host has not checked (the value reason through a CELL too), in level 0, 1 or 2: the refused job
    writes nothing, the other jobs of its level - of all four families - and every earlier level are written, later levels write
    nothing in any family"""
    start = cases.refusal_start()
    for code, by_cell in [(code, False) for code in REASONS] + [(VALUE_REASON, True)]:
        plan, at, kept = cases.refused_plan(code, by_cell=by_cell, bad_level=bad_level)
        got, flags = emu_run(emul, plan, REFUSAL_N, start)
        assert named(emul, flags, plan) == ("sha", at, code), code
        assert flags[1] == NONE and flags[2] == NONE
        assert (got == cases.plan_sha_model(start, kept)).all(), code
        assert not got[:, BAD_FIRST:].any(), "the refused job wrote something"
        for l in range(3):
            rows = list(range(SHA_FIRST[l], SHA_FIRST[l] + ROWS)) + (LATER[l - 1] if l else [0, 1, 2, 40, 50])
            assert got[:, rows].any(axis=0).all() == (l <= bad_level), (code, l)
            assert got[:, rows].any() == (l <= bad_level), (code, l)


def test_the_first_refused_job_is_named_rec_before_sha_before_u32_before_poseidon(emul):
    s = cases.sp()
    start = cases.refusal_start()
    bad_sha, bad_u32 = cases.reason_cases(by_cell=True)[VALUE_REASON][0], u32_reason_cases(by_cell=True)[4][0]
    # two refused SHA jobs in one level: the one that comes first in the list
    levels, kept = cases.refusal_levels(bad_sha)
    levels[1][0].insert(0, (0, cases.imms(range(3)) + [cases.rg().PREV(1)] + cases.imms(range(12))))   # refused by src: writes nothing on rows 0..309
    plan = s.pack_sha_plan(levels)
    got, flags = emu_run(emul, plan, REFUSAL_N, start)
    assert named(emul, flags, plan) == ("sha", cases.index_of_sha(plan, 0), 3) and flags[3] >> 8 == cases.index_of_sha(plan, 0) + 2
    assert (got == cases.plan_sha_model(start, s.pack_sha_plan(kept))).all()
    # every subset of the four families refusing in level 1
    for mask in range(1, 16):
        bad_rec, with_sha, with_u32, bad_swap = bool(mask & 1), bool(mask & 2), bool(mask & 4), bool(mask & 8)
        levels, kept = cases.refusal_levels(bad_sha if with_sha else None, bad_u32=bad_u32 if with_u32 else None, bad_rec=bad_rec, bad_swap=bad_swap)
        plan, kept = s.pack_sha_plan(levels), s.pack_sha_plan(kept)
        got, flags = emu_run(emul, plan, REFUSAL_N, start)
        want = (("rec", index_of_rec(plan, 30), 9) if bad_rec else ("sha", cases.index_of_sha(plan, BAD_FIRST), VALUE_REASON) if with_sha
                else ("u32", index_of(plan, BAD_ROW), 4) if with_u32 else ("poseidon", 1, 9))
        assert named(emul, flags, plan) == want, mask
        assert [(f != NONE) for f in flags[1:]] == [bad_swap, with_u32, with_sha], mask
        assert (got == cases.plan_sha_model(start, kept)).all(), mask
        assert not got[:, [7, 43, 52, 30, BAD_ROW]].any() and not got[:, SHA_FIRST[2]:].any() and got[:, SHA_FIRST[1]:SHA_FIRST[2]].any(axis=0).all()


def test_the_decode_of_hand_built_flag_words(emul):
    """plan_refusal_sha for rec_level_ends = [4, 4, 7], u32_level_ends = [0, 5, 9] and sha_level_ends = [2, 2, 6]: flags[3] carries the
    job index shifted by level + 1; flags[0] says which family to read, and without the SHA marker the words mean what they meant"""
    from types import SimpleNamespace
    u32 = lambda a: np.array(a, dtype=np.uint32)   # noqa: E731
    plan = SimpleNamespace(rec_level_ends=u32([4, 4, 7]), u32_level_ends=u32([0, 5, 9]), sha_level_ends=u32([2, 2, 6]))
    assert named(emul, [NONE] * 4, plan) is None
    assert named(emul, [0x5FD, NONE, NONE, 0x206], plan) == ("sha", 1, 6)           # level 0: marker 4 + 1, job 1 at index 1 + 1
    assert named(emul, [0xAFD, 0x509, 0xB05, 0x503], plan) == ("sha", 2, 3)         # level 2: marker 7 + 3, job 2 at index 2 + 3; before u32 and poseidon
    assert named(emul, [0xAFD, NONE, NONE, 0x801], plan) == ("sha", 5, 1)
    assert named(emul, [0x708, 0x509, 0x809, 0x503], plan) == ("rec", 4, 8)         # a rec job of level 2 before everything
    assert named(emul, [0x6FE, 0x509, 0x609, NONE], plan) == ("u32", 4, 9)          # the three-word decode, unchanged
    assert named(emul, [0x6FF, 0x509, NONE, NONE], plan) == ("poseidon", 5, 9)


def test_without_sha_jobs_it_is_the_existing_runner(emul, emu_u32):
    """nsha = 0: the matrix and the flag words of the three-family level of tests/emu/emu_plan_u32.cpp (flags[3] is never touched), and
    without u32 jobs too the two words of rows_lib.run_levels - also when jobs are refused"""
    from test_u32_plan_emu import mixed_levels, refusal_levels, refusal_start
    s = cases.sp()
    bad_u32 = u32_reason_cases(by_cell=True)[4][0]
    for small, start in ((mixed_levels(), cases.pattern(64, 3)), (refusal_levels(bad_u32, bad_rec=True, bad_swap=True)[0], refusal_start()),
                         (refusal_levels(bad_u32, bad_swap=True)[0], refusal_start())):
        plan = s.pack_sha_plan([([],) + tuple(level) for level in small])
        got, flags = emu_run(emul, plan, 64, start)
        ref, ref_flags = start.copy(), np.full(3, NONE, dtype=np.uint64)
        ends = [[0] + e.tolist() for e in (plan.rec_level_ends, plan.u32_level_ends, plan.pos_level_ends)]
        for l in range(3):
            emu_u32.emu_plan_u32_level(vp(plan.rec_jobs), ends[0][l], ends[0][l + 1], vp(plan.u32_jobs), ends[1][l], ends[1][l + 1], vp(plan.pos_jobs),
                                       plan.pos_jobs.size, vp(plan.chain_ends), ends[2][l], ends[2][l + 1], vp(plan.operands), plan.operands.size,
                                       rows_lib.vp(ref), NW, 64, rows_lib.vp(ref_flags), l, THREADS)
        assert (got == ref).all() and flags[:3] == [int(f) for f in ref_flags] and flags[3] == NONE
        assert not (got == start).all()
    base = s.pack_sha_plan([([], [], rec, chains) for _, rec, chains in refusal_levels(None, bad_swap=True)[0]])
    got, flags = emu_run(emul, base, 64, refusal_start())
    ref, ref_flags = rows_lib.run_levels(rows_lib.emu_plan(), base, 64, start=refusal_start(), threads=THREADS)
    assert (got == ref).all() and flags == ref_flags + [NONE, NONE] and ref_flags[1] != NONE


def test_entry_point_checks_its_pointers_first():
    """without a device there is no context, and the null check comes first: LCP2_E_INVALID whatever the lists hold"""
    import eth_lc_plonky2_amd as m
    lib = m.load_library()
    plans = (cases.case("mixed")[0], cases.refused_plan(3)[0], cases.sp().pack_sha_plan([]))
    structs = [cases.plan_struct(m, plan) for plan in plans]
    check_null_context(lambda a, mem, w: lib.lcp2_witness_plan_rows_sha(None, *a, mem, w, NW, 64), [(ctypes.byref(s),) for s, keep in structs] + [(None,)],
                       (m.MEM_HOST, m.MEM_DEVICE))
