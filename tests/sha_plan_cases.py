"""What tests/test_sha_plan_emu.py (CPU) and tests/test_sha_plan.py (GPU) share (test harness only): the model of
lcp2_witness_plan_rows_sha over Python integers, and the plans both run - flat levels, a Merkle tree chained through digest cells,
all four families in one plan, empty levels, non-canonical inputs, an operand inside the job's own rows, and the refusals.

A case is (plan, n, start): the namespace of sha_plan.pack_sha_plan, the row count, and a [135][n] matrix of arbitrary words (with
the few cells a case reads set), so that a store outside the 108 x 310 blocks shows.  The model's matrix is computed once per case."""
import hashlib
import struct

import numpy as np

import sha_rows_ref as ref
from rows_lib import NW, P
from test_sha_rows import SPECIAL, model_rows, scattered_rows
from test_u32_plan_emu import ADD, SOURCE_ROW
from test_u32_plan_emu import refusal_levels as small_refusal_levels

ROWS, COLUMNS = ref.ROWS, ref.COLUMNS
REC_ARITH = 0
FAMILIES = ("rec", "poseidon", "u32", "sha")
REASONS = {1: "rows out of range", 2: "operands run past", 3: "operand src above 1", 4: "cell operand column", 5: "cell operand row",
           6: "operand value of 2^32 or more"}
VALUE_REASON = 6


def sp():
    from eth_lc_plonky2_amd import sha_plan
    return sha_plan


def rg():
    from eth_lc_plonky2_amd import recursion_gates
    return recursion_gates


def ug():
    from eth_lc_plonky2_amd import u32_gates
    return u32_gates


def pattern(n, seed):
    """a matrix of any u64 words: cells a plan does not own must keep them"""
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(NW, n), dtype=np.uint64)


def words(rng):
    return [int(x) for x in rng.integers(0, 1 << 32, size=16)]


def imms(msg):
    return [rg().IMM(w) for w in msg]


def digest_cells(first_row, which=range(8)):
    return [rg().CELL(*sp().digest_cell(first_row, i)) for i in which]


# ------------------------------------------------------------------ the model
def one_level(plan, lv):
    """the rec jobs, u32 jobs and chains of level lv as a one-level plan of u32_gates.plan_u32_model (the operand list whole)"""
    from types import SimpleNamespace
    cut = lambda ends: ((int(ends[lv - 1]) if lv else 0), int(ends[lv]))   # noqa: E731
    (rb, re), (ub, ue), (cb, ce) = cut(plan.rec_level_ends), cut(plan.u32_level_ends), cut(plan.pos_level_ends)
    first = int(plan.chain_ends[cb - 1]) if cb else 0
    last = int(plan.chain_ends[ce - 1]) if ce else 0
    u32 = lambda a: np.array(a, dtype=np.uint32)   # noqa: E731
    return SimpleNamespace(rec_jobs=plan.rec_jobs[rb:re], rec_level_ends=u32([re - rb]), u32_jobs=plan.u32_jobs[ub:ue], u32_level_ends=u32([ue - ub]),
                           pos_jobs=plan.pos_jobs[first:last], chain_ends=u32(plan.chain_ends[cb:ce]) - np.uint32(first), pos_level_ends=u32([ce - cb]),
                           operands=plan.operands)


def plan_sha_model(start, plan):
    """lcp2_witness_plan_rows_sha in Python integers: the matrix after the plan ran on `start`.  Per level the SHA jobs are resolved
    against the matrix as it stood BEFORE the level and their rows written (sha_rows_ref.expected_rows), then the other three
    families run through u32_gates.plan_u32_model on the level alone"""
    out = start.copy()
    for lv in range(len(plan.sha_level_ends)):
        jobs = plan.sha_jobs[(int(plan.sha_level_ends[lv - 1]) if lv else 0):int(plan.sha_level_ends[lv])]
        resolved = []
        for j in jobs:
            first = int(j["first_operand"])
            msg = [int(out[int(o["col"]), int(o["v"])]) % P if int(o["src"]) == 1 else int(o["v"]) % P for o in plan.operands[first:first + 16]]
            assert all(w < 1 << 32 for w in msg), msg
            resolved.append(msg)
        for j, msg in zip(jobs, resolved):
            out[:COLUMNS, int(j["first_row"]):int(j["first_row"]) + ROWS] = model_rows(msg)
        out = ug().plan_u32_model(out, one_level(plan, lv))
    return out


def owned_by_sha(plan, n):
    """[NW][n] bool: the 108 x 310 blocks of the SHA jobs"""
    own = np.zeros((NW, n), dtype=bool)
    for j in plan.sha_jobs:
        own[:COLUMNS, int(j["first_row"]):int(j["first_row"]) + ROWS] = True
    return own


def digest_of(matrix, first_row):
    return [int(matrix[col, row]) for row, col in (sp().digest_cell(first_row, i) for i in range(8))]


# ------------------------------------------------------------------ (a) flat levels, all IMM
def flat_case(njobs, seed=None, specials=True):
    """njobs independent hashes in one level on scattered rows, the last block flush against row n"""
    rng = np.random.default_rng(2000 + njobs if seed is None else seed)
    n = ROWS * njobs + (0 if njobs == 1 else 7)
    msgs = [words(rng) for _ in range(njobs)]
    if specials:
        for k, msg in enumerate(SPECIAL[:njobs] if njobs > 1 else SPECIAL[2:]):
            msgs[(2 * k + 1) % njobs] = list(msg)
    rows = scattered_rows(rng, njobs, n)
    assert max(rows) + ROWS == n
    plan = sp().pack_sha_plan([([(r, imms(msg)) for r, msg in zip(rows, msgs)], [], [], [])])
    return plan, n, pattern(n, 10 + njobs)


# ------------------------------------------------------------------ (b) a Merkle tree through digest cells
MERKLE_N = 7 * ROWS + 5


def merkle_parts():
    """(leaves [8][8] u32, the first rows of the 7 hashes bottom level first - not in level order, the hashlib root as 8 words)"""
    rng = np.random.default_rng(31)
    leaves = rng.integers(0, 1 << 32, size=(8, 8), dtype=np.uint64)
    rows = scattered_rows(rng, 7, MERKLE_N)
    assert rows != sorted(rows)
    nodes = [struct.pack(">8I", *[int(w) for w in leaf]) for leaf in leaves]
    while len(nodes) > 1:
        nodes = [hashlib.sha256(nodes[k] + nodes[k + 1]).digest() for k in range(0, len(nodes), 2)]
    return leaves, rows, list(struct.unpack(">8I", nodes[0]))


def merkle_case():
    leaves, rows, _ = merkle_parts()
    plan = sp().pack_sha_plan([(level, [], [], []) for level in sp().merkle_levels(leaves, rows)])
    assert plan.sha_level_ends.tolist() == [4, 6, 7] and (plan.operands["src"][16 * 4:] == 1).all()
    return plan, MERKLE_N, pattern(MERKLE_N, 32)


# ------------------------------------------------------------------ (c) all four families
MIXED_N = 3 * ROWS + 13
MIXED_U32_ROW, MIXED_REC_ROW, MIXED_CHAIN_ROW = 3 * ROWS + 1, 3 * ROWS + 4, 3 * ROWS + 9


def mixed_levels():
    """level 0: two SHA jobs; level 1: an ADD_MANY job and a rec ARITHMETIC job (0 * m0 * m1 + 1 * addend: the addend, a u32) that
    read digest cells; level 2: a SHA job whose words are the u32 output cell, the rec output cell, IMMs and a digest cell, beside a
    PoseidonGate chain that reads digest cells"""
    g, s = rg(), sp()
    rng = np.random.default_rng(41)
    sha0 = [(ROWS, imms(words(rng))), (0, imms(words(rng)))]
    u1 = [(MIXED_U32_ROW, ADD, 2, [g.CELL(*s.digest_cell(ROWS, 0)), g.CELL(*s.digest_cell(0, 7)), g.IMM(4000000000), g.IMM(3)])]
    rec1 = [(MIXED_REC_ROW, REC_ARITH, 5, [g.IMM(0), g.IMM(1), g.IMM(9), g.IMM(9), g.CELL(*s.digest_cell(0, 4))])]
    msg = [g.CELL(MIXED_U32_ROW, 6 * 2 + 4), g.CELL(MIXED_REC_ROW, 4 * 5 + 3)] + imms(words(rng)[:6]) + digest_cells(ROWS, range(2, 8)) + digest_cells(0, (1, 3))
    chain = [[(MIXED_CHAIN_ROW, g.IMM(1), digest_cells(0) + digest_cells(ROWS, range(4)))]]
    return [(sha0, [], [], []), ([], u1, rec1, []), ([(2 * ROWS, msg)], [], [], chain)]


def mixed_case():
    return sp().pack_sha_plan(mixed_levels()), MIXED_N, pattern(MIXED_N, 42)


# ------------------------------------------------------------------ (d) empty levels, (e) non-canonical inputs, (f) own rows
def empty_levels_case():
    """level 0: one SHA job; level 1: empty in every family; level 2: no SHA job, one u32 job reading the digest; level 3: a SHA job"""
    g, s = rg(), sp()
    rng = np.random.default_rng(51)
    n = 2 * ROWS + 3
    levels = [([(3, imms(words(rng)))], [], [], []), ([], [], [], []),
              ([], [(0, ADD, 0, [g.CELL(*s.digest_cell(3, 5)), g.IMM(1), g.IMM(2), g.IMM(0)])], [], []),
              ([(3 + ROWS, digest_cells(3) + [g.CELL(0, 4)] + imms(words(rng)[:7]))], [], [], [])]
    plan = s.pack_sha_plan(levels)
    assert plan.sha_level_ends.tolist() == [1, 1, 1, 2] and plan.u32_level_ends.tolist() == [0, 0, 1, 1]
    return plan, n, pattern(n, 52)


def noncanonical_case():
    """an IMM spelled p + 5 and a cell holding p + 7: both accepted, the words are 5 and 7"""
    g = rg()
    n = ROWS + 2
    start = pattern(n, 61)
    start[120, n - 1] = P + 7
    msg = [g.IMM(P + 5), g.CELL(n - 1, 120), g.IMM(0xFFFFFFFE + P), g.IMM(P)] + imms(words(np.random.default_rng(62))[:12])
    return sp().pack_sha_plan([([(1, msg)], [], [], [])]), n, start


OWN_WORDS = (0x12345678, 0xFFFFFFFF, 7)


def own_rows_case():
    """operands that are cells of the job's OWN rows - its message cell W_3, a digest cell, a bit column of its first row - yield the
    words the matrix held before the call: all 16 operands are read before the first store"""
    g, s = rg(), sp()
    n = ROWS + 4
    start = pattern(n, 71)
    cells = [s.message_cell(2, 3), s.digest_cell(2, 6), (2, 40)]
    for (row, col), w in zip(cells, OWN_WORDS):
        start[col, row] = w
    msg = [g.CELL(*c) for c in cells] + imms(words(np.random.default_rng(72))[:13])
    return s.pack_sha_plan([([(2, msg)], [], [], [])]), n, start


def wide_level_case():
    """70 hashes in one level: more jobs than one block of several waves would hold"""
    return flat_case(70, specials=False)


CASES = {"flat1": lambda: flat_case(1), "flat2": lambda: flat_case(2), "flat5": lambda: flat_case(5), "merkle": merkle_case, "mixed": mixed_case,
         "empty_levels": empty_levels_case, "noncanonical": noncanonical_case, "own_rows": own_rows_case}
_BUILT = {}


def case(name):
    """(plan, n, start, the model's matrix) of a case of CASES or of wide_level_case ("wide"), built once; nobody writes to them"""
    if name not in _BUILT:
        plan, n, start = wide_level_case() if name == "wide" else CASES[name]()
        want = plan_sha_model(start, plan)
        start.setflags(write=False)
        want.setflags(write=False)
        _BUILT[name] = (plan, n, start, want)
    return _BUILT[name]


# ------------------------------------------------------------------ refusals
REFUSAL_N = 64 + 4 * ROWS
BAD_FIRST = 64 + 3 * ROWS   # the rows of the refused SHA job: free in every level
SHA_FIRST = (64, 64 + ROWS, 64 + 2 * ROWS)


def refusal_start():
    """zeros, and the cells of tests/test_u32_plan_emu.py at SOURCE_ROW: 2^32, 2, a non-canonical u32, 1, 16"""
    start = np.zeros((NW, REFUSAL_N), dtype=np.uint64)
    start[:5, SOURCE_ROW] = [1 << 32, 2, 41 + P, 1, 16]
    return start


def refusal_levels(bad=None, bad_level=1, bad_u32=None, bad_rec=False, bad_swap=False):
    """the three levels of test_u32_plan_emu.refusal_levels over rows 0..63 - u32 jobs, a rec job and a chain each - with a SHA job
    per level behind them (level 1 and 2 read the digest of the level before).  bad: a SHA item put into level `bad_level`; bad_u32 /
    bad_rec / bad_swap: a refused job of that family in level 1.  Returns (levels, the levels as they must come out)"""
    small, small_kept = small_refusal_levels(bad_u32, bad_rec=bad_rec, bad_swap=bad_swap)
    rng = np.random.default_rng(81)
    sha = [[(SHA_FIRST[0], imms(words(rng)))], [(SHA_FIRST[1], digest_cells(SHA_FIRST[0]) + imms(words(rng)[:8]))],
           [(SHA_FIRST[2], imms(words(rng)[:8]) + digest_cells(SHA_FIRST[1]))]]
    levels = [(list(sha[l]) + ([bad] if bad is not None and l == bad_level else []),) + tuple(small[l]) for l in range(3)]
    written = len(small_kept) if bad is None else min(len(small_kept), bad_level + 1)   # the levels up to the first refusal
    return levels, [(list(sha[l]),) + tuple(small_kept[l]) for l in range(written)]


def reason_cases(by_cell=False):
    """{reason code: (the SHA item, what to patch in the packed job: {field: value})}; by_cell: the value reason through a CELL, which
    only the device sees"""
    g = rg()
    ok = imms(range(16))
    at = lambda k, o: ok[:k] + [o] + ok[k + 1:]   # noqa: E731
    return {1: ((REFUSAL_N - ROWS + 1, ok), {}), 2: ((BAD_FIRST, ok), {"first_operand": None}), 3: ((BAD_FIRST, at(15, g.PREV(0))), {}),
            4: ((BAD_FIRST, at(0, g.CELL(0, NW))), {}), 5: ((BAD_FIRST, at(7, g.CELL(REFUSAL_N, 0))), {}),
            6: ((BAD_FIRST, at(9, g.CELL(SOURCE_ROW, 0) if by_cell else g.IMM(1 << 32))), {})}


def index_of_sha(plan, first_row):
    hit = [i for i, j in enumerate(plan.sha_jobs) if int(j["first_row"]) == first_row]
    assert len(hit) == 1
    return hit[0]


def refused_plan(code, by_cell=False, bad_level=1):
    """(the packed plan with reason `code` in one SHA job of level `bad_level`, that job's index, the plan as it must come out)"""
    item, patch = reason_cases(by_cell)[code]
    levels, kept = refusal_levels(item, bad_level=bad_level)
    plan = sp().pack_sha_plan(levels)
    at = index_of_sha(plan, item[0])
    for field, value in patch.items():
        plan.sha_jobs[at][field] = plan.operands.size - 15 if value is None else value
    return plan, at, sp().pack_sha_plan(kept)


LISTS = ("sha_jobs", "u32_jobs", "rec_jobs", "pos_jobs", "chain_ends", "operands")
ENDS = ("sha_level_ends", "u32_level_ends", "rec_level_ends", "pos_level_ends")


def plan_struct(m, plan, counts=None):
    """(the ctypes lcp2_witness_plan_sha over the host arrays, the arrays kept alive)"""
    keep = {name: np.ascontiguousarray(getattr(plan, name)) for name in LISTS + ENDS}
    ptr = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    c, k, b = counts or {}, keep, m.binding
    base = b.WitnessPlan(ptr(k["rec_jobs"]), c.get("nrec", k["rec_jobs"].size), ptr(k["rec_level_ends"]), ptr(k["pos_jobs"]),
                         c.get("npos", k["pos_jobs"].size), ptr(k["chain_ends"]), c.get("nchains", k["chain_ends"].size), ptr(k["pos_level_ends"]),
                         ptr(k["operands"]), c.get("noperands", k["operands"].size), c.get("nlevels", k["sha_level_ends"].size))
    mid = b.WitnessPlanU32(base, ptr(k["u32_jobs"]), c.get("nu32", k["u32_jobs"].size), ptr(k["u32_level_ends"]))
    return b.WitnessPlanSha(mid, ptr(k["sha_jobs"]), c.get("nsha", k["sha_jobs"].size), ptr(k["sha_level_ends"])), keep
