"""lcp2_sha256_witness and lcp2_scatter_cells: the 310 rows of every two_to_one_sha256 filled on the device, level by level, and the
scattered cells beside them.

The reference is tests/sha_rows_ref.py, a model over Python integers that shares nothing with csrc/.  Without a GPU it is pinned to
hashlib and to the gates' own constraint programs (host/gates.cpp through tests/emu/dump_host_gates.cpp and gate_program_ref.py;
booleanity and the sum equations leave one value for every carry, so satisfied constraints plus the chaining of a plain SHA-256 fix
the whole matrix), and csrc/sha_rows.hpp - the lanes of k_sha_jobs_level / k_sha_fill_rows with their grids as loops, and the
validation of the entry point - runs on the CPU (tests/emu/emu_sha.cpp) against it.  On the GPU the same cases go through the
library, with the staging cases on top.  A matrix is [135][n] and full of a sentinel before every call: afterwards columns 0..107
of the rows a job owns equal the model, zeros included, and every other cell still holds the sentinel."""
import ctypes
import hashlib
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import gate_program_ref
import sha_rows_ref as ref

from rows_lib import HERE, INVALID, NW, ROOT, build_emu

HOST = os.path.join(ROOT, "eth-lc-plonky2_amd", "host")
SENTINEL = 0xA5A5A5A5A5A5A5A5
M32 = 0xFFFFFFFF
PIN_BYTES = 4 << 20   # lcp2_ctx::PIN_BYTES (csrc/internal.hpp)
T_COVER, T_MONOTONE, T_ROWS, T_SOURCE = ("sha witness: level table does not cover the jobs", "sha witness: level table not monotone",
                                         "sha witness: rows out of range", "sha witness: bad message source")
SPECIAL = ([0] * 16, [M32] * 16, [0x80000000] * 16)
CARRY_RANGES = {"schedule": range(4), "round_e": range(5), "e_new": range(2), "round_a": range(3), "add": range(2)}


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


@pytest.fixture(scope="module")
def emus():
    """tests/emu/libemu_sha.so"""
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_sha", (("emu_sha_job_bytes", c.c_uint, []), ("emu_sha_cell_bytes", c.c_uint, []), ("emu_sha_rows", c.c_uint, []),
                                 ("emu_sha_row_columns", c.c_uint, []), ("emu_sha_problem_str", c.c_char_p, [c.c_uint]),
                                 ("emu_sha_jobs_problem", c.c_uint, [V, U, V, c.c_uint, U, U, V]),
                                 ("emu_sha256_witness", c.c_uint, [V, U, V, c.c_uint, V, U, V, U, V]), ("emu_scatter_cells", c.c_uint, [V, U, V, U])))


@pytest.fixture(scope="module")
def programs():
    """{gate name: (code words, immediates)} of build_gate_set(9), through the dump program"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "dump_host_gates")
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "emu", "dump_host_gates.cpp"), os.path.join(HOST, "gates.cpp"),
                        os.path.join(HOST, "poseidon_host.cpp")], check=True, cwd=ROOT)
        text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    out, imm = {}, None
    for line in text.splitlines():
        tok = line.split()
        if tok[0] == "gateset":
            imm = [int(v, 16) for v in tok[3:3 + int(tok[2], 16)]]
        elif tok[0] == "gate":
            m, length = int(tok[3], 16), int(tok[4], 16)
            words = [int(v, 16) for v in tok[5:]]
            assert len(words) == 2 * length
            out[tok[1]] = (words, imm, m)
    assert {g: out[g][2] for g in (ref.GATE_SCHEDULE, ref.GATE_ROUND_E, ref.GATE_ROUND_A, ref.GATE_ADD)} == {
        ref.GATE_SCHEDULE: 64 + 2 + 1 + 2, ref.GATE_ROUND_E: 96 + 3 + 1 + 3 + 1 + 1, ref.GATE_ROUND_A: 96 + 3 + 1 + 2, ref.GATE_ADD: 3 * 35}
    return out


# ------------------------------------------------------------------ the model's rows, computed once per message
_ROWS = {}


def model_rows(words16):
    """[108][310] u64 of one message (cached: the CPU and the GPU tests share it, nobody writes to it)"""
    key = tuple(int(x) for x in words16)
    if key not in _ROWS:
        a = np.array(ref.expected_rows(key), dtype=np.uint64).T.copy()
        a.setflags(write=False)
        _ROWS[key] = a
    return _ROWS[key]


def make_jobs(items):
    import eth_lc_plonky2_amd as m
    jobs = np.zeros(len(items), dtype=m.binding.SHA_JOB_DTYPE)
    for i, (first_row, src) in enumerate(items):
        jobs[i]["first_row"], jobs[i]["in_src"] = first_row, src
    return jobs


def make_cells(items):
    import eth_lc_plonky2_amd as m
    cells = np.zeros(len(items), dtype=m.binding.CELL_DTYPE)
    for i, (row, col, value) in enumerate(items):
        cells[i]["row"], cells[i]["col"], cells[i]["value"] = row, col, value
    return cells


def digest_src(job, word):
    return -1 - (8 * job + word)


def scattered_rows(rng, njobs, n):
    """first rows of njobs blocks of 310 rows in [0, n): not in row order (njobs > 1), the slack spread as gaps in front of blocks,
    the last block flush against row n"""
    slack = n - 310 * njobs
    assert slack >= 0
    gaps = np.bincount(rng.integers(0, njobs, size=slack), minlength=njobs)
    starts = np.cumsum(gaps) + 310 * np.arange(njobs)
    assert starts[-1] + 310 == n
    order = rng.permutation(njobs)
    if njobs > 1 and (order == np.arange(njobs)).all():
        order = order[::-1]
    return [int(starts[k]) for k in order]


def counts_messages(njobs):
    rng = np.random.default_rng(1000 + njobs)
    msgs = [[int(x) for x in rng.integers(0, 1 << 32, size=16)] for _ in range(njobs)]
    if njobs == 1:
        msgs[0] = SPECIAL[2]
    elif njobs == 2:
        msgs[0], msgs[1] = SPECIAL[0], SPECIAL[1]
    else:
        msgs[1], msgs[njobs // 2], msgs[njobs - 1] = SPECIAL
    return msgs


def level0_case(msgs, n, seed):
    """all jobs in level 0; the words of every message scattered over words_in"""
    rng = np.random.default_rng(seed)
    njobs = len(msgs)
    slots = rng.permutation(16 * njobs)
    words = np.zeros(16 * njobs, dtype=np.uint32)
    items = []
    for j, (first, msg) in enumerate(zip(scattered_rows(rng, njobs, n), msgs)):
        src = [int(s) for s in slots[16 * j:16 * j + 16]]
        words[src] = msg
        items.append((first, src))
    return dict(items=items, levels=[0, njobs], words=words, n=n)


def counts_case(njobs):
    return level0_case(counts_messages(njobs), 310 * njobs + 7, 2000 + njobs)


def merkle_case():
    """a SHA-256 Merkle tree of height 4: 16 leaves of 8 words, 15 jobs in 4 levels; the last job's digest is the root"""
    rng = np.random.default_rng(31)
    words = rng.integers(0, 1 << 32, size=128, dtype=np.uint32)
    n = 310 * 15 + 5
    rows = scattered_rows(rng, 15, n)
    items, levels, below = [], [0], None
    for width in (8, 4, 2, 1):
        base = len(items)
        for k in range(width):
            if below is None:
                src = list(range(16 * k, 16 * k + 16))
            else:
                src = [digest_src(below + 2 * k + side, w) for side in (0, 1) for w in range(8)]
            items.append((rows[len(items)], src))
        below = base
        levels.append(len(items))
    return dict(items=items, levels=levels, words=words, n=n)


def two_wide_levels_case():
    """70 jobs behind 70: the second launch of k_sha_jobs_level has first != 0 and crosses a 64-lane block"""
    rng = np.random.default_rng(32)
    words = rng.integers(0, 1 << 32, size=16 * 70, dtype=np.uint32)
    n = 310 * 140 + 3
    rows = scattered_rows(rng, 140, n)
    items = [(rows[j], list(range(16 * j, 16 * j + 16))) for j in range(70)]
    for k in range(70):
        items.append((rows[70 + k], [digest_src(k, w) for w in range(8)] + [digest_src((k + 33) % 70, 7 - w) for w in range(8)]))
    return dict(items=items, levels=[0, 70, 140], words=words, n=n)


def mixed_sources_case():
    """job 3 (level 3) takes words of words_in, digest words of the level before, of two and of three levels back, one of them twice;
    job 4 shares its level"""
    rng = np.random.default_rng(33)
    words = rng.integers(0, 1 << 32, size=40, dtype=np.uint32)
    n = 310 * 5 + 11
    rows = scattered_rows(rng, 5, n)
    items = [(rows[0], list(range(16))),
             (rows[1], [digest_src(0, w) for w in range(8)] + list(range(16, 24))),
             (rows[2], [digest_src(1, 7 - w) for w in range(8)] + [digest_src(0, w) for w in range(8)]),
             (rows[3], [39, digest_src(2, 0), digest_src(1, 5), digest_src(0, 7), digest_src(0, 7), 24, digest_src(1, 5), digest_src(2, 7),
                        digest_src(0, 0), 25, 25, digest_src(1, 0), digest_src(2, 3), 0, digest_src(0, 3), 38]),
             (rows[4], [digest_src(0, w) for w in range(8)] + [digest_src(2, w) for w in range(8)])]
    return dict(items=items, levels=[0, 1, 2, 3, 5], words=words, n=n)


def empty_level_case():
    """level_start repeated in the middle: level 1 is empty, level 2 reads level 0"""
    rng = np.random.default_rng(34)
    words = rng.integers(0, 1 << 32, size=32, dtype=np.uint32)
    n = 310 * 3 + 2
    rows = scattered_rows(rng, 3, n)
    items = [(rows[0], list(range(16))), (rows[1], list(range(16, 32))),
             (rows[2], [digest_src(1, w) for w in range(8)] + [digest_src(0, w) for w in range(8)])]
    return dict(items=items, levels=[0, 2, 2, 3], words=words, n=n)


CASES = {"njobs1": lambda: counts_case(1), "njobs2": lambda: counts_case(2), "njobs63": lambda: counts_case(63), "njobs64": lambda: counts_case(64),
         "njobs65": lambda: counts_case(65), "njobs130": lambda: counts_case(130),
         "one_job_n310": lambda: level0_case([[int(x) for x in np.random.default_rng(5).integers(0, 1 << 32, size=16)]], 310, 6),
         "merkle_height4": merkle_case, "levels_70_behind_70": two_wide_levels_case, "mixed_sources": mixed_sources_case,
         "empty_level": empty_level_case}


def expected_matrix(case):
    """([135][n] with the model's rows in a sea of sentinel, the model's digests)"""
    messages, digests = ref.resolve(case["items"], case["levels"], case["words"])
    want = np.full((NW, case["n"]), SENTINEL, dtype=np.uint64)
    for (first, _), msg in zip(case["items"], messages):
        want[:ref.COLUMNS, first:first + ref.ROWS] = model_rows(msg)
    return want, np.array(digests, dtype=np.uint32).reshape(-1, 8)


# ------------------------------------------------------------------ the two ways to run a call
class Emulation:
    """csrc/sha_rows.hpp on the CPU: (status, text, matrix, digests)"""

    def __init__(self, E):
        self.E = E

    def sha(self, jobs, levels, words, n, digests=True):
        levels, words = np.ascontiguousarray(levels, dtype=np.uint32), np.ascontiguousarray(words, dtype=np.uint32)
        m = np.full((NW, n), SENTINEL, dtype=np.uint64)
        d = np.zeros((jobs.size, 8), dtype=np.uint32) if digests else None
        problem = self.E.emu_sha256_witness(vp(jobs), jobs.size, vp(levels), max(levels.size, 1) - 1, vp(words), words.size, vp(m), n, vp(d))
        return (INVALID if problem else 0), self.E.emu_sha_problem_str(problem).decode(), m, d

    def scatter(self, cells, n, columns=NW):
        m = np.full((columns, n), SENTINEL, dtype=np.uint64)
        problem = self.E.emu_scatter_cells(vp(cells), cells.size, vp(m), n)
        return (INVALID if problem else 0), "scatter: row out of range" if problem else "", m


class Device:
    """the library on the GPU, through Context.sha256_witness / Context.scatter_cells"""

    def __init__(self, ctx):
        self.ctx = ctx

    def _call(self, n, columns, fn):
        import eth_lc_plonky2_amd as m
        ptr = self.ctx.buffer_alloc(columns * n)
        try:
            self.ctx.buffer_write(ptr, np.full((columns, n), SENTINEL, dtype=np.uint64))
            status, text, out = 0, "", None
            try:
                out = fn(ptr)
            except m.Lcp2Error as e:
                status, text = e.status, str(e)
            return status, text, self.ctx.buffer_read(ptr, columns * n).reshape(columns, n), out
        finally:
            self.ctx.buffer_free(ptr)

    def sha(self, jobs, levels, words, n, digests=True):
        return self._call(n, NW, lambda ptr: self.ctx.sha256_witness(jobs, levels, words, ptr, n, digests=digests))

    def scatter(self, cells, n, columns=NW):
        return self._call(n, columns, lambda ptr: self.ctx.scatter_cells(cells, ptr, n))[:3]


def check_case(run, name):
    case = CASES[name]()
    want, want_digests = expected_matrix(case)
    status, text, got, digests = run.sha(make_jobs(case["items"]), case["levels"], case["words"], case["n"])
    assert status == 0, text
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing cell (column, row): %s" % bad[0]
    assert (digests == want_digests).all()
    if name == "merkle_height4":   # the root against hashlib, leaf bytes big-endian as SHA-256 reads them
        level = [struct.pack(">8I", *case["words"][8 * k:8 * k + 8]) for k in range(16)]
        while len(level) > 1:
            level = [hashlib.sha256(level[2 * k] + level[2 * k + 1]).digest() for k in range(len(level) // 2)]
        assert struct.pack(">8I", *digests[14]) == level[0]
    if name.startswith("njobs") or name == "one_job_n310":   # section a: a job ends on the last row, and the order is not the rows'
        firsts = [f for f, _ in case["items"]]
        assert max(firsts) + 310 == case["n"] and (len(firsts) == 1 or firsts != sorted(firsts))


# ------------------------------------------------------------------ the model, pinned without a GPU
def message_bytes(words16):
    return struct.pack(">16I", *words16)


def test_model_digest_is_hashlib():
    """the outputs of the last three addition rows (and digest_words) are SHA-256 of the 64-byte message"""
    rng = np.random.default_rng(11)
    for msg in list(SPECIAL) + [[int(x) for x in rng.integers(0, 1 << 32, size=16)] for _ in range(20)]:
        rows = ref.expected_rows(msg)
        outs = [rows[307 + i // 3][3 * (i % 3) + 2] for i in range(8)]
        assert struct.pack(">8I", *outs) == hashlib.sha256(message_bytes(msg)).digest()
        assert ref.digest_words(msg) == outs
        mid = [rows[176 + i // 3][3 * (i % 3) + 2] for i in range(8)]   # the data block's additions feed the padding block's
        assert [rows[307 + i // 3][3 * (i % 3)] for i in range(8)] == mid


def violated(programs, rows, only=None):
    """[(row, constraint)] the gate programs do not find zero on a 310-row matrix of the model's layout"""
    out = []
    for lr, (gate, c0) in enumerate(ref.row_gates()):
        if only is not None and lr not in only:
            continue
        code, imm, m = programs[gate]
        emitted = gate_program_ref.emitted_constraints(code, imm, list(rows[lr]) + [0] * (NW - ref.COLUMNS), [c0, 0], [0] * 4)
        assert len(emitted) == m
        out += [(lr, k) for k, v in enumerate(emitted) if v]
    return out


def test_model_rows_satisfy_their_gates(programs):
    """every row of the model gives all-zero constraints under its gate's program, with K_t resp. K_t + W_pad_t as gate constant 0"""
    rng = np.random.default_rng(12)
    for msg in list(SPECIAL) + [[int(x) for x in rng.integers(0, 1 << 32, size=16)] for _ in range(2)]:
        assert violated(programs, ref.expected_rows(msg)) == []
    assert max(c0 for _, c0 in ref.row_gates()) > M32   # some constant of the padding block does not fit 32 bits: not reduced


def test_constraint_check_rejects_single_cell_changes(programs):
    """the check above bites: one cell changed in a word, a decomposition bit, a carry of each of the four row kinds"""
    rows = ref.expected_rows([int(x) for x in np.random.default_rng(13).integers(0, 1 << 32, size=16)])
    sched, round_e, round_a, add, pad_e, pad_add = 5, 48 + 2 * 9, 48 + 2 * 9 + 1, 177, 179 + 2 * 20, 308
    changes = [(sched, 4), (round_e, 6), (round_e, 5), (round_a, 4), (add, 2), (pad_e, 7),          # words
               (sched, 8 + 3), (sched, 40 + 31), (round_e, 72), (round_a, 40 + 17), (add, 9 + 33 + 5), (pad_add, 9),   # decomposition bits
               (sched, 104), (sched, 105), (round_e, 104), (round_e, 106), (round_e, 107), (round_a, 104), (round_a, 105),
               (add, 9 + 32), (add, 9 + 33 + 32), (pad_add, 9 + 66 + 32), (pad_e, 105)]             # carries
    for lr, col in changes:
        v = rows[lr][col]
        for new in ((v + 1) & M32, v ^ 0x80000000) if col < 8 else (v ^ 1, ):
            changed = [list(r) for r in rows]
            changed[lr][col] = new
            assert violated(programs, changed, only={lr}), (lr, col, new)
    changed = [list(r) for r in rows]   # an unused cell may hold anything as far as the gates go: the model's zeros are the layout's word
    changed[sched][80] = 7
    assert violated(programs, changed, only={sched}) == []


def test_carries_take_every_value_over_the_count_cases():
    """over the messages of the njobs cases every carry field takes every value its sum allows (from the model alone)"""
    seen = {}
    for njobs in (1, 2, 63, 64, 65, 130):
        for msg in counts_messages(njobs):
            ref.expected_rows(msg, carries=seen)
    assert {k: sorted(v) for k, v in seen.items()} == {k: list(r) for k, r in CARRY_RANGES.items()}


# ------------------------------------------------------------------ csrc/sha_rows.hpp on the CPU
def test_harness_layout(emus):
    import eth_lc_plonky2_amd as m
    assert emus.emu_sha_job_bytes() == m.binding.SHA_JOB_DTYPE.itemsize and emus.emu_sha_cell_bytes() == m.binding.CELL_DTYPE.itemsize
    assert (emus.emu_sha_rows(), emus.emu_sha_row_columns()) == (ref.ROWS, ref.COLUMNS) == (m.binding.SHA_ROWS, m.binding.SHA_ROW_COLUMNS)


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_rows_equal_the_model(emus, name):
    check_case(Emulation(emus), name)


def check_without_digests(run):
    case = CASES["mixed_sources"]()
    status, text, got, digests = run.sha(make_jobs(case["items"]), case["levels"], case["words"], case["n"], digests=False)
    assert status == 0 and digests is None and (got == expected_matrix(case)[0]).all()


def test_emulated_rows_without_digests(emus):
    check_without_digests(Emulation(emus))


def refusals():
    """[(name, items, levels, nwords, n, text or None)]: lists the entry point refuses on the host, before any launch"""
    n = 310 * 4 + 40
    good = [(0, list(range(16))), (320, list(range(16, 32))), (n - 310, [digest_src(0, w) for w in range(8)] + [digest_src(1, w) for w in range(8)]),
            (640, list(range(16)))]

    def with_job(k, first=None, src=None):
        items = list(good)
        items[k] = (items[k][0] if first is None else first, list(items[k][1]) if src is None else src)
        return items

    def src_with(k, i, s):
        src = list(good[k][1])
        src[i] = s
        return src
    return [("first entry not 0", good, [1, 2, 4], 32, n, T_COVER),
            ("last entry not njobs", good, [0, 2, 3], 32, n, T_COVER),
            ("last entry above njobs", good, [0, 2, 5], 32, n, T_COVER),
            ("table not monotone", good, [0, 2, 1, 4], 32, n, T_MONOTONE),
            ("table entry above njobs", good, [0, 100, 2, 4], 32, n, T_MONOTONE),
            ("one row too far", with_job(3, first=n - 309), [0, 2, 4], 32, n, T_ROWS),
            ("first row at the end of u32", with_job(1, first=0xFFFFFFFF), [0, 2, 4], 32, n, T_ROWS),
            ("source == nwords", with_job(1, src=src_with(1, 15, 32)), [0, 2, 4], 32, n, T_SOURCE),
            ("source of the same level", with_job(2, src=src_with(2, 0, digest_src(3, 0))), [0, 2, 4], 32, n, T_SOURCE),
            ("source is the job itself", with_job(2, src=src_with(2, 9, digest_src(2, 1))), [0, 2, 4], 32, n, T_SOURCE),
            ("source of a later level", with_job(1, src=src_with(1, 3, digest_src(2, 0))), [0, 2, 4], 32, n, T_SOURCE),
            ("digest source in level 0", with_job(0, src=src_with(0, 0, digest_src(0, 0))), [0, 2, 4], 32, n, T_SOURCE),
            ("most negative source", with_job(2, src=src_with(2, 4, -(1 << 31))), [0, 2, 4], 32, n, T_SOURCE),
            ("no levels", good, [0], 32, n, None),
            ("no level table", good, [], 32, n, None)]


def check_refusals(run):
    for name, items, levels, nwords, n, text in refusals():
        status, said, got, _ = run.sha(make_jobs(items), levels, np.arange(nwords, dtype=np.uint32), n)
        assert status == INVALID, name
        if text is not None:
            assert said.endswith(text), (name, said)
        assert (got == SENTINEL).all(), name
    # no jobs: LCP2_OK, nothing written - with or without a level table
    for levels in ([0], [], [0, 0]):
        status, said, got, _ = run.sha(make_jobs([]), levels, np.arange(4, dtype=np.uint32), 64)
        assert status == 0 and (got == SENTINEL).all()
    # the list the refusals were cut from is good (and a call after refusals works)
    case = dict(items=refusals()[0][1], levels=[0, 2, 4], words=np.arange(32, dtype=np.uint32), n=refusals()[0][4])
    status, said, got, digests = run.sha(make_jobs(case["items"]), case["levels"], case["words"], case["n"])
    want, want_digests = expected_matrix(case)
    assert status == 0 and (got == want).all() and (digests == want_digests).all()


def test_emulated_refusals(emus):
    check_refusals(Emulation(emus))
    E = emus   # which job, and the two texts the entry point cannot reach
    jobs, levels, where = make_jobs(refusals()[5][1]), np.array([0, 2, 4], dtype=np.uint32), ctypes.c_uint(99)
    assert E.emu_sha_jobs_problem(vp(jobs), 4, vp(levels), 2, 32, refusals()[5][4], ctypes.byref(where)) == 3 and where.value == 3
    assert E.emu_sha_jobs_problem(vp(jobs), 4, vp(levels), 0, 32, 1 << 20, ctypes.byref(where)) == 5
    assert [E.emu_sha_problem_str(k).decode() for k in (1, 2, 3, 4)] == [T_COVER, T_MONOTONE, T_ROWS, T_SOURCE]


def check_scatter(run):
    n, rng = 300, np.random.default_rng(41)
    # 257 cells (two blocks of the kernel) on distinct places, a non-canonical value and the largest u64 among them, stored as given
    places = rng.permutation(NW * n)[:257]
    values = rng.integers(0, 1 << 64, size=257, dtype=np.uint64)
    values[0], values[255], values[256] = 0xFFFFFFFF00000001, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000000
    items = [(int(p % n), int(p // n), int(v)) for p, v in zip(places, values)]
    items[3] = (n - 1, NW - 1, 5)    # the last cell of the matrix
    items[4] = (0, 0, 6)
    want = np.full((NW, n), SENTINEL, dtype=np.uint64)
    for row, col, v in items:
        want[col, row] = v
    status, said, got = run.scatter(make_cells(items), n)
    assert status == 0 and (got == want).all()
    # no cells: LCP2_OK, nothing written
    status, said, got = run.scatter(make_cells([]), n)
    assert status == 0 and (got == SENTINEL).all()
    # row == n anywhere in the list: refused, nothing written (a column is not checked: the call does not know how many there are)
    for at in (0, 100, 256):
        bad = list(items)
        bad[at] = (n, 0, 1)
        status, said, got = run.scatter(make_cells(bad), n)
        assert status == INVALID and said.endswith("scatter: row out of range") and (got == SENTINEL).all()


def test_emulated_scatter(emus):
    check_scatter(Emulation(emus))


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_rows_equal_the_model(gpu_ctx, name):
    check_case(Device(gpu_ctx), name)


@pytest.mark.gpu
def test_device_digests_and_staging(gpu_ctx):
    """the same 65 jobs four ways - without digests, everything through the pinned staging buffer, words_in too long for it (the
    words go up from the caller's memory), and jobs + words filling it to within 1 KiB (the digests come back directly): identical
    rows and digests"""
    run, case = Device(gpu_ctx), CASES["njobs65"]()
    jobs, n = make_jobs(case["items"]), case["n"]
    want, want_digests = expected_matrix(case)
    staged_jobs = (jobs.nbytes + 63) & ~63
    assert staged_jobs + case["words"].nbytes + 65 * 32 < PIN_BYTES
    over = np.concatenate([case["words"], np.full(PIN_BYTES // 4, 0x5A5A5A5A, dtype=np.uint32)])   # past 4 MiB on its own
    brim = np.concatenate([case["words"], np.full((PIN_BYTES - staged_jobs - 512 - case["words"].nbytes) // 4, 0x5A5A5A5A, dtype=np.uint32)])
    assert brim.nbytes % 64 == 0 and 0 < PIN_BYTES - staged_jobs - brim.nbytes <= 1024 < 65 * 32
    for words, digests in ((case["words"], False), (case["words"], True), (over, True), (brim, True)):
        status, text, got, d = run.sha(jobs, case["levels"], words, n, digests=digests)
        assert status == 0, text
        assert (got == want).all()
        assert (d == want_digests).all() if digests else d is None


@pytest.mark.gpu
def test_device_refusals(gpu_ctx):
    check_refusals(Device(gpu_ctx))


@pytest.mark.gpu
def test_device_scatter(gpu_ctx):
    check_scatter(Device(gpu_ctx))
