"""SHA-256 jobs inside a witness plan (lcp2_witness_plan_rows_sha): where a hash's words live in the matrix, and the packer.

One two_to_one_sha256 is 310 rows of columns 0..107 (csrc/sha_layout.hpp).  Its 16 message words are operands of the plan - IMM or
CELL, as recursion_gates.IMM / CELL build them - and its digest is read back as cells, so hashes chain through the matrix:

    parent = (first_row, [CELL(*digest_cell(left, i)) for i in range(8)] + [CELL(*digest_cell(right, i)) for i in range(8)])
"""
from types import SimpleNamespace

import numpy as np

from .binding import SHA_PLAN_JOB_DTYPE, SHA_PLAN_OPERANDS

DIGEST_ROW, MESSAGE_ROW, MESSAGE_COLUMN = 307, 48, 5


def digest_cell(first_row, i):
    """(row, column) of digest word i (0..7) of the hash whose rows begin at first_row: output i of the last three addition rows"""
    assert 0 <= i < 8
    return int(first_row) + DIGEST_ROW + i // 3, 3 * (i % 3) + 2


def message_cell(first_row, t):
    """(row, column) of message word W_t (0..15) of the hash whose rows begin at first_row: wire w of the round E row of round t"""
    assert 0 <= t < 16
    return int(first_row) + MESSAGE_ROW + 2 * t, MESSAGE_COLUMN


def pack_sha_plan(levels):
    """levels: [(sha items, u32 items, rec items, chains), ..]: sha items [(first_row, [16 x IMM(..) / CELL(..)]), ..] in the order
    they are to be listed, the other three as in u32_gates.pack_u32_plan -> a namespace of the ten lists of lcp2_witness_plan_rows_sha:
    the eight of pack_u32_plan, sha_jobs (SHA_PLAN_JOB_DTYPE) and sha_level_ends.  The operands of the SHA jobs follow those of the
    other three families in the one list, in job order."""
    from . import u32_gates
    base = u32_gates.pack_u32_plan([(u32, rec, chains) for _, u32, rec, chains in levels])
    jobs = np.zeros(sum(len(sha) for sha, _, _, _ in levels), dtype=SHA_PLAN_JOB_DTYPE)
    ops = np.zeros(SHA_PLAN_OPERANDS * jobs.size, dtype=base.operands.dtype)
    k, ends = 0, []
    for sha, _, _, _ in levels:
        for first_row, operands in sha:
            assert len(operands) == SHA_PLAN_OPERANDS, len(operands)
            jobs[k] = (first_row, base.operands.size + SHA_PLAN_OPERANDS * k)
            for t, (v, col, src) in enumerate(operands):
                ops[SHA_PLAN_OPERANDS * k + t] = (v % (1 << 64), col, src)
            k += 1
        ends.append(k)
    return SimpleNamespace(sha_jobs=jobs, sha_level_ends=np.array(ends, dtype=np.uint32), u32_jobs=base.u32_jobs, u32_level_ends=base.u32_level_ends,
                           rec_jobs=base.rec_jobs, pos_jobs=base.pos_jobs, chain_ends=base.chain_ends, operands=np.concatenate([base.operands, ops]),
                           rec_level_ends=base.rec_level_ends, pos_level_ends=base.pos_level_ends)


def merkle_levels(leaves, first_rows):
    """The SHA items of a binary Merkle tree over `leaves` (2^h x 8 words: 2^(h-1) bottom hashes of two leaves each), level by level
    from the bottom: [[(first_row, operands), ..], ..] with the parents' words the digest cells of their children.  first_rows: one
    first row per hash, bottom level first (2^h - 1 of them)."""
    from .recursion_gates import CELL, IMM
    leaves = np.asarray(leaves).reshape(-1, 8)
    width = leaves.shape[0] // 2
    assert width >= 1 and width & (width - 1) == 0 and len(first_rows) == 2 * width - 1
    rows = [int(r) for r in first_rows]
    level = [(rows[j], [IMM(w) for w in leaves[2 * j]] + [IMM(w) for w in leaves[2 * j + 1]]) for j in range(width)]
    out, at = [level], width
    while width > 1:
        below, width = out[-1], width // 2
        level = [(rows[at + j], [CELL(*digest_cell(below[2 * j + side][0], i)) for side in (0, 1) for i in range(8)]) for j in range(width)]
        out.append(level)
        at += width
    return out
