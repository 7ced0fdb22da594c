#!/usr/bin/env python3
"""Filling SHA-256 rows (310 per two_to_one_sha256, columns 0..107) in a device-resident matrix [135][n], three ways:
  (a) lcp2_sha256_witness with host jobs and host words_in, no digests copied back: the existing call, the yardstick
  (b) lcp2_witness_plan_rows_sha with host lists (validated on the host, staged through the pinned buffer)
  (c) lcp2_witness_plan_rows_sha with the lists resident in HBM (validated by the kernel)
on three shapes: 2^12 independent hashes in one level, a Merkle tree of height 12 (4 095 hashes in 12 levels, the parents' words the
digests of their children: record sources for (a), digest CELLs for (b) and (c)), and 2^16 independent hashes in one level.
`warmup` untimed calls and then `reps` timed ones (wall clock around the call, which synchronises the context's stream before it
returns; the device is idle before it starts), median and minimum; the matrices of (a) and (c) must be equal.  Prints ONE JSON line
and writes it to profiles/sha_plan.json.
    python3 tools/sha_plan_probe.py [reps [warmup]]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NW, ROWS = 135, 310


def shape_lists(level_sizes, seed):
    """hashes in levels of `level_sizes`; level 0 reads 16 leaf words each, a hash k of a later level the digests of hashes 2k and
    2k + 1 of the level before.  Returns (sha256_witness jobs, level_start, words_in, plan jobs, operands, sha_level_ends), hash j
    on rows 310 j .."""
    import numpy as np
    from eth_lc_plonky2_amd.binding import PLAN_CELL, REC_OPERAND_DTYPE, SHA_JOB_DTYPE, SHA_PLAN_JOB_DTYPE
    total = sum(level_sizes)
    words = np.random.default_rng(seed).integers(0, 1 << 32, size=16 * level_sizes[0], dtype=np.uint64).astype(np.uint32)
    first_row = ROWS * np.arange(total, dtype=np.int64)
    jobs = np.zeros(total, dtype=SHA_JOB_DTYPE)
    jobs["first_row"] = first_row
    plan_jobs = np.zeros(total, dtype=SHA_PLAN_JOB_DTYPE)
    plan_jobs["first_row"], plan_jobs["first_operand"] = first_row, 16 * np.arange(total)
    ops = np.zeros(16 * total, dtype=REC_OPERAND_DTYPE)
    jobs["in_src"][:level_sizes[0]] = np.arange(16 * level_sizes[0]).reshape(-1, 16)
    ops["v"][:16 * level_sizes[0]] = words
    word = np.arange(16) % 8
    below, at = 0, level_sizes[0]
    for size in level_sizes[1:]:
        child = below + 2 * np.arange(size)[:, None] + (np.arange(16) // 8)[None, :]   # [size][16]: the hash whose digest word it is
        jobs["in_src"][at:at + size] = -1 - (8 * child + word[None, :])
        mine = ops[16 * at:16 * (at + size)]
        mine["v"], mine["col"], mine["src"] = (ROWS * child + 307 + word[None, :] // 3).ravel(), np.tile(3 * (word % 3) + 2, size), PLAN_CELL
        below, at = at, at + size
    starts = np.concatenate([[0], np.cumsum(level_sizes)]).astype(np.uint32)
    return jobs, starts, words, plan_jobs, ops, starts[1:].copy()


def measure_shape(ctx, name, level_sizes, reps, warmup, seed=9):
    import numpy as np
    import torch
    jobs, starts, words, plan_jobs, ops, ends = shape_lists(level_sizes, seed)
    total = int(jobs.size)
    n = ROWS * total
    w = torch.zeros((NW, n), dtype=torch.int64, device="cuda")
    none32, zeros = np.zeros(0, dtype=np.uint32), np.zeros(len(level_sizes), dtype=np.uint32)
    from eth_lc_plonky2_amd.binding import POS_JOB_DTYPE, REC_JOB_DTYPE
    no_rec, no_pos = np.zeros(0, dtype=REC_JOB_DTYPE), np.zeros(0, dtype=POS_JOB_DTYPE)

    def resident(records):
        raw = np.ascontiguousarray(records).tobytes()
        return torch.from_numpy(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.int64).copy()).cuda()

    def timed(call):
        times = []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()   # synchronises the context's stream before it returns
            if i >= warmup:
                times.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)

    a = timed(lambda: ctx.sha256_witness(jobs, starts, words, w.data_ptr(), n, digests=False))
    reference = w[:108].clone()
    w.zero_()
    b = timed(lambda: ctx.witness_plan_rows_sha(plan_jobs, no_rec, no_rec, no_pos, none32, ops, ends, zeros, zeros, zeros, w.data_ptr(), NW, n))
    b_equal = bool(torch.equal(w[:108], reference))
    w.zero_()
    d_jobs, d_ops = resident(plan_jobs), resident(ops)
    c = timed(lambda: ctx.witness_plan_rows_sha(d_jobs.data_ptr(), 0, 0, 0, 0, d_ops.data_ptr(), ends, zeros, zeros, zeros, w.data_ptr(), NW, n,
                                                nsha=total, nu32=0, nrec=0, npos=0, nchains=0, noperands=ops.size))
    c_equal = bool(torch.equal(w[:108], reference)) and not bool(w[108:].any())
    out = {"shape": name, "hashes": total, "levels": len(level_sizes), "rows": n, "bytes_written": 8 * 108 * n}
    for key, (median, low, high) in (("a_sha256_witness_host_jobs", a), ("b_plan_rows_sha_host_lists", b), ("c_plan_rows_sha_device_lists", c)):
        out.update({key + "_ms_median": median, key + "_ms_min": low, key + "_ms_max": high})
    out.update({"b_over_a": round(b[0] / a[0], 3), "c_over_a": round(c[0] / a[0], 3), "b_matrix_equals_a": b_equal, "c_matrix_equals_a": c_equal})
    return out


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps, warmup = (int(args[0]) if args else 10), (int(args[1]) if len(args) > 1 else 3)
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    shapes = [("flat_2p12", [1 << 12]), ("tree_height_12", [1 << k for k in range(11, -1, -1)]), ("flat_2p16", [1 << 16])]
    sizes = [measure_shape(ctx, name, levels, reps, warmup) for name, levels in shapes]
    line = json.dumps({"workload": "SHA-256 rows filled in a resident matrix [135][310 x hashes]: (a) lcp2_sha256_witness with host jobs, (b) "
                                   "lcp2_witness_plan_rows_sha with host lists, (c) the same with lists in HBM",
                       "reps": reps, "warmup": warmup, "sizes": sizes})
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sha_plan.json"), "w") as f:
        f.write(line + "\n")
