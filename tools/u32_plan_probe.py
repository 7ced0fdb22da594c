#!/usr/bin/env python3
"""Filling the plonky2_u32 / comparison rows of the reference's gate mix (u32_gates.ReferenceMix: of every 16 rows 6 U32AddMany in
pairs - the second row's first addends are the first row's results - 2 U32Arithmetic, 1 U32RangeCheck, 1 U32Subtraction,
1 Comparison) at 2^18 and 2^22 rows, three ways:
  (a) the numpy fillers of u32_gates.py on the host (ReferenceMix.fill), one run
  (b) lcp2_u32_gate_rows from a device list of precomputed immediate jobs (u32_gates.witness_jobs of the filled matrix)
  (c) lcp2_witness_plan_rows_u32 from a device plan of two levels whose non-leaf operands are CELLs: level 1 holds the second rows
      of the U32AddMany pairs, their addend_0 the CELL of the first row's output_result; every other operand is an IMM leaf
(b) and (c) from a zero matrix, `warmup` untimed calls and then `reps` timed ones (wall clock around the call, which synchronises the
context's stream before it returns; the device is idle before it starts), median and minimum; the three matrices must be equal.
`--only-b` measures (b) alone: what a tree without the new call can run.  Prints ONE JSON line; the full run writes it to
profiles/u32_plan.json.
    python3 tools/u32_plan_probe.py [--only-b] [reps [warmup]]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NW = 135


def mix_rows(n, seed):
    """(wires [135][n] from the numpy fillers, gate_of_row, G, first / second rows of the U32AddMany pairs, seconds the fill took)"""
    import numpy as np
    from eth_lc_plonky2_amd import u32_gates as ug
    mix = ug.ReferenceMix()
    names = ["NoopGate"] + sorted(set(mix.PATTERN.values()))
    G = {name: k for k, name in enumerate(names)}
    gate_of_row = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    for r, name in mix.PATTERN.items():
        gate_of_row[rows % 16 == r] = G[name]
    wires = np.zeros((NW, n), dtype=np.uint64)
    pairs = []
    t0 = time.perf_counter()
    mix.fill(wires, gate_of_row, G, np.random.default_rng(seed), lambda second, c2, first, c1: pairs.append((second, first)))
    seconds = time.perf_counter() - t0
    return wires, gate_of_row, G, pairs[0][1], pairs[0][0], seconds


def plan_of(jobs, first, second, n):
    """the two-level plan of the immediate jobs `jobs` (sorted by (kind, op, row)): (u32_jobs, operands, u32_level_ends)"""
    import numpy as np
    from eth_lc_plonky2_amd.binding import PLAN_CELL, REC_OPERAND_DTYPE, U32_ADD_MANY, U32_PLAN_JOB_DTYPE, U32_PLAN_OPERANDS
    partner = np.full(n, -1, dtype=np.int64)
    partner[second] = first
    late = (jobs["kind"] == U32_ADD_MANY) & (partner[jobs["row"]] >= 0)
    ordered = np.concatenate([jobs[~late], jobs[late]])   # each level still sorted by (kind, op, row)
    count = np.array([U32_PLAN_OPERANDS[k] for k in range(5)], dtype=np.int64)[ordered["kind"]]
    start = np.cumsum(count) - count
    plan_jobs = np.zeros(ordered.size, dtype=U32_PLAN_JOB_DTYPE)
    for name in ("row", "kind", "op"):
        plan_jobs[name] = ordered[name]
    plan_jobs["first_operand"] = start
    job_of = np.repeat(np.arange(ordered.size), count)
    k = np.arange(job_of.size) - start[job_of]
    ops = np.zeros(job_of.size, dtype=REC_OPERAND_DTYPE)
    ops["v"] = ordered["in"][job_of, k]
    level1 = int((~late).sum())
    cells = start[level1:]   # operand 0 of every job of level 1
    ops["v"][cells], ops["col"][cells], ops["src"][cells] = partner[ordered["row"][level1:]], 6 * ordered["op"][level1:].astype(np.int64) + 4, PLAN_CELL
    return plan_jobs, ops, np.array([level1, ordered.size], dtype=np.uint32)


def measure_size(ctx, degree_bits, reps, warmup, only_b, seed=5):
    import numpy as np
    import torch
    from eth_lc_plonky2_amd import u32_gates as ug
    n = 1 << degree_bits
    wires, gate_of_row, G, first, second, fill_seconds = mix_rows(n, seed)
    jobs = ug.witness_jobs(wires, gate_of_row, G)
    want = torch.from_numpy(wires.view(np.int64)).cuda()
    del wires
    w = torch.zeros_like(want)

    def resident(records):
        raw = np.ascontiguousarray(records).tobytes()
        return torch.from_numpy(np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype=np.int64).copy()).cuda()

    def timed(call):
        times = []
        for i in range(warmup + reps):
            w.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()   # synchronises the context's stream before it returns
            if i >= warmup:
                times.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(times), 3), round(min(times), 3)

    d_jobs = resident(jobs)
    b_median, b_min = timed(lambda: ctx.u32_gate_rows(d_jobs.data_ptr(), w.data_ptr(), n, njobs=jobs.size))
    out = {"degree_bits": degree_bits, "u32_rows": int((gate_of_row > 0).sum()), "jobs": int(jobs.size), "job_list_bytes": int(jobs.nbytes),
           "b_u32_gate_rows_ms_median": b_median, "b_u32_gate_rows_ms_min": b_min, "b_matrix_equals_numpy": bool(torch.equal(w, want))}
    if only_b:
        return out
    plan_jobs, ops, ends = plan_of(jobs, first, second, n)
    del d_jobs
    d_plan, d_ops = resident(plan_jobs), resident(ops)
    zeros = np.zeros(2, dtype=np.uint32)
    c_median, c_min = timed(lambda: ctx.witness_plan_rows_u32(d_plan.data_ptr(), 0, 0, 0, d_ops.data_ptr(), ends, zeros, zeros, w.data_ptr(), NW, n,
                                                              nu32=plan_jobs.size, nrec=0, npos=0, nchains=0, noperands=ops.size))
    out.update({"a_numpy_fillers_ms": round(1e3 * fill_seconds, 1), "plan_bytes": int(plan_jobs.nbytes + ops.nbytes), "operands": int(ops.size),
                "cell_operands": int((ops["src"] == 1).sum()), "level_ends": ends.tolist(), "c_plan_rows_u32_ms_median": c_median,
                "c_plan_rows_u32_ms_min": c_min, "c_over_b": round(c_median / b_median, 3), "c_matrix_equals_numpy": bool(torch.equal(w, want))})
    return out


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    only_b = "--only-b" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps, warmup = (int(args[0]) if args else 10), (int(args[1]) if len(args) > 1 else 3)
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    sizes = [measure_size(ctx, db, reps, warmup, only_b) for db in (18, 22)]
    line = json.dumps({"workload": "the u32 / comparison rows of the reference's gate mix filled from a zero matrix: (a) numpy fillers, (b) lcp2_u32_gate_rows "
                                   "from resident immediate jobs, (c) lcp2_witness_plan_rows_u32 from a resident two-level plan",
                       "reps": reps, "warmup": warmup, "only_b": only_b, "sizes": sizes})
    print(line)
    if not only_b:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "u32_plan.json"), "w") as f:
            f.write(line + "\n")
