#!/usr/bin/env python3
"""lcp2_rec_gate_rows as a workload: recursion_gates.chain_plan over 2^bits rows in `levels` levels (about 2^16 jobs at the defaults),
run from a zero matrix with host lists (validation and upload included) and with lists already in HBM, the result compared with the
Python-integer matrix.  Prints ONE JSON line and writes it to profiles/rec_rows_probe.json, with the host time the same plan needs
in Python integers (recursion_gates.run_plan) and in C++ (csrc/rec_rows.hpp compiled for the CPU, one thread: tests/emu/emu_plan.cpp).
    python3 tools/rec_rows_probe.py 16 8 5"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # rows_lib: the builder of the CPU emulations


def host_cpp_ms(plan, n, reps):
    """the plan through rec_rows.hpp on one host thread, level by level as the witness plan without chains it is (best of reps), and
    whether it gives the expected matrix and refuses nothing"""
    import rows_lib
    E, levels = rows_lib.emu_plan(), rows_lib.rec_plan(plan.jobs, plan.operands, plan.level_ends)
    best, same = None, True
    for _ in range(reps):
        t0 = time.perf_counter()
        got, flags = rows_lib.run_levels(E, levels, n, threads=256)
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
        same = same and rows_lib.refusal(E, flags, levels) is None and bool((got == plan.expected).all())
    return 1e3 * best, same


def measure(ctx, bits=16, levels=8, reps=5, seed=3):
    import numpy as np
    import torch
    from eth_lc_plonky2_amd import recursion_gates as rg
    n = 1 << bits
    t0 = time.perf_counter()
    plan = rg.chain_plan(n, seed, levels=levels)   # (its expected matrix is run_plan over the packed lists)
    t_plan = time.perf_counter() - t0
    t0 = time.perf_counter()
    rg.run_plan(plan.jobs, plan.operands, plan.level_ends, 135, n)
    ms_python = 1e3 * (time.perf_counter() - t0)
    ms_cpp, cpp_same = host_cpp_ms(plan, n, reps)
    cells = sum(len(rg.job_columns(int(k), int(o))) for k, o in zip(plan.jobs["kind"], plan.jobs["op"]))

    want = torch.from_numpy(plan.expected.view(np.int64)).cuda()
    w = torch.zeros_like(want)
    d_jobs = torch.from_numpy(plan.jobs.view(np.int64)).cuda()
    d_ops = torch.from_numpy(plan.operands.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def timed(call):
        best = None
        for _ in range(reps):
            w.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()   # synchronises the context's stream before it returns
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return 1e3 * best

    ms_host = timed(lambda: ctx.rec_gate_rows(plan.jobs, plan.operands, plan.level_ends, w.data_ptr(), 135, n))
    same = bool(torch.equal(w, want))
    ms_device = timed(lambda: ctx.rec_gate_rows(d_jobs.data_ptr(), d_ops.data_ptr(), plan.level_ends, w.data_ptr(), 135, n,
                                                njobs=plan.jobs.size, noperands=plan.operands.size))
    same = same and bool(torch.equal(w, want))
    return {"workload": "lcp2_rec_gate_rows on recursion_gates.chain_plan(2^%d, levels=%d): every level one job of each of the ten kinds per "
                        "group of ten rows (ARITHMETIC 4, RANDOM_ACCESS 2), operands of the later levels CELL references into the level before; "
                        "from a zero matrix, lists sorted by (kind, op, row) inside a level" % (bits, levels),
            "rows": n, "levels": int(plan.level_ends.size), "jobs": int(plan.jobs.size), "operands": int(plan.operands.size),
            "list_bytes": int(plan.jobs.nbytes + plan.operands.nbytes), "cells_written": int(cells),
            "ms_host_lists_validation_and_upload_included": round(ms_host, 3), "ms_resident_lists": round(ms_device, 3),
            "ms_host_lists_minus_resident_lists": round(ms_host - ms_device, 3),
            "matrix_equals_python_integers": same,
            "ms_host_python_run_plan_one_thread": round(ms_python, 1), "ms_host_cpp_rec_rows_hpp_one_thread": round(ms_cpp, 3),
            "host_cpp_matrix_equals_python_integers": cpp_same, "ms_chain_plan_build_and_expected": round(1e3 * t_plan, 1), "best_of": reps}


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bits = int(args[0]) if args else 16
    levels = int(args[1]) if len(args) > 1 else 8
    reps = int(args[2]) if len(args) > 2 else 5
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    line = json.dumps(measure(ctx, bits, levels, reps))
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rec_rows_probe.json"), "w") as f:
        f.write(line + "\n")
