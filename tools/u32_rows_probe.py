#!/usr/bin/env python3
"""lcp2_u32_gate_rows as a workload: u32_gates.reference_mix_circuit at 2^bits rows, the U32AddMany / U32Arithmetic /
U32Subtraction / U32RangeCheck / Comparison rows of a device copy of its witness zeroed and refilled with ONE call - from the host
job list (validation and upload included) and from a list already in HBM - the refilled matrix compared with the host witness on the
device, one proof from it, verified.  Prints ONE JSON line with the times of the call and of the numpy fillers (u32_gates.fill_*) that
write the same rows on the host.
    python3 tools/u32_rows_probe.py 22 3"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(ctx, degree_bits=22, reps=3, seed=3):
    import numpy as np
    import torch
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import u32_gates as ug
    params = m.standard_params(degree_bits, 5)
    circ, wires, pis = ug.reference_mix_circuit(params, seed=seed, small_values=True)
    n, nw = circ.n, params.num_wires
    gate_of_row, G = ug.gate_rows(circ)
    t0 = time.perf_counter()
    jobs = ug.witness_jobs(wires, gate_of_row, G)
    t_jobs = time.perf_counter() - t0
    rows_of = {kind: np.nonzero(gate_of_row == G[name])[0] for kind, (name, _, _) in ug.U32_JOB_KINDS.items()}
    cells = sum(rows_of[kind].size * len(ug.job_columns(kind, op)) for kind, (_, ops, _) in ug.U32_JOB_KINDS.items() for op in range(ops))

    # the device matrix, and what the refill must give: the host witness with the cells no job owns on those rows at zero
    w = torch.from_numpy(wires.view(np.int64)).cuda()
    want = w.clone()
    for kind, (_, ops, _) in ug.U32_JOB_KINDS.items():
        rows = torch.from_numpy(rows_of[kind]).cuda()
        owned = sorted(c for op in range(ops) for c in ug.job_columns(kind, op))
        rest = torch.tensor([c for c in range(nw) if c not in owned], device="cuda")
        want[rest[:, None], rows[None, :]] = 0
        w[:, rows] = 0
    d_jobs = torch.from_numpy(jobs.view(np.int64)).cuda()   # 24-byte records as three words each
    torch.cuda.synchronize()

    def timed(call):
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            call()   # synchronises the context's stream before it returns
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return 1e3 * best

    ms_host = timed(lambda: ctx.u32_gate_rows(jobs, w.data_ptr(), n))
    refilled = bool(torch.equal(w, want))
    for rows in rows_of.values():
        w[:, torch.from_numpy(rows).cuda()] = 0
    torch.cuda.synchronize()
    ms_device = timed(lambda: ctx.u32_gate_rows(d_jobs.data_ptr(), w.data_ptr(), n, njobs=jobs.size))
    refilled = refilled and bool(torch.equal(w, want))
    del want

    data = m.CircuitData.build(ctx, circ)
    t0 = time.perf_counter()
    proof = data.prove(w.data_ptr(), pis, mem=m.MEM_DEVICE)
    ms_prove = 1e3 * (time.perf_counter() - t0)
    data.verify(proof, pis)
    data.close()
    del w, d_jobs
    torch.cuda.empty_cache()

    # the host path this replaces: the numpy fillers over the same rows (they draw their random inputs too: timed apart)
    fillers = {m.binding.U32_ARITHMETIC: ug.fill_u32_arithmetic, m.binding.U32_ADD_MANY: ug.fill_u32_add_many,
               m.binding.U32_SUBTRACTION: ug.fill_u32_subtraction, m.binding.U32_RANGE_CHECK: ug.fill_u32_range_check,
               m.binding.U32_COMPARISON: ug.fill_comparison}
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    for kind, fill in fillers.items():
        fill(wires, rows_of[kind], rng)
    ms_fill = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for kind, (_, ops, input_wires) in ug.U32_JOB_KINDS.items():
        for op in range(ops):
            for _ in input_wires(op):
                rng.integers(0, 1 << 32, size=rows_of[kind].size, dtype=np.uint64)
    ms_draw = 1e3 * (time.perf_counter() - t0)

    upload_ms = ms_host - ms_device
    return {"workload": "lcp2_u32_gate_rows on the reference's gate mix at 2^%d rows: %s; the rows zeroed in a device copy of the witness and refilled "
                        "with one call, list sorted by (kind, op, row); proof from the refilled matrix verified"
                        % (degree_bits, ", ".join("%s x%d" % (ug.U32_JOB_KINDS[k][0], rows_of[k].size) for k in sorted(rows_of))),
            "degree_bits": degree_bits, "jobs": int(jobs.size), "job_list_bytes": int(jobs.nbytes), "cells_written": int(cells), "bytes_written": int(8 * cells),
            "ms_host_list_validation_and_upload_included": round(ms_host, 3), "ms_device_resident_list": round(ms_device, 3),
            "ms_host_list_minus_device_list": round(upload_ms, 3),
            "dominates_host_list_call": "upload" if upload_ms > ms_device else "stores",
            "store_gb_per_s_device_list": round(8 * cells / ms_device / 1e6, 1),
            "refilled_matrix_equals_host_witness_on_owned_cells_and_zero_elsewhere": refilled,
            "ms_numpy_fillers_same_rows_one_host_thread": round(ms_fill, 1), "ms_of_that_drawing_random_inputs": round(ms_draw, 1),
            "ms_witness_jobs_numpy": round(1e3 * t_jobs, 1), "ms_prove_from_refilled_matrix_first_call": round(ms_prove, 1), "proof_verified": True,
            "best_of": reps}


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bits = int(args[0]) if args else 22
    reps = int(args[1]) if len(args) > 1 else 3
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    print(json.dumps(measure(ctx, bits, reps)))
