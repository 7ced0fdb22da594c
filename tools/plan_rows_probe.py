#!/usr/bin/env python3
"""lcp2_witness_plan_rows as a workload: PoseidonGate chains walked on the device, against the same rows through
lcp2_poseidon_gate_rows with inputs the host computes.  Three workloads:
  (a) one sponge chain of 3 152 rows (8 immediates per row, the capacity PREV 8..11)
  (b) 2 776 rows as independent chains of Merkle-path depth (recursion_gates.MERKLE_DEPTHS in turn: PREV 0..3, an immediate sibling)
  (c) recursion_gates.verifier_plan at the size of the recursive step (653 paths, a 3 152-row sponge: all five levels, rec jobs included)
each from a zero matrix with resident lists and with host lists (validation and upload included), best of `reps`.  The host side of the
comparison walks the same plan on ONE host thread through csrc/pos_plan.hpp compiled for the CPU (tests/emu/emu_plan.cpp: the
permutation of every row, which is what a host generator has to run before it knows the next row's inputs), gathers (row, swap,
12 inputs) per row and calls lcp2_poseidon_gate_rows once; both parts are timed, and the three matrices must be equal.
Prints ONE JSON line and writes it to profiles/plan_rows_probe.json.
    python3 tools/plan_rows_probe.py 5"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # rows_lib: the builder of the CPU emulations
NW = 135


def host_walk(E, plan, n):
    """the plan on one host thread, level by level: (matrix, ms)"""
    import rows_lib
    t0 = time.perf_counter()
    got, flags = rows_lib.run_levels(E, plan, n, threads=256)
    ms = 1e3 * (time.perf_counter() - t0)
    assert rows_lib.refusal(E, flags, plan) is None
    return got, ms


def workload(ctx, E, name, plan, n, reps):
    import numpy as np
    import torch
    import eth_lc_plonky2_amd as m
    host_matrix, ms_walk = min((host_walk(E, plan, n) for _ in range(reps)), key=lambda r: r[1])
    want = torch.from_numpy(host_matrix.view(np.int64)).cuda()
    w = torch.zeros_like(want)
    dev = [torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * (-a.nbytes % 8) + b"\0" * 8, dtype=np.int64).copy()).cuda()
           for a in (plan.rec_jobs, plan.pos_jobs, plan.chain_ends, plan.operands)]
    torch.cuda.synchronize()

    def timed(call, clear=True):
        best = None
        for _ in range(reps):
            if clear:
                w.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()   # synchronises the context's stream before it returns
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        return 1e3 * best

    ends = (plan.rec_level_ends, plan.pos_level_ends)
    ms_host = timed(lambda: ctx.witness_plan_rows(plan.rec_jobs, plan.pos_jobs, plan.chain_ends, plan.operands, *ends, w.data_ptr(), NW, n))
    same = bool(torch.equal(w, want))
    ms_resident = timed(lambda: ctx.witness_plan_rows(*(d.data_ptr() for d in dev), *ends, w.data_ptr(), NW, n, nrec=plan.rec_jobs.size,
                                                      npos=plan.pos_jobs.size, nchains=plan.chain_ends.size, noperands=plan.operands.size))
    same = same and bool(torch.equal(w, want))
    # the same PoseidonGate rows through lcp2_poseidon_gate_rows: inputs and swap flags as the host walk left them
    rows = np.zeros(plan.pos_jobs.size, dtype=m.binding.POSEIDON_ROW_DTYPE)
    r = plan.pos_jobs["row"]
    rows["row"], rows["swap"], rows["in"] = r, host_matrix[24, r], host_matrix[:12, r].T
    w.copy_(want)   # (the rec rows stay; the PoseidonGate rows are rewritten)
    w[:, torch.from_numpy(r.astype(np.int64)).cuda()] = 0
    ms_rows = timed(lambda: ctx.poseidon_gate_rows(rows, w.data_ptr(), n), clear=False)
    same_rows = bool(torch.equal(w, want))
    longest = int(np.diff(np.concatenate([[0], plan.chain_ends])).max())
    return {"name": name, "poseidon_rows": int(plan.pos_jobs.size), "chains": int(plan.chain_ends.size), "longest_chain": longest,
            "rec_jobs": int(plan.rec_jobs.size), "levels": int(len(plan.rec_level_ends)), "matrix_rows": n,
            "list_bytes": int(sum(a.nbytes for a in (plan.rec_jobs, plan.pos_jobs, plan.chain_ends, plan.operands))),
            "ms_resident_lists": round(ms_resident, 3), "ms_host_lists_validation_and_upload_included": round(ms_host, 3),
            "ms_host_walk_one_thread": round(ms_walk, 3), "ms_poseidon_gate_rows_from_host_inputs": round(ms_rows, 3),
            "ms_host_walk_plus_poseidon_gate_rows": round(ms_walk + ms_rows, 3),
            "us_per_row_host_walk": round(1e3 * ms_walk / max(plan.pos_jobs.size, 1), 3),
            "faster": "device (resident lists)" if ms_resident < ms_walk + ms_rows else "host walk + lcp2_poseidon_gate_rows",
            "device_matrices_equal_host_walk": same, "poseidon_gate_rows_matrix_equal": same_rows}


def measure(ctx, reps=5):
    import numpy as np
    from eth_lc_plonky2_amd import recursion_gates as rg
    import rows_lib
    E = rows_lib.emu_plan()
    rng = np.random.default_rng(31)
    f = lambda: int(rng.integers(0, rg.P, dtype=np.uint64))   # noqa: E731
    Z = rg.IMM(0)
    sponge = [(k, Z, [rg.IMM(f()) for _ in range(8)] + ([Z] * 4 if k == 0 else [rg.PREV(8 + i) for i in range(4)])) for k in range(3152)]
    a = rg.pack_witness_plan([([], [sponge])])
    paths, row = [], 0
    while row < 2776:
        depth = min(rg.MERKLE_DEPTHS[len(paths) % len(rg.MERKLE_DEPTHS)], 2776 - row)
        paths.append([(row + k, rg.IMM(f() & 1), ([rg.IMM(f()) for _ in range(4)] if k == 0 else [rg.PREV(i) for i in range(4)])
                       + [rg.IMM(f()) for _ in range(4)] + [Z] * 4) for k in range(depth)])
        row += depth
    b = rg.pack_witness_plan([([], paths)])
    c = rg.verifier_plan(8192, seed=3, paths=653, sponge=3152, expected=False)
    out = [workload(ctx, E, "a: one sponge chain of 3152 rows", a, 4096, reps),
           workload(ctx, E, "b: 2776 rows as independent chains of Merkle-path depth", b, 4096, reps),
           workload(ctx, E, "c: verifier_plan(8192, paths=653, sponge=3152)", c, 8192, reps)]
    per_row = round(1e3 * out[0]["ms_resident_lists"] / 3152, 3)
    return {"workload": "lcp2_witness_plan_rows (k_pos_plan_chains: one 16-lane group per chain) from a zero matrix, resident and host lists, next to "
                        "one host thread walking the same plan (csrc/pos_plan.hpp on the CPU) followed by lcp2_poseidon_gate_rows",
            "us_per_row_device_chain_a": per_row, "workloads": out, "best_of": reps}


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 5
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    line = json.dumps(measure(ctx, reps))
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "plan_rows_probe.json"), "w") as f:
        f.write(line + "\n")
