#!/usr/bin/env python3
"""lcp2_witness_fill_copies as a workload: the synthetic circuit at 2^bits rows.  Times (wall, the calls synchronise the stream):
  - the one-time construction of the class table (the first lcp2_circuit_copy_classes of a fresh handle), with the event time the
    library books for it under LCP2_K_OTHER and the number of pointer-jumping rounds (scopes booked minus the decode and the numbering
    scope); the decode itself is the one lcp2_check_witness runs per call, whose copy pass (LCP2_K_PERM_Z) is timed beside it;
  - warm and alternating, best of `reps`: lcp2_witness_fill_copies with ONE cell per class into a zeroed device matrix,
    lcp2_scatter_cells of EVERY cell of every class of the same witness (the list a caller without this call sends), and the
    plain upload of the whole matrix.  The cells in no class are the same plain writes either way and are left out of both lists.
The cells of the classes are compared with the witness on the device after every call.  Prints ONE JSON line.
    python3 tools/fill_copies_probe.py 22 3"""
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
    params = m.standard_params(degree_bits, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=seed)
    n, nr = circ.n, params.num_routed_wires
    data = m.CircuitData.build(ctx, circ)
    ctx.prof_enable(True)
    ctx.prof_reset()
    t0 = time.perf_counter()
    class_of, num_classes = data.copy_classes()
    ms_build_and_download = 1e3 * (time.perf_counter() - t0)
    prof = ctx.prof_get()
    ms_build_events, scopes = prof["other"]["ms"], int(prof["other"]["launches"])
    t0 = time.perf_counter()
    data.copy_classes()
    ms_download = 1e3 * (time.perf_counter() - t0)
    # the decode pass alone: the same circuit with one sigma value that is no cell id is refused right after the decode and its
    # permutation check, before the first round; the rounds and the numbering are the rest of the sum
    cs = circ.constants_sigmas.copy()
    cs[params.num_constants + 3, 9] = np.uint64(pow(7, nr, 0xFFFFFFFF00000001))
    refused = m.CircuitData.build(ctx, m.circuit.Circuit(params, circ.gateset, cs, circ.k_is, circ.num_public_inputs))
    del cs
    ctx.prof_reset()
    try:
        refused.copy_classes()
        raise AssertionError("the broken sigma column was accepted")
    except m.Lcp2Error:
        pass
    ms_decode = ctx.prof_get()["other"]["ms"]
    refused.close()

    # one cell per class: the smallest (the classes are numbered in the order of their smallest cells, so a class's first cell is
    # where the running maximum of the numbers steps up)
    flat = class_of.ravel()
    in_class = np.nonzero(flat != 0xFFFFFFFF)[0]
    numbers = flat[in_class].astype(np.int64)
    before = np.concatenate([[-1], np.maximum.accumulate(numbers)[:-1]])
    owners = in_class[numbers > before]
    assert owners.size == num_classes

    def cells(at):
        out = np.zeros(at.size, dtype=m.binding.CELL_DTYPE)
        out["row"], out["col"] = at % n, at // n
        out["value"] = wires[:nr].ravel()[at]
        return out

    per_class, every = cells(owners), cells(in_class)   # one cell per class; every cell of every class (what a caller sends without the call)
    mask = torch.from_numpy(flat != 0xFFFFFFFF).cuda()
    del numbers, before
    w = torch.zeros(wires.shape, dtype=torch.int64, device="cuda")
    want = torch.from_numpy(wires.view(np.int64)).cuda()
    best = {"fill": None, "scatter": None, "upload": None}
    same = True
    for _ in range(reps + 1):   # the first pass warms the scratch buffers up and is not counted
        for what in ("fill", "scatter", "upload"):
            w.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if what == "fill":
                report = data.fill_copies(per_class, w.data_ptr())
            elif what == "scatter":
                ctx.scatter_cells(every, w.data_ptr(), n)
            else:
                ctx.buffer_write(w.data_ptr(), wires)
            t = 1e3 * (time.perf_counter() - t0)
            same = same and bool(torch.equal(w[:nr].reshape(-1)[mask], want[:nr].reshape(-1)[mask]))
            if _:
                best[what] = t if best[what] is None else min(best[what], t)
    ctx.prof_reset()
    ok = data.check_witness(w.data_ptr(), pis, mem=m.binding.MEM_DEVICE).ok   # (w holds the uploaded matrix here)
    ms_decode_proxy = ctx.prof_get()["perm_z"]["ms"]
    data.close()
    return {"workload": "lcp2_witness_fill_copies on the synthetic circuit at 2^%d rows: one cell per copy class into a zeroed device matrix, "
                        "against lcp2_scatter_cells of every cell of every class and the upload of the whole matrix" % degree_bits,
            "degree_bits": degree_bits, "routed_cells": int(nr * n), "num_classes": int(num_classes), "cells_in_classes": int((flat != 0xFFFFFFFF).sum()),
            "class_table_bytes": int(flat.nbytes),
            "ms_class_table_first_call_wall_with_download": round(ms_build_and_download, 2), "ms_class_table_download_alone": round(ms_download, 2),
            "ms_class_table_device_events": round(ms_build_events, 3), "jumping_rounds_launched": scopes - 2,
            "ms_decode_and_permutation_check": round(ms_decode, 3), "ms_rounds_and_numbering": round(ms_build_events - ms_decode, 3),
            "ms_check_witness_copy_pass_same_decode": round(ms_decode_proxy, 3),
            "cells_sent_fill": int(per_class.size), "cells_sent_scatter": int(every.size), "matrix_bytes": int(wires.nbytes),
            "ms_fill_copies": round(best["fill"], 3), "ms_scatter_every_cell": round(best["scatter"], 3), "ms_upload_matrix": round(best["upload"], 3),
            "cells_filled": int(report.cells_filled), "classes_set": int(report.classes_set),
            "class_cells_equal_the_witness_after_every_call": same, "check_witness_ok": bool(ok), "best_of": reps}


def headline(ctx, steps=6, extra=6):
    """the benchmark's light-client step (2^22 rows with `extra` more committees) proved with the host layer's opt-in off and on,
    alternating: wall ms per data.prove(pw), proofs compared.  With LCP2_PROF set the host layer prints its own split of every
    witness generation (host generators, device rows, cells sent, their scatter / fill) to stdout."""
    import numpy as np
    from eth_lc_plonky2_amd import light_client as lc
    prev, cur = lc.reference_updates()
    sessions = {"off": lc.LightClientStep(ctx, prev, cur, 0, extra), "on": lc.LightClientStep(ctx, prev, cur, lc.FILL_COPIES, extra)}
    ms, proofs = {"off": [], "on": []}, {}
    for k in range(steps + 1):   # the first pass plans the witness generation (and builds the class table) and is not counted
        for mode, s in sessions.items():
            t0 = time.perf_counter()
            proof, pis = s.prove()
            if k:
                ms[mode].append(1e3 * (time.perf_counter() - t0))
            proofs[mode] = proof
    sessions["off"].verify(proofs["on"], pis)
    return {"workload": "light-client step 633 -> 634 + %d committees, data.prove(pw) with witness generation, opt-in off / on alternating" % extra,
            "degree_bits": int(sessions["on"].info.degree_bits), "steps": steps,
            "ms_per_prove_off": [round(v, 2) for v in ms["off"]], "ms_per_prove_on": [round(v, 2) for v in ms["on"]],
            "proofs_equal_word_for_word": bool((proofs["on"] == proofs["off"]).all()), "proof_verified": True}


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    if "--headline" in sys.argv:
        torch.cuda.set_device(0)
        print(json.dumps(headline(m.Context(0, stream=torch.cuda.current_stream().cuda_stream))), flush=True)
        sys.exit(0)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bits = int(args[0]) if args else 22
    reps = int(args[1]) if len(args) > 1 else 3
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    print(json.dumps(measure(ctx, bits, reps)))
