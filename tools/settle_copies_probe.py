#!/usr/bin/env python3
"""lcp2_witness_settle_copies beside lcp2_witness_fill_copies as a workload: the synthetic circuit of tools/fill_copies_probe.py at 2^bits
rows, ONE source per copy class (the smallest cell), the device matrix holding the witness with every other cell of every class
overwritten before each call.  Times, wall around the call (both calls synchronise the stream) and the event time the library
books for the call's passes under LCP2_K_OTHER, 3 warm-ups and the median of 10, the four variants alternating:
  (a) lcp2_witness_fill_copies from a host list      (b) the same from a device list
  (c) lcp2_witness_settle_copies from a device list  (d) the same from a host list
After every call the matrix is compared with the witness on the device.  Prints ONE JSON line per size.
    python3 tools/settle_copies_probe.py 18 22"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUPS, REPS = 3, 10


def measure(ctx, degree_bits):
    import numpy as np
    import torch
    import eth_lc_plonky2_amd as m
    params = m.standard_params(degree_bits, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=3)
    n, nr = circ.n, params.num_routed_wires
    data = m.CircuitData.build(ctx, circ)
    class_of, num_classes = data.copy_classes()
    # one cell per class: the smallest (the classes are numbered in the order of their smallest cells, so a class's first cell is
    # where the running maximum of the numbers steps up)
    flat = class_of.ravel()
    in_class = np.nonzero(flat != 0xFFFFFFFF)[0]
    numbers = flat[in_class].astype(np.int64)
    owners = in_class[numbers > np.concatenate([[-1], np.maximum.accumulate(numbers)[:-1]])]
    assert owners.size == num_classes
    cells = np.zeros(owners.size, dtype=m.binding.CELL_DTYPE)
    cells["row"], cells["col"], cells["value"] = owners % n, owners // n, wires[:nr].ravel()[owners]
    sources = np.zeros(owners.size, dtype=m.binding.CELL_REF_DTYPE)
    sources["row"], sources["col"] = cells["row"], cells["col"]
    d_cells = torch.from_numpy(cells.view(np.int64).copy()).cuda()
    d_sources = torch.from_numpy(sources.view(np.int64).copy()).cuda()

    want = torch.from_numpy(wires.view(np.int64)).cuda()
    others = torch.from_numpy(flat != 0xFFFFFFFF)
    others[torch.from_numpy(owners)] = False
    start = want.clone()
    start[:nr].view(-1)[others.cuda()] = 0x5EED   # every cell of every class but its source
    del numbers, in_class, others
    w = torch.empty_like(want)
    D = m.binding.MEM_DEVICE
    calls = {"fill_host_list": lambda: data.fill_copies(cells, w.data_ptr()),
             "fill_device_list": lambda: data.fill_copies(d_cells.data_ptr(), w.data_ptr(), mem=D, ncells=cells.size),
             "settle_device_list": lambda: data.settle_copies(d_sources.data_ptr(), w.data_ptr(), mem=D, nsources=sources.size),
             "settle_host_list": lambda: data.settle_copies(sources, w.data_ptr())}
    wall, events = {k: [] for k in calls}, {k: [] for k in calls}
    same = True
    ctx.prof_enable(True)
    for rep in range(WARMUPS + REPS):
        for what, call in calls.items():
            w.copy_(start)
            torch.cuda.synchronize()
            ctx.prof_reset()
            t0 = time.perf_counter()
            report = call()
            t = 1e3 * (time.perf_counter() - t0)
            same = same and bool(torch.equal(w, want)) and report.classes_set == num_classes and not report.unsat
            if rep >= WARMUPS:
                wall[what].append(t)
                events[what].append(ctx.prof_get()["other"]["ms"])
    ctx.prof_enable(False)
    ok = data.check_witness(w.data_ptr(), pis, mem=D).ok
    data.close()
    med = {k: statistics.median(v) for k, v in wall.items()}
    return {"workload": "synthetic circuit at 2^%d rows, one source per copy class (its smallest cell), every other class cell overwritten before each call; "
                        "wall ms around the call, %d warm-ups, median of %d, the four variants alternating" % (degree_bits, WARMUPS, REPS),
            "degree_bits": degree_bits, "routed_cells": int(nr * n), "num_classes": int(num_classes), "cells_filled": int(report.cells_filled),
            "list_bytes_fill": int(cells.nbytes), "list_bytes_settle": int(sources.nbytes),
            "ms_median": {k: round(v, 3) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in wall.items()},
            "ms_device_events_median": {k: round(statistics.median(v), 3) for k, v in events.items()},
            "ratio_settle_device_over_fill_device": round(med["settle_device_list"] / med["fill_device_list"], 4),
            "matrix_equals_the_witness_after_every_call": same, "check_witness_ok": bool(ok)}


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    for bits in [int(a) for a in sys.argv[1:]] or [18, 22]:
        print(json.dumps(measure(ctx, bits)), flush=True)
