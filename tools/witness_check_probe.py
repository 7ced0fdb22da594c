#!/usr/bin/env python3
"""lcp2_check_witness as a workload: the call on a witness resident in HBM, beside lcp2_prove of the same circuit from the same run.
For each size (default 19 and 22) and each circuit (the synthetic gate set, the reference gate mix): best-of-`reps` wall time of
the call, and the two kernels separately from the context's event timers (the gate pass is booked under the quotient family, the
copy pass under the permutation family; the probe resets the timers around the call), with the register footprint of the kernels
(tools/kernel_regs.py).  Prints ONE JSON line and writes the record, indented, to profiles/witness_check.json.
    python3 tools/witness_check_probe.py 19 22 --reps 5"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(ctx, bits, mix, reps):
    import numpy as np
    import torch
    import eth_lc_plonky2_amd as m
    extra = m.u32_gates.ReferenceMix() if mix else None
    circ, wires, pis = m.circuit.synthetic_circuit(m.standard_params(bits, 5 if mix else 4), seed=1, extra=extra)
    data = m.CircuitData.build(ctx, circ)
    w = torch.from_numpy(wires.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def best(call):
        t_best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            call()   # both calls synchronise the context's stream before they return
            t = time.perf_counter() - t0
            t_best = t if t_best is None else min(t_best, t)
        return 1e3 * t_best

    report = data.check_witness(w.data_ptr(), pis, mem=m.MEM_DEVICE)   # warm-up: tables, scratch
    ms_check = best(lambda: data.check_witness(w.data_ptr(), pis, mem=m.MEM_DEVICE))
    ctx.prof_enable(True)
    ctx.prof_reset()
    data.check_witness(w.data_ptr(), pis, mem=m.MEM_DEVICE)
    fam = ctx.prof_get()
    ctx.prof_enable(False)
    data.prove(w.data_ptr(), pis, mem=m.MEM_DEVICE)
    ms_prove = best(lambda: data.prove(w.data_ptr(), pis, mem=m.MEM_DEVICE))
    data.close()
    return {"circuit": "reference_mix" if mix else "synthetic", "degree_bits": bits, "ok": bool(report.ok),
            "ms_check_witness_resident": round(ms_check, 3), "ms_prove_resident_same_run": round(ms_prove, 3),
            "check_over_prove": round(ms_check / ms_prove, 4), "ms_k_witness_gates": round(fam["quotient"]["ms"], 3),
            "ms_k_witness_copies": round(fam["perm_z"]["ms"], 3), "best_of": reps,
            "method": "best of %d wall times of the call on a resident witness (it synchronises the stream), warm; the kernels from HIP "
                      "events of one more call; lcp2_prove best of the same count in the same process" % reps}


def kernel_footprints():
    """tools/kernel_regs.py k_witness, parsed"""
    import re
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "k_witness"], capture_output=True, text=True).stdout
    regs = {}
    for ln in out.splitlines():
        m = re.match(r"\S*?(k_witness\w+)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spill v(\d+) s(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            regs[m.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "vgpr_spills", "sgpr_spills", "static_lds", "scratch"), map(int, m.groups()[1:])))
    return regs


if __name__ == "__main__":
    import torch
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    if "--reps" in sys.argv:
        args.remove(str(reps))
    sizes = [int(a) for a in args] or [19, 22]
    torch.cuda.set_device(0)
    ctx = m.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    record = {"what": "lcp2_check_witness on an MI355X (tools/witness_check_probe.py %s): the call on a resident witness beside lcp2_prove of the "
                      "same circuit from the same run, and its two kernels separately" % " ".join(map(str, sizes)),
              "kernels": kernel_footprints(),
              "k_witness_gates_dynamic_lds": "(num_regs + 12) x threads x 8 bytes: 128 threads where that fits 64 KiB, else 64",
              "host_orc_check_witness": "not measured: tests/checks/ records no time of the oracle's orc_check_witness to set beside these",
              "no_threshold": "no test sets a bound on these figures",
              "runs": [measure(ctx, b, mix, reps) for b in sizes for mix in (False, True)]}
    print(json.dumps(record))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "witness_check.json"), "w") as f:
        f.write(json.dumps(record, indent=1) + "\n")
