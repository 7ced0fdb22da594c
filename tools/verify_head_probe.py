#!/usr/bin/env python3
"""lcp2_verify_batch_ex, host head against device head: one proof of the synthetic circuit under standard_params(19), made once on the
GPU and replicated, verified in batches of 1, 8, 32 and 256 with head="host" and head="device" ALTERNATELY in the same run, on
host-resident and on device-resident proofs.  `reps` samples each after one warm-up call; every sample is kept, the best is reported.
One more line for a small circuit with many public inputs (--many_pis=N, default 2000; 0 leaves it out).  No threshold is set here:
the figures are recorded as they come, with the smallest batch from which the device head wins.  Prints ONE JSON line and writes it
to profiles/verify_head_probe.json (or --out=PATH).  The whole run ends itself after --limit=SECONDS (default 420).
    python3 tools/verify_head_probe.py 5"""
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (1, 8, 32, 256)


def alternate(calls, reps):
    """{name: samples in ms}: one warm-up call of each, then `reps` rounds of every call in turn"""
    for f in calls.values():
        f()
    samples = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            samples[k].append(round(1e3 * (time.perf_counter() - t0), 3))
    return samples


def batches(ctx, m, data, proof, pis, reps, counts):
    import numpy as np
    rows = []
    for count in counts:
        proofs = np.ascontiguousarray(np.repeat(proof[None, :], count, axis=0))
        all_pis = np.ascontiguousarray(np.repeat(np.asarray(pis, dtype=np.uint64)[None, :], count, axis=0))
        dev = ctx.buffer_alloc(proofs.size)
        ctx.buffer_write(dev, proofs)

        def call(head, device):
            def f():
                got = (ctx.verify_batch(data, dev, all_pis, mem=m.binding.MEM_DEVICE, count=count, head=head) if device
                       else ctx.verify_batch(data, proofs, all_pis, head=head))
                assert not got.any()
            return f
        samples = alternate({"host_head_host_proofs": call("host", False), "device_head_host_proofs": call("device", False),
                             "host_head_device_proofs": call("host", True), "device_head_device_proofs": call("device", True)}, reps)
        ctx.buffer_free(dev)
        rows.append({"count": count, "best_of": reps, **{"ms_" + k: min(v) for k, v in samples.items()}, "samples_ms": samples})
    return rows


def measure(ctx, reps, degree_bits=19, many_pis=2000):
    import eth_lc_plonky2_amd as m
    params = m.standard_params(degree_bits, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=degree_bits)
    data = m.CircuitData.build(ctx, circ)
    proof = data.prove(wires, pis)
    data.verify(proof, pis)
    rows = batches(ctx, m, data, proof, pis, reps, BATCHES)
    data.close()
    out = {"workload": "lcp2_verify_batch_ex on copies of one 2^%d-row proof under standard_params: LCP2_VERIFY_HEAD_HOST against "
                       "LCP2_VERIFY_HEAD_DEVICE (k_verify_transcript, k_verify_identity, k_verify_head_finish), alternately" % degree_bits,
           "degree_bits": degree_bits, "num_public_inputs": int(circ.num_public_inputs), "batches": rows}
    for mem in ("host_proofs", "device_proofs"):
        wins = [r["count"] for r in rows if r["ms_device_head_" + mem] < r["ms_host_head_" + mem]]
        out["smallest_batch_where_device_head_wins_" + mem] = min(wins) if wins else None
    if many_pis:
        bits = 10
        while (1 << bits) < many_pis // 8 + 16:
            bits += 1
        try:
            circ, wires, pis = m.circuit.synthetic_circuit(m.standard_params(bits, 4), seed=3, npi=many_pis)
            data = m.CircuitData.build(ctx, circ)
            proof = data.prove(wires, pis)
            data.verify(proof, pis)
            out["many_public_inputs"] = {"degree_bits": bits, "num_public_inputs": many_pis, "batches": batches(ctx, m, data, proof, pis, reps, (1, 32))}
            data.close()
        except (AssertionError, m.Lcp2Error) as e:  # recorded, not hidden: the line is then missing from the table
            out["many_public_inputs"] = {"degree_bits": bits, "num_public_inputs": many_pis, "error": repr(e)}
    return out


if __name__ == "__main__":
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    signal.alarm(int(opts.get("limit", 420)))  # the run's own time limit
    ctx = m.Context(0)
    line = json.dumps(measure(ctx, int(args[0]) if args else 5, int(opts.get("degree_bits", 19)), int(opts.get("many_pis", 2000))))
    print(line)
    out = opts.get("out", os.path.join(ROOT, "profiles", "verify_head_probe.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    ctx.close()
