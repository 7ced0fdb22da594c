#!/usr/bin/env python3
"""lcp2_verify_batch against a loop of lcp2_verify: one proof of the synthetic circuit under standard_params(19), made once on the
GPU and replicated, verified in batches of 1, 8, 32 and 256 - by the host verifier one proof after another, by the batch call on
host-resident proofs and by the batch call on device-resident proofs.  Best of `reps` after one warm-up call each.  No threshold is
set here: the host loop is the yardstick and the figures are recorded as they come (ms per proof on either side, and the smallest
batch from which the device call wins).  Prints ONE JSON line and writes it to profiles/verify_batch_probe.json (or --out=PATH).
The whole run ends itself after --limit=SECONDS (default 420).
    python3 tools/verify_batch_probe.py 5"""
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (1, 8, 32, 256)


def best(f, reps):
    f()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append(time.perf_counter() - t0)
    return 1e3 * min(times)


def measure(ctx, reps, degree_bits=19):
    import numpy as np
    import eth_lc_plonky2_amd as m
    params = m.standard_params(degree_bits, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=degree_bits)
    data = m.CircuitData.build(ctx, circ)
    proof = data.prove(wires, pis)
    data.verify(proof, pis)
    L = m.proof_layout(params)
    rows = []
    for count in BATCHES:
        proofs = np.ascontiguousarray(np.repeat(proof[None, :], count, axis=0))
        all_pis = np.ascontiguousarray(np.repeat(np.asarray(pis, dtype=np.uint64)[None, :], count, axis=0))
        dev = ctx.buffer_alloc(proofs.size)
        ctx.buffer_write(dev, proofs)

        def host_loop():
            for i in range(count):
                data.verify(proofs[i], all_pis[i])

        def batch_host():
            assert not ctx.verify_batch(data, proofs, all_pis).any()

        def batch_device():
            assert not ctx.verify_batch(data, dev, all_pis, mem=m.binding.MEM_DEVICE, count=count).any()
        r = max(1, reps if count <= 32 else min(reps, 3))
        ms = {"host_loop": best(host_loop, r), "batch_host_proofs": best(batch_host, r), "batch_device_proofs": best(batch_device, r)}
        ctx.buffer_free(dev)
        rows.append({"count": count, "best_of": r, **{"ms_" + k: round(v, 3) for k, v in ms.items()},
                     **{"ms_per_proof_" + k: round(v / count, 4) for k, v in ms.items()}})
    wins = [r["count"] for r in rows if r["ms_batch_host_proofs"] < r["ms_host_loop"]]
    wins_dev = [r["count"] for r in rows if r["ms_batch_device_proofs"] < r["ms_host_loop"]]
    data.close()
    return {"workload": "lcp2_verify (host, one proof at a time) against lcp2_verify_batch (k_verify_canon, k_verify_paths, k_verify_fri) on copies of one "
                        "2^%d-row proof under standard_params" % degree_bits,
            "degree_bits": degree_bits, "proof_words": int(L.total), "words_outside_queries": int(L.queries + L.total - L.final_poly),
            "num_query_rounds": int(params.num_query_rounds), "num_fri_layers": int(params.num_fri_layers),
            "ms_per_proof_host_verifier": rows[0]["ms_per_proof_host_loop"], "batches": rows,
            "smallest_batch_where_batch_call_wins_host_proofs": min(wins) if wins else None,
            "smallest_batch_where_batch_call_wins_device_proofs": min(wins_dev) if wins_dev else None}


if __name__ == "__main__":
    import eth_lc_plonky2_amd as m
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    signal.alarm(int(opts.get("limit", 420)))  # the run's own time limit
    ctx = m.Context(0)
    line = json.dumps(measure(ctx, int(args[0]) if args else 5, int(opts.get("degree_bits", 19))))
    print(line)
    out = opts.get("out", os.path.join(ROOT, "profiles", "verify_batch_probe.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    ctx.close()
