#!/usr/bin/env python3
"""Compressed proofs (pruned Merkle multiproofs): what they save and what verifying them costs.
  sizes   CPU only, exact arithmetic: compressed_words (eth-lc-plonky2_amd/proof_compress.py) over `--sets=N` random index sets
          (default 100, seed 0) for the standard config at 2^19 rows and the two wrap configs of lcp2_params_config's comment
          (rate_bits 7 / 12 queries; rate_bits 8 / cap_height 0 / 10 queries) at 2^12 rows: mean, minimum and maximum of the
          compressed size against the full size.
  verify  on a GPU (skipped with --sizes-only): lcp2_verify_batch_compressed against lcp2_verify_batch on the same 32 proofs - one
          2^19-row proof under standard_params(19), made on the GPU and replicated - under both heads, the four runs alternating
          inside every repetition (`reps` repetitions after one warm-up round; every sample is kept).
Prints ONE JSON line and writes it to profiles/compress_probe.json (or --out=PATH).  No threshold is set here.  The run ends itself
after --limit=SECONDS (default 420).
    python3 tools/compress_probe.py 7"""
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNT = 32


def sizes(sets):
    import numpy as np
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import proof_compress as pc
    configs = {"standard_2^19": m.standard_params(19, 4), "wrap_rate7_12_queries_2^12": m.params_config(12, 4, 7, 4, 16, 12, 4, 5),
               "wrap_rate8_cap0_10_queries_2^12": m.params_config(12, 4, 8, 0, 20, 10, 4, 5)}
    rng = np.random.default_rng(0)
    out = {}
    for name, p in configs.items():
        L = pc.layout(p)
        n = 1 << (p.degree_bits + p.rate_bits)
        words = [pc.compressed_words(p, rng.integers(0, n, size=p.num_query_rounds), L) for _ in range(sets)]
        out[name] = {"full_words": int(L.total), "words_outside_queries": int(L.outside), "index_sets": sets, "mean_words": round(float(np.mean(words)), 1),
                     "min_words": int(min(words)), "max_words": int(max(words)), "mean_ratio": round(float(np.mean(words)) / L.total, 4),
                     "min_ratio": round(min(words) / L.total, 4), "max_ratio": round(max(words) / L.total, 4),
                     "full_bytes": int(8 * L.total), "mean_bytes": int(8 * np.mean(words))}
    return out


def verify(ctx, reps, degree_bits=19):
    import numpy as np
    import eth_lc_plonky2_amd as m
    params = m.standard_params(degree_bits, 4)
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=degree_bits)
    data = m.CircuitData.build(ctx, circ)
    proof = data.prove(wires, pis)
    data.verify(proof, pis)
    comp = data.compress(proof, pis)
    assert (data.decompress(comp, pis) == proof).all()
    proofs = np.ascontiguousarray(np.repeat(proof[None, :], COUNT, axis=0))
    comps = np.ascontiguousarray(np.repeat(comp[None, :], COUNT, axis=0)).ravel()
    offsets = np.arange(COUNT + 1, dtype=np.uint64) * np.uint64(comp.size)
    all_pis = np.ascontiguousarray(np.repeat(np.asarray(pis, dtype=np.uint64)[None, :], COUNT, axis=0))
    runs = {}
    for head in ("host", "device"):
        runs["full_%s_head" % head] = lambda head=head: ctx.verify_batch(data, proofs, all_pis, head=head)
        runs["compressed_%s_head" % head] = lambda head=head: data.verify_batch_compressed(comps, all_pis, head=head, offsets=offsets)
    samples = {k: [] for k in runs}
    for rep in range(reps + 1):  # round 0 warms up
        for k, f in runs.items():
            t0 = time.perf_counter()
            got = f()
            dt = 1e3 * (time.perf_counter() - t0)
            assert not got.any()
            if rep:
                samples[k].append(round(dt, 3))
    data.close()
    return {"workload": "lcp2_verify_batch_compressed against lcp2_verify_batch on %d copies of one 2^%d-row proof under standard_params, host proofs, runs "
                        "alternating inside every repetition" % (COUNT, degree_bits),
            "count": COUNT, "proof_words": int(proof.size), "compressed_words": int(comp.size), "reps": reps, "samples_ms": samples,
            "median_ms": {k: round(float(np.median(v)), 3) for k, v in samples.items()}, "min_ms": {k: min(v) for k, v in samples.items()}}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--") and "=" not in a]
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    signal.alarm(int(opts.get("limit", 420)))  # the run's own time limit
    result = {"sizes": sizes(int(opts.get("sets", 100)))}
    if "--sizes-only" not in flags:
        import eth_lc_plonky2_amd as m
        ctx = m.Context(0)
        result["verify"] = verify(ctx, int(args[0]) if args else 7, int(opts.get("degree_bits", 19)))
        ctx.close()
    line = json.dumps(result)
    print(line)
    out = opts.get("out", os.path.join(ROOT, "profiles", "compress_probe.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
