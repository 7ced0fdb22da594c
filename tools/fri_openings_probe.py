#!/usr/bin/env python3
"""Times lcp2_fri_prove_openings on the Plonk-shaped instance beside lcp2_fri_open of a circuit of the same size, in one process.

The instance: 4 oracles of 135 / num_constants + 80 / 20 / 16 columns of random coefficients, 2 points (zeta over everything,
g zeta over the first two columns of the third oracle), standard config (rate 3, cap height 4, 16 PoW bits, 28 queries, arity 4).
The comparison: lcp2_fri_open on a synthetic circuit of the same number of rows, proven up to its quotient once and then opened again
and again at the same zeta (the handle stays at that stage).  Both calls are synchronous and return host data, so wall time around
the call is the measure.  After warm-up calls the two are timed ALTERNATELY, call by call, so that clocks and other tenants of the
device hit both alike; reported are the median, the extremes and the ratio of the medians, and - from one further call each with
lcp2_prof_* on - the time per kernel family.  The proof of the generic call is verified (lcp2_fri_verify_openings) once.

    python3 tools/fri_openings_probe.py [--log-rows 16 19] [--rounds 9] [--out profiles/fri_openings_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eth_lc_plonky2_amd as m  # noqa: E402

P = m.GOLDILOCKS_P
NUM_CONSTANTS = 4


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def clone(state):
    out = type(state)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(state), ctypes.sizeof(out))
    return out


def families(ctx):
    return {k: round(v["ms"], 4) for k, v in ctx.prof_get().items() if v["launches"]}


def probe(ctx, log_n, rounds, warmup, seed=1):
    rng = np.random.default_rng(seed)
    params = m.standard_params(log_n, NUM_CONSTANTS)
    n = 1 << log_n
    # ---- the circuit handle, up to its quotient
    circ, wires, pis = m.circuit.synthetic_circuit(params, seed=seed, small_values=True)
    data = m.CircuitData.build(ctx, circ)
    data.commit_wires(wires)
    draw = lambda k: rng.integers(1, P, k, dtype=np.uint64)
    data.perm_zs(draw(2), draw(2))
    data.quotient(draw(2), m.binding.hash_no_pad(pis))
    zeta = draw(2)
    plonk_proof = np.zeros(data.proof_words, dtype=np.uint64)
    start = m.binding.Challenger()
    start.observe(draw(4))

    def plonk_call():
        state = clone(start.state)
        t = time.perf_counter()
        data.fri_open(zeta, state, plonk_proof)
        return 1e3 * (time.perf_counter() - t)

    # ---- the bare oracles of the same shape
    cols = [135, NUM_CONSTANTS + 80, 20, 16]
    oracles = []
    for k in cols:
        coeffs = rng.integers(0, P, (k, n), dtype=np.uint64)
        oracles.append(ctx.commit_coeffs(coeffs, params.rate_bits, params.cap_height))
        del coeffs
    ranges = [[(o, 0, k) for o, k in enumerate(cols)], [(2, 0, 2)]]
    inst = m.fri_instance(4, ranges)
    cfg = m.fri_config(log_n, params.rate_bits, params.cap_height, params.proof_of_work_bits, params.num_query_rounds, 4, 5)
    assert cfg.num_fri_layers == params.num_fri_layers
    g = pow(1753635133440165772, 1 << (32 - log_n), P)
    points = [(int(zeta[0]), int(zeta[1])), (int(zeta[0]) * g % P, int(zeta[1]) * g % P)]
    kept = {}

    def generic_call():
        state = clone(start.state)
        t = time.perf_counter()
        kept["proof"] = ctx.fri_prove_openings(oracles, inst, points, cfg, state)
        return 1e3 * (time.perf_counter() - t)

    try:
        for _ in range(warmup):
            plonk_call()
            generic_call()
        verdict = m.fri_verify_openings([o.cap for o in oracles], cols, log_n, inst, points, cfg, clone(start.state), kept["proof"])
        plonk_ms, generic_ms = [], []
        for _ in range(rounds):   # alternately, call by call
            plonk_ms.append(plonk_call())
            generic_ms.append(generic_call())
        ctx.prof_enable(True)
        ctx.prof_reset()
        plonk_call()
        plonk_families = families(ctx)
        ctx.prof_reset()
        generic_call()
        generic_families = families(ctx)
        ctx.prof_enable(False)
    finally:
        for o in oracles:
            o.close()
        data.close()
    a, b = stats(plonk_ms), stats(generic_ms)
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    return {"log_rows": log_n, "oracle_columns": cols, "points_ranges": ranges, "proof_words": int(kept["proof"].size), "generic_proof_verified": verdict == 0,
            "lcp2_fri_open": a, "lcp2_fri_prove_openings": b, "ratio_generic_over_fri_open": b["median_ms"] / a["median_ms"],
            "difference_ms": b["median_ms"] - a["median_ms"], "run_to_run_spread_ms": spread,
            "kernel_family_ms_one_call": {"lcp2_fri_open": plonk_families, "lcp2_fri_prove_openings": generic_families}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--log-rows", type=int, nargs="+", default=[16, 19])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_openings_probe.json"))
    args = ap.parse_args()
    ctx = m.Context(0)
    results = []
    try:
        for log_n in args.log_rows:
            results.append(probe(ctx, log_n, args.rounds, args.warmup))
            print(json.dumps(results[-1]), flush=True)
    finally:
        ctx.close()
    out = {"tool": "tools/fri_openings_probe.py", "method": "wall time around each synchronous call; %d warm-up calls each, then %d calls each, alternating; "
           "both calls in one process on one context" % (args.warmup, args.rounds), "results": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
