#!/usr/bin/env python3
"""Times lcp2_stark_prove for the Fibonacci and the Poseidon full-round AIR of eth_lc_plonky2_amd.stark.

Per AIR and size (2^16, 2^18, 2^20 rows by default): wall time around the synchronous call (warm-up calls first, then the median and
the extremes of the timed ones), and from one further call with lcp2_prof_* on the time per kernel family - the witness check and the
quotient kernel are the `quotient` family, the quotient's transform is `intt` next to the trace's, commitments are `lde` / `leaf_hash`
/ `merkle`, the openings `openings` / `fri` / `pow`.  Standard config (rate 3, cap height 4, 16 PoW bits, 28 queries, arity 4), two
challenges.  Each proof is verified (lcp2_stark_verify) once.  Nothing is asserted about the times: they are recorded.

    python3 tools/stark_probe.py [--log-rows 16 18 20] [--rounds 5] [--out profiles/stark_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eth_lc_plonky2_amd as m  # noqa: E402
from eth_lc_plonky2_amd import stark  # noqa: E402

AIRS = {"fibonacci": 0, "poseidon_round": 3}   # name -> quotient_degree_bits


def clone(state):
    out = type(state)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(state), ctypes.sizeof(out))
    return out


def probe(ctx, air_name, log_n, rounds, warmup):
    make_air, make_trace = stark.AIRS[air_name]
    air = make_air()
    trace, pis = make_trace(log_n)
    cfg = m.fri_config(log_n)
    desc = stark.pack_stark_desc(air, cfg, log_n, AIRS[air_name], 2)
    start = m.binding.Challenger()
    start.observe([log_n, len(air.code)])
    times, proof = [], None
    for r in range(warmup + rounds):
        state = clone(start.state)
        t0 = time.perf_counter()
        proof = ctx.stark_prove(desc, trace, pis, state)
        if r >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    assert m.stark_verify(desc, pis, clone(start.state), proof) == 0
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.stark_prove(desc, trace, pis, clone(start.state))
    families = {k: round(v["ms"], 4) for k, v in ctx.prof_get().items() if v["launches"]}
    ctx.prof_enable(False)
    return {"air": air_name, "log_rows": log_n, "width": air.width, "quotient_degree_bits": AIRS[air_name], "proof_words": int(proof.size),
            "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times), "families_ms": families}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_probe.json"))
    a = ap.parse_args()
    ctx = m.Context(0)
    results = [probe(ctx, air, lg, a.rounds, a.warmup) for air in AIRS for lg in a.log_rows]
    for r in results:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/stark_probe.py", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
