#!/usr/bin/env python3
"""Times lcp2_stark_prove for the Fibonacci and the Poseidon full-round AIR of eth_lc_plonky2_amd.stark.

Per AIR and size (2^16, 2^18, 2^20 rows by default): wall time around the synchronous call (warm-up calls first, then the median and
the extremes of the timed ones), and from one further call with lcp2_prof_* on the time per kernel family - the witness check and the
quotient kernel are the `quotient` family, the quotient's transform is `intt` next to the trace's, commitments are `lde` / `leaf_hash`
/ `merkle`, the openings `openings` / `fri` / `pow`.  Standard config (rate 3, cap height 4, 16 PoW bits, 28 queries, arity 4), two
challenges.  Each proof is verified (lcp2_stark_verify) once.  Nothing is asserted about the times: they are recorded.

--perm times lcp2_stark_prove_perm instead, on the range-check AIR (width 2, one pair of one column, q = 1, two challenges in one
batch: one Z column): k_stark_perm_ratio, k_stark_perm_close and the PERM quotient kernel are in the `quotient` family, the running
product in `perm_z`, the commitment of Z with the other commitments.  Its default output is profiles/stark_perm_probe.json.

    python3 tools/stark_probe.py [--perm] [--log-rows 16 18 20] [--rounds 5] [--out profiles/stark_probe.json]
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
PERM_AIRS = {"range_check": (1, 2)}            # name -> (quotient_degree_bits, batch size)


def clone(state):
    out = type(state)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(state), ctypes.sizeof(out))
    return out


def probe(ctx, air_name, log_n, rounds, warmup, perm=False):
    if perm:
        make_air, make_trace, make_perm = stark.PERM_AIRS[air_name]
        q, batch = PERM_AIRS[air_name]
        sperm = stark.pack_stark_perm(make_perm(batch))
    else:
        make_air, make_trace = stark.AIRS[air_name]
        q, sperm = AIRS[air_name], None
    air = make_air()
    trace, pis = make_trace(log_n)
    cfg = m.fri_config(log_n)
    desc = stark.pack_stark_desc(air, cfg, log_n, q, 2)
    start = m.binding.Challenger()
    start.observe([log_n, len(air.code)])
    times, proof = [], None
    for r in range(warmup + rounds):
        state = clone(start.state)
        t0 = time.perf_counter()
        proof = ctx.stark_prove(desc, trace, pis, state, perm=sperm)
        if r >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    assert m.stark_verify(desc, pis, clone(start.state), proof, perm=sperm) == 0
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.stark_prove(desc, trace, pis, clone(start.state), perm=sperm)
    families = {k: round(v["ms"], 4) for k, v in ctx.prof_get().items() if v["launches"]}
    ctx.prof_enable(False)
    return {"air": air_name, "permutation": bool(perm), "log_rows": log_n, "width": air.width, "quotient_degree_bits": q, "proof_words": int(proof.size),
            "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": len(times), "families_ms": families}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--perm", action="store_true", help="time lcp2_stark_prove_perm on the range-check AIR")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "stark_perm_probe.json" if a.perm else "stark_probe.json")
    ctx = m.Context(0)
    results = [probe(ctx, air, lg, a.rounds, a.warmup, a.perm) for air in (PERM_AIRS if a.perm else AIRS) for lg in a.log_rows]
    for r in results:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/stark_probe.py", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
