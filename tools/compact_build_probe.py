#!/usr/bin/env python3
"""The host layer's compact build (LCH_COMPACT_BUILD: no expanded matrix, lcp2_circuit_create_from_rows) against the ordinary build on
the benchmark's light-client step (2^22 rows with 6 more committees, through lc_capi), alternating, `runs` times each.  Every run is a
fresh child process, so that ru_maxrss is the peak of that build alone.  Per run: build_ms with its phases, attach_ms, the bytes
uploaded for the preprocessed columns, the LCP2_K_OTHER scopes booked while the session was created (compact: the passes of the
expansion), the wall ms of data.prove(pw) (one warm-up, then `proofs` timed) and the peak host memory.  The parent reports mean and
spread (max - min) of build_ms + attach_ms per mode and whether the proofs of the two modes are equal word for word.
    python3 tools/compact_build_probe.py [--runs 3] [--proofs 3] [--extra 6] [--out profiles/compact_build.json]"""
import hashlib
import json
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(mode, extra, proofs):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import light_client as lc
    ctx = m.Context(0)
    ctx.prof_enable(True)
    ctx.prof_reset()
    prev, cur = lc.reference_updates()
    t0 = time.perf_counter()
    s = lc.LightClientStep(ctx, prev, cur, lc.COMPACT_BUILD if mode == "compact" else 0, extra)
    create_wall = 1e3 * (time.perf_counter() - t0)
    rss_after_build = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    other = ctx.prof_get()["other"]
    i = s.info
    ms = []
    for k in range(proofs + 1):
        t0 = time.perf_counter()
        proof, pis = s.prove()
        if k:
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    s.verify(proof, pis)
    return {"mode": mode, "degree_bits": int(i.degree_bits), "gates": int(i.num_gates), "build_ms": round(i.build_ms, 1), "attach_ms": round(i.attach_ms, 1),
            "build_plus_attach_ms": round(i.build_ms + i.attach_ms, 1), "create_wall_ms": round(create_wall, 1),
            "build_phases_ms": {"gadgets": round(i.build_gadgets_ms, 1), "matrix": round(i.build_matrix_ms, 1), "identity_sigmas": round(i.build_identity_ms, 1),
                                "classes": round(i.build_classes_ms, 1), "cycles": round(i.build_cycles_ms, 1)},
            "attach_upload_bytes": int(i.attach_upload_bytes), "other_scopes_during_create": {"ms": round(other["ms"], 3), "scopes": int(other["launches"])},
            "prove_ms": ms, "proof_sha256": hashlib.sha256(proof.tobytes()).hexdigest(), "ru_maxrss_after_build_kib": int(rss_after_build),
            "ru_maxrss_end_kib": int(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)}


def spread(values):
    return {"mean": round(sum(values) / len(values), 1), "min": round(min(values), 1), "max": round(max(values), 1), "spread": round(max(values) - min(values), 1)}


def main(argv):
    def opt(name, default):
        return type(default)(argv[argv.index(name) + 1]) if name in argv else default
    if "--child" in argv:
        print(json.dumps(child(opt("--child", "ordinary"), opt("--extra", 6), opt("--proofs", 3))), flush=True)
        return 0
    runs, extra, proofs, out = opt("--runs", 3), opt("--extra", 6), opt("--proofs", 3), opt("--out", "")
    results = []
    for k in range(runs):
        for mode in ("ordinary", "compact"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--extra", str(extra), "--proofs", str(proofs)],
                               capture_output=True, text=True, timeout=400)
            if r.returncode != 0:   # nothing more is started on the device after a failed run
                print(r.stdout[-2000:] + r.stderr[-4000:], file=sys.stderr)
                return 1
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(results[-1]), flush=True)
    by = {mode: [r for r in results if r["mode"] == mode] for mode in ("ordinary", "compact")}
    summary = {"workload": "light-client step 633 -> 634 + %d committees through lc_capi: ordinary build (expanded matrix, lcp2_circuit_create) against "
                           "LCH_COMPACT_BUILD (rows and bindings, lcp2_circuit_create_from_rows), alternating, one fresh process per run" % extra,
               "runs_per_mode": runs,
               "build_plus_attach_ms": {mode: spread([r["build_plus_attach_ms"] for r in rs]) for mode, rs in by.items()},
               "build_ms": {mode: spread([r["build_ms"] for r in rs]) for mode, rs in by.items()},
               "attach_ms": {mode: spread([r["attach_ms"] for r in rs]) for mode, rs in by.items()},
               "prove_ms": {mode: spread([v for r in rs for v in r["prove_ms"]]) for mode, rs in by.items()},
               "ru_maxrss_after_build_kib": {mode: spread([r["ru_maxrss_after_build_kib"] for r in rs]) for mode, rs in by.items()},
               "attach_upload_bytes": {mode: rs[0]["attach_upload_bytes"] for mode, rs in by.items()},
               "proofs_equal_word_for_word": len({r["proof_sha256"] for r in results}) == 1,
               "runs": results}
    text = json.dumps(summary, indent=1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(text + "\n")
    print(json.dumps({k: v for k, v in summary.items() if k != "runs"}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
