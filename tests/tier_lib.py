"""The gate degrees and the half-tier bundles of K6 restated in Python from a GateSet's programs (include/lcp2.h:
lcp2_gate_program_degree, lcp2_circuit_gate_tiers), for the tests that hold the library to them."""
import os
import subprocess

from gate_program_ref import program_degree  # noqa: F401  (the rule itself; the bundle logic below builds on it)


def gateset_degrees(gs):
    return [program_degree(gs.code[2 * g.code_offset:2 * (g.code_offset + g.code_len)], gs.max_regs) for g in gs.gates]


def expected_bundles(gs, quotient_degree_factor):
    """the bundles of a GateSet, from the degrees restated here"""
    return bundles_of([(G.selector_index, G.group_start, G.group_end, G.num_constraints) for G in gs.gates], gateset_degrees(gs),
                      quotient_degree_factor)


def bundles_of(gates, deg, quotient_degree_factor):
    """bundle index per gate (-1: full tier) for gates = [(selector_index, group_start, group_end, num_constraints)]: per selector
    group the gates with constraints and degree <= 2^(q-1), by falling degree, first-fit into bundles with
    max degree + size - 1 <= 2^(q-1)"""
    q = (quotient_degree_factor - 1).bit_length()
    half = 1 << (q - 1)
    order = sorted((g for g in range(len(gates)) if gates[g][3] and deg[g] <= half), key=lambda g: -deg[g])
    bundles, out = [], [-1] * len(gates)   # bundles: [group key, max degree, members]
    for g in order:
        key = tuple(gates[g][:3])
        for b, (k, md, members) in enumerate(bundles):
            if k == key and md + len(members) <= half:
                break
        else:
            b = len(bundles)
            bundles.append([key, deg[g], []])
        bundles[b][2].append(g)
        out[g] = b
    return out


# ---------------------------------------------------------------- tests/cpp/test_tiers: the same on the host layer's light-client gate set
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS_BIN = os.path.join(ROOT, "tests", "cpp", "test_tiers")


def build_tiers_binary():
    import cpp_build
    cpp_build.build()   # liblcp2.so, liboracle.so, golden_data.hpp
    src = os.path.join(cpp_build.CPP, "test_tiers.cpp")
    srcs = [src] + [os.path.join(cpp_build.HOST, f) for f in cpp_build.HOST_SOURCES]
    deps = srcs + [os.path.join(cpp_build.HOST, f) for f in os.listdir(cpp_build.HOST) if f.endswith(".hpp")] + cpp_build.SHARED_HEADERS + [
        os.path.join(ROOT, "oracle", "plonk.h"), os.path.join(cpp_build.CPP, "golden_data.hpp")]
    if not os.path.exists(TIERS_BIN) or any(os.path.getmtime(d) > os.path.getmtime(TIERS_BIN) for d in deps):
        pkg, orc = os.path.join(ROOT, "eth-lc-plonky2_amd"), os.path.join(ROOT, "oracle")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", TIERS_BIN] + srcs + ["-L", pkg, "-llcp2", "-L", orc, "-loracle",
                        "-Wl,-rpath," + pkg, "-Wl,-rpath," + orc, "-fopenmp"], check=True)
    return TIERS_BIN


def run_tiers_binary(*args, timeout=300):
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "16")
    env.pop("LCP2_QUOTIENT_TIERS", None)
    return subprocess.run([build_tiers_binary()] + list(args), capture_output=True, text=True, timeout=timeout, env=env)
