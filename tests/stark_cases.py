"""What the STARK tests share (test harness only): the CPU emulation tests/emu/emu_stark.cpp, the shapes, and per shape the AIR, its
trace, the description for the C ABI and - computed once per process, never changed - the model's proof."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np

from rows_lib import build_emu

P = 0xFFFFFFFF00000001
SEED = (11, 7)   # what every transcript of these tests observes first


@functools.lru_cache(maxsize=None)
def emu():
    """tests/emu/libemu_stark.so"""
    import eth_lc_plonky2_amd as m
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    D = c.POINTER(m.StarkDesc)
    return build_emu("emu_stark", (("emu_stark_words", U, [D]), ("emu_stark_next_leaf", U, [U, c.c_uint, c.c_uint]),
                                   ("emu_stark_quotient", c.c_int, [D, V, V, V, V]), ("emu_stark_check", c.c_int, [D, V, V, c.POINTER(m.StarkViolation)]),
                                   ("emu_stark_verify", c.c_int, [D, V, c.POINTER(m.binding.ChallengerState), V, U, c.POINTER(c.c_int)])))


# name -> (air, log_n, rate_bits, q, challenges, cap_height, pow bits, query rounds, arity schedule)
GPU_CASES = {
    "fib_n2": ("fibonacci", 1, 1, 0, 1, 0, 0, 2, []),
    "fib_n8": ("fibonacci", 3, 1, 1, 2, 2, 3, 3, [1, 1]),
    "fib_n32": ("fibonacci", 5, 3, 0, 4, 0, 4, 2, [2, 1]),
    "fib_crosses_workgroup": ("fibonacci", 9, 1, 1, 1, 2, 2, 2, [2, 2, 1]),
    "cubic_n2": ("cubic", 1, 3, 2, 2, 2, 0, 2, [1]),
    "cubic_n8": ("cubic", 3, 3, 2, 1, 0, 4, 4, [2]),
    "cubic_n32": ("cubic", 5, 3, 3, 2, 2, 2, 3, [1, 2]),
    "poseidon_n2": ("poseidon_round", 1, 3, 3, 1, 0, 2, 2, []),
    "poseidon_n8": ("poseidon_round", 3, 3, 3, 2, 2, 3, 2, [2, 1]),
    "poseidon_n32": ("poseidon_round", 5, 3, 3, 1, 2, 4, 2, [1, 1, 2]),
}


def shape(air_name, log_n, rate_bits, q, challenges, cap_height=0, pow_bits=0, queries=2, schedule=()):
    """the AIR, a satisfying trace with its public inputs, the config and the description"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    make_air, make_trace = stark.AIRS[air_name]
    air = make_air()
    trace, pis = make_trace(log_n)
    cfg = m.fri_config(log_n, rate_bits, cap_height, pow_bits, queries, 1, log_n, schedule=list(schedule))
    return SimpleNamespace(air=air, log_n=log_n, rate_bits=rate_bits, q=q, challenges=challenges, cfg=cfg, trace=trace,
                           pis=np.array(pis, dtype=np.uint64), desc=stark.pack_stark_desc(air, cfg, log_n, q, challenges))


@functools.lru_cache(maxsize=None)
def case(name):
    return shape(*GPU_CASES[name])


def model_challenger():
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = fo.Challenger()
    ch.observe(SEED)
    return ch


def lib_challenger():
    import eth_lc_plonky2_amd as m
    ch = m.binding.Challenger()
    ch.observe(SEED)
    return ch


def model_proof_of(s):
    """(proof, the transcript after it) from the model's prover"""
    from eth_lc_plonky2_amd import stark
    ch = model_challenger()
    proof = stark.prove(s.air, s.cfg, s.log_n, s.q, s.challenges, s.trace, s.pis, ch)
    return proof, ch.words()


@functools.lru_cache(maxsize=None)
def model_proof(name):
    proof, after = model_proof_of(case(name))
    proof.setflags(write=False)
    return proof, after


def model_verdict(s, proof, pis=None):
    from eth_lc_plonky2_amd import stark
    ch = model_challenger()
    return stark.verify(s.air, s.cfg, s.log_n, s.q, s.challenges, s.pis if pis is None else pis, ch, proof), ch.words()


def lib_verdict(s, proof, pis=None, desc=None):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = lib_challenger()
    return m.stark_verify(desc or s.desc, s.pis if pis is None else pis, ch.state, proof), fo.state_words(ch.state)


def emu_verdict(s, proof, pis=None, desc=None):
    """(status, failed check, transcript) from the portable verifier on the CPU"""
    from eth_lc_plonky2_amd import fri_openings as fo
    from rows_lib import vp
    ch = lib_challenger()
    failed = ctypes.c_int(0)
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    pis = np.ascontiguousarray(s.pis if pis is None else pis, dtype=np.uint64)
    rc = emu().emu_stark_verify(ctypes.byref(desc or s.desc), vp(pis), ctypes.byref(ch.state), vp(pr), pr.size, ctypes.byref(failed))
    return rc, failed.value, fo.state_words(ch.state)
