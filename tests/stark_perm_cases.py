"""What the tests of the STARK permutation argument share (test harness only): the CPU emulation tests/emu/emu_stark_perm.cpp, the
shapes, and per shape the AIR, its permutation, a satisfying trace, the descriptions for the C ABI and - computed once per process,
never changed - the model's proof."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np

import stark_cases as sc
from rows_lib import build_emu, vp

P = sc.P


@functools.lru_cache(maxsize=None)
def emu():
    """tests/emu/libemu_stark_perm.so"""
    import eth_lc_plonky2_amd as m
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    D, Q = c.POINTER(m.StarkDesc), c.POINTER(m.StarkPerm)
    return build_emu("emu_stark_perm", (("emu_stark_perm_words", U, [D, Q]), ("emu_stark_perm_problem", c.c_int, [D, Q, c.c_char_p, c.c_uint]),
                                        ("emu_stark_perm_columns", c.c_int, [D, Q, V, V, c.c_uint, V, V]),
                                        ("emu_stark_perm_quotient", c.c_int, [D, Q, V, V, V, V, V, V]),
                                        ("emu_stark_perm_verify", c.c_int, [D, Q, V, c.POINTER(m.binding.ChallengerState), V, U, c.POINTER(c.c_int)])))


# name -> (air, log_n, rate_bits, q, challenges, batch size, cap_height, pow bits, query rounds, arity schedule)
GPU_CASES = {
    "shuffle_n2": ("shuffle", 1, 1, 0, 1, 1, 0, 0, 2, []),
    "range_n8": ("range_check", 3, 1, 1, 2, 2, 2, 3, 3, [1, 1]),
    "tuples_n32": ("tuples", 5, 3, 2, 2, 4, 2, 2, 2, [2, 1]),   # 6 instances in 2 Z columns: the second batch is partial
    "range_crosses_workgroup": ("range_check", 9, 1, 1, 1, 1, 2, 2, 2, [2, 2, 1]),
}


def shape(air_name, log_n, rate_bits, q, challenges, batch, cap_height=0, pow_bits=0, queries=2, schedule=()):
    """the AIR, its permutation, a satisfying trace with its public inputs, the config and the descriptions"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import stark
    make_air, make_trace, make_perm = stark.PERM_AIRS[air_name]
    air, perm = make_air(), make_perm(batch)
    trace, pis = make_trace(log_n)
    cfg = m.fri_config(log_n, rate_bits, cap_height, pow_bits, queries, 1, log_n, schedule=list(schedule))
    return SimpleNamespace(air=air, perm=perm, log_n=log_n, rate_bits=rate_bits, q=q, challenges=challenges, batch=batch, cfg=cfg, trace=trace,
                           pis=np.array(pis, dtype=np.uint64), desc=stark.pack_stark_desc(air, cfg, log_n, q, challenges), sperm=stark.pack_stark_perm(perm))


@functools.lru_cache(maxsize=None)
def case(name):
    return shape(*GPU_CASES[name])


def flat_draws(sets):
    """the challenge sets as the words were drawn: per set, per challenge, beta then gamma"""
    return np.array([w for s in sets for pair in s for w in pair], dtype=np.uint64)


def model_proof_of(s, trace=None):
    from eth_lc_plonky2_amd import stark
    ch = sc.model_challenger()
    proof = stark.prove(s.air, s.cfg, s.log_n, s.q, s.challenges, s.trace if trace is None else trace, s.pis, ch, perm=s.perm)
    return proof, ch.words()


@functools.lru_cache(maxsize=None)
def model_proof(name):
    proof, after = model_proof_of(case(name))
    proof.setflags(write=False)
    return proof, after


def model_verdict(s, proof, pis=None):
    from eth_lc_plonky2_amd import stark
    ch = sc.model_challenger()
    return stark.verify(s.air, s.cfg, s.log_n, s.q, s.challenges, s.pis if pis is None else pis, ch, proof, perm=s.perm), ch.words()


def lib_verdict(s, proof, pis=None):
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = sc.lib_challenger()
    return m.stark_verify(s.desc, s.pis if pis is None else pis, ch.state, proof, perm=s.sperm), fo.state_words(ch.state)


def emu_verdict(s, proof, pis=None, desc=None, sperm=None, no_perm=False):
    """(status, failed check, transcript) from the portable verifier on the CPU"""
    from eth_lc_plonky2_amd import fri_openings as fo
    ch = sc.lib_challenger()
    failed = ctypes.c_int(0)
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    pis = np.ascontiguousarray(s.pis if pis is None else pis, dtype=np.uint64)
    perm = None if no_perm else ctypes.byref(sperm or s.sperm)
    rc = emu().emu_stark_perm_verify(ctypes.byref(desc or s.desc), perm, vp(pis), ctypes.byref(ch.state), vp(pr), pr.size, ctypes.byref(failed))
    return rc, failed.value, fo.state_words(ch.state)


def emu_problem(desc, sperm):
    """None, or the reason the description is refused for"""
    buf = ctypes.create_string_buffer(256)
    return buf.value.decode() if emu().emu_stark_perm_problem(ctypes.byref(desc), ctypes.byref(sperm) if sperm is not None else None, buf, 256) else None
