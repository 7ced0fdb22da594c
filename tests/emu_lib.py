"""Loads tests/emu/libemu.so and libemu_gates.so: CPU emulation of the device kernels' phases (test harness only), built by
rows_lib.build_emu."""
import ctypes as c

from rows_lib import build_emu

V = c.c_void_p


def load():
    return build_emu("emu", (
        ("emu_poseidon_permute", None, [V]), ("emu_poseidon_permute_grouped", None, [V]), ("emu_poseidon_partial_max_entry", c.c_uint32, []),
        ("emu_gl_mul", c.c_uint64, [c.c_uint64, c.c_uint64]), ("emu_gl_shl", c.c_uint64, [c.c_uint64, c.c_uint]),
        ("emu_ntt_forward", c.c_int, [V, V, c.c_uint32, c.c_uint32, c.c_uint64, c.c_uint32]),
        ("emu_ntt_inverse_natural", None, [V, V, c.c_uint32, c.c_uint32]), ("emu_ntt_inverse_bitrev", None, [V, V, c.c_uint32, c.c_uint32, c.c_uint64])))


def load_gates():
    """tests/emu/libemu_gates.so: the generated gate evaluators (csrc/generated_gates_*.hpp) and the walk of the two light native gates
    (csrc/light_gates.hpp) compiled for the CPU"""
    return build_emu("emu_gates", (
        ("emu_generated_count", c.c_uint, []), ("emu_generated_waves", c.c_uint, [c.c_uint]),
        ("emu_generated_gate", c.c_int, [c.c_uint, V, V, V, c.c_uint, c.c_uint64, V, V]),
        ("emu_light_walk", None, [c.c_uint, c.c_uint, V, c.c_uint, V, c.c_uint, c.c_uint64, V, V, V, V, V]),
        ("emu_gl_mul_u32", c.c_uint64, [c.c_uint64, c.c_uint32]), ("emu_gl_shl_nc", c.c_uint64, [c.c_uint64, c.c_uint])), opt="-O1")
