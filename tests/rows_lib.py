"""What the tests of the witness-row and verifier families share (test harness only): the one builder of the CPU emulations
tests/emu/<name>.cpp -> tests/emu/lib<name>.so, the constants of the row texts, a plan's levels through the emulated launches and
the decode of its flag words, a matrix and a record list in HBM, a gate's own constraint program on one row, and the null-context
walk of the entry points.  tools/*_probe.py build their emulation here too."""
import ctypes
import glob
import os
import subprocess
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
P = 0xFFFFFFFF00000001
MAX = (1 << 64) - 1
INVALID = -1     # LCP2_E_INVALID
NW = 135
NONE = MAX       # a flag word while nothing is refused
TAG = MAX - 1    # not a canonical field element: no cell a job writes holds it


def build_emu(name, signatures, opt="-O2"):
    """tests/emu/lib<name>.so from tests/emu/<name>.cpp, with every (symbol, restype, argtypes) of `signatures` bound.  Rebuilt when
    any source under tests/emu/, any csrc/*.hpp or include/*.h is newer: nobody lists the headers a harness reaches, so none can be
    forgotten (too many rebuilds cost seconds, one too few tests old code)."""
    src, lib = os.path.join(EMU, name + ".cpp"), os.path.join(EMU, "lib" + name + ".so")
    deps = [f for f in glob.glob(os.path.join(EMU, "*")) if not f.endswith((".so", ".tmp"))]
    deps += glob.glob(os.path.join(ROOT, "eth-lc-plonky2_amd", "csrc", "*.hpp")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.run(["g++", opt, "-std=c++17", "-fPIC", "-shared", "-o", lib + ".tmp", src], check=True)
        os.replace(lib + ".tmp", lib)
    E = ctypes.CDLL(lib)
    for symbol, restype, argtypes in signatures:
        getattr(E, symbol).restype, getattr(E, symbol).argtypes = restype, argtypes
    return E


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ a plan's levels through tests/emu/emu_plan.cpp
def emu_plan():
    """tests/emu/libemu_plan.so"""
    c, V, U = ctypes, ctypes.c_void_p, ctypes.c_uint64
    return build_emu("emu_plan", (("emu_plan_pos_job_bytes", c.c_uint, []), ("emu_plan_operand_bytes", c.c_uint, []), ("emu_plan_pos_operands", c.c_uint, []),
                                  ("emu_plan_problem_str", c.c_char_p, [c.c_uint]), ("emu_plan_pos_problem", c.c_uint, [V, c.c_int, V, U, c.c_uint, U]),
                                  ("emu_plan_lists_problem", c.c_uint, [V, U, V, V, U, V, U, c.c_uint, U, V, V]),
                                  ("emu_plan_level", None, [V, U, U, V, U, V, U, U, V, U, V, c.c_uint, U, V, U, c.c_uint]),
                                  ("emu_plan_refusal", c.c_uint, [V, V, U, V, V])))


def vpn(a):
    """(an empty list of a plan goes in as a null pointer)"""
    return vp(a) if a.size else None


def rec_plan(jobs, operands, level_ends):
    """the witness plan a rec-gate call is: these rec jobs, no PoseidonGate job, no chain"""
    none = np.zeros(0, dtype=np.uint32)
    return SimpleNamespace(rec_jobs=jobs, pos_jobs=none, chain_ends=none, operands=operands, rec_level_ends=np.asarray(level_ends, dtype=np.uint32),
                           pos_level_ends=np.zeros(len(level_ends), dtype=np.uint32))


def run_levels(E, plan, n, start=None, order=None, threads=64):
    """the plan through the emulated launches, level by level (`order`: these levels, in this order): (matrix, the two flag words)"""
    got = np.zeros((NW, n), dtype=np.uint64) if start is None else start.copy()
    flags = np.full(2, NONE, dtype=np.uint64)
    rec_ends, pos_ends = [0] + plan.rec_level_ends.tolist(), [0] + plan.pos_level_ends.tolist()
    for l in (range(len(rec_ends) - 1) if order is None else order):
        E.emu_plan_level(vpn(plan.rec_jobs), rec_ends[l], rec_ends[l + 1], vpn(plan.pos_jobs), plan.pos_jobs.size, vpn(plan.chain_ends), pos_ends[l],
                         pos_ends[l + 1], vpn(plan.operands), plan.operands.size, vp(got), NW, n, vp(flags), l, threads)
    return got, [int(f) for f in flags]


def refusal(E, flags, plan):
    """(family, job, reason code) the two flag words name, as the entry points decode them; None while nothing is refused"""
    family, job = ctypes.c_uint(0), ctypes.c_uint64(0)
    code = E.emu_plan_refusal(vp(np.array(flags, dtype=np.uint64)), vpn(plan.rec_level_ends), plan.rec_level_ends.size, ctypes.byref(family), ctypes.byref(job))
    return (("rec", "poseidon")[family.value], job.value, code) if code else None


def gate_constraints(gs, name, row, consts):
    """the constraints the gate's own program emits on one row"""
    import gate_program_ref as ref
    g = gs.gates[gs.index(name)]
    code = gs.code[2 * g.code_offset:2 * (g.code_offset + g.code_len)]
    emitted = ref.emitted_constraints(code, gs.imm, row, consts, None)
    assert len(emitted) == g.num_constraints
    return emitted


def check_null_context(call, lists, mems=(None,), null_wires=None):
    """without a device there is no context, and the null check of an entry point comes first: call(arguments, mem, wires) with a
    null context is LCP2_E_INVALID whatever the `lists` hold (valid jobs, refused ones, nothing), for every lcp2_mem, also for
    `null_wires` (a null list with a non-zero count, and a null matrix) - never a crash or another status, and nothing is written"""
    buf = np.zeros(NW * 64, dtype=np.uint64)
    for mem in mems:
        for arguments in lists:
            assert call(arguments, mem, vp(buf)) == INVALID, arguments
        if null_wires is not None:
            assert call(null_wires, mem, None) == INVALID
    assert not buf.any()


class DeviceMatrix:
    """a [columns][n] matrix in HBM"""

    def __init__(self, ctx, host):
        self.ctx, self.shape = ctx, host.shape
        self.ptr = ctx.buffer_alloc(host.size)
        ctx.buffer_write(self.ptr, host)

    def read(self):
        return self.ctx.buffer_read(self.ptr, self.shape[0] * self.shape[1]).reshape(self.shape)

    def free(self):
        self.ctx.buffer_free(self.ptr)


def upload(ctx, records):
    """records of 4, 8, 16 or 24 bytes -> a device pointer (padded to whole words)"""
    raw = np.frombuffer(np.ascontiguousarray(records).tobytes() + b"\0" * (-records.nbytes % 8), dtype=np.uint64)
    ptr = ctx.buffer_alloc(max(raw.size, 1))
    if raw.size:
        ctx.buffer_write(ptr, raw)
    return ptr
