"""What the tests of the witness-row and verifier families share (test harness only): the one builder of the CPU emulations
tests/emu/<name>.cpp -> tests/emu/lib<name>.so, the constants of the row texts, a matrix and a record list in HBM, a gate's own
constraint program on one row, and the null-context walk of the entry points.  tools/*_probe.py build their emulation here too."""
import ctypes
import glob
import os
import subprocess

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
