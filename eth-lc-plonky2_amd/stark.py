"""AIR proofs over the openings of bare oracles (lcp2_stark_prove / lcp2_stark_verify): an independent model over Python integers,
on top of the model of the opening layer (fri_openings.py) - the proof layout, the witness check, the verifier and, for small
shapes, the prover, written from the definitions in include/lcp2.h: the constraints of first_row, transition and last_row as one
list, per challenge the Horner pass acc <- acc alpha + f(c) c with the filters L_first, X - g^-1, L_last, the quotient acc / Z_H on
the coset 7 H_{2^q n}, its chunks, and the identity at zeta.  The next row of a coset point x is found as the point g x itself, not by
an index formula.  No arithmetic is shared with csrc/stark.hpp.  Also here: an assembler for the constraint programs, three sample
AIRs with their traces, and pack_stark_desc for the C ABI.

Permutation arguments (lcp2_stark_prove_perm / lcp2_stark_verify_perm; starky's permutation_pairs): a Permutation lists pairs of
column tuples and a batch size B; every function that takes perm= then follows the extended protocol - B challenge sets of
(beta, gamma) pairs after the trace cap, the grand-product columns Z as a second oracle between the trace and the quotient, the
constraints Z - 1 on the first row and Z(next) prod rhs - Z prod lhs on ALL rows behind the AIR's list, Z opened at zeta and g zeta.
perm_z_columns computes the Z columns for whole traces at once; three more sample AIRs (PERM_AIRS) use the argument."""
import ctypes
from types import SimpleNamespace

import numpy as np

from . import fri_openings as fo
from . import poseidon_py

P = fo.P
OP_ADD, OP_SUB, OP_MUL, OP_EMIT, OP_XOR, OP_DBLADD, OP_EMITBOOL, OP_MULADD, OP_SBOX, OP_PMDS = range(10)
REG, WIRE, CONST, IMM, PI = range(5)
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8] + [0] * 11
KINDS = ("first_row", "transition", "last_row")
CHECKS = {**fo.CHECKS, 8: "non-canonical cap word", 9: "quotient identity"}
KIND_PERM = 3   # the kind of a violation of the permutation argument: the running product of a Z column does not close


# ------------------------------------------------------------------ programs
def insn(op, dst=0, a=(REG, 0), b=(REG, 0)):
    """the two words of one instruction; a, b = (kind, index)"""
    return [op | dst << 8 | a[0] << 16 | b[0] << 20, a[1] | b[1] << 16]


class Air:
    """width, num_public_inputs, num_regs, the code words, the immediates and per kind (code_offset, code_len, num_constraints)"""

    def __init__(self, name, width, num_public_inputs, num_regs, programs, imm=()):
        self.name, self.width, self.num_public_inputs, self.num_regs, self.imm = name, width, num_public_inputs, num_regs, [int(v) for v in imm]
        self.code, self.programs = [], []
        for prog in programs:   # each a list of instructions
            words = [w for i in prog for w in i]
            emits = sum(1 for i in prog if i[0] & 0xF in (OP_EMIT, OP_EMITBOOL))
            self.programs.append((len(self.code) // 2, len(prog), emits))
            self.code += words

    def local(self, j):
        return (WIRE, j)

    def next(self, j):
        return (WIRE, self.width + j)


def emitted(air, kind, local, nxt, pis, F):
    """the constraints of one program in program order over the field F (BASE or EXT); local / nxt: the two rows"""
    first, length, _ = air.programs[kind]
    reg, out = [F.zero] * (air.num_regs + 12), []

    def operand(k, i):
        if k == REG:
            return reg[i]
        if k == WIRE:
            return local[i] if i < air.width else nxt[i - air.width]
        if k == IMM:
            return F.const(air.imm[i])
        assert k == PI
        return F.const(pis[i])

    for pc in range(first, first + length):
        w0, w1 = air.code[2 * pc], air.code[2 * pc + 1]
        op, dst, ka, kb, ia, ib = w0 & 0xF, (w0 >> 8) & 0xFF, (w0 >> 16) & 0xF, (w0 >> 20) & 0xF, w1 & 0xFFFF, w1 >> 16
        if op == OP_PMDS:
            src = reg[ia:ia + 12]
            for r in range(12):
                t = F.const(air.imm[ib + r])
                t = F.add(t, F.mul(src[r], F.const(MDS_DIAG[r])))
                for i in range(12):
                    t = F.add(t, F.mul(src[(i + r) % 12], F.const(MDS_CIRC[i])))
                reg[dst + r] = t
            continue
        x = operand(ka, ia)
        if op == OP_EMIT:
            out.append(x)
        elif op == OP_EMITBOOL:
            out.append(F.sub(F.mul(x, x), x))
        elif op == OP_SBOX:
            x2 = F.mul(x, x)
            reg[dst] = F.mul(F.mul(F.mul(x2, x2), x2), x)
        else:
            y = operand(kb, ib)
            if op == OP_ADD:
                reg[dst] = F.add(x, y)
            elif op == OP_SUB:
                reg[dst] = F.sub(x, y)
            elif op == OP_MUL:
                reg[dst] = F.mul(x, y)
            elif op == OP_XOR:
                xy = F.mul(x, y)
                reg[dst] = F.sub(F.sub(F.add(x, y), xy), xy)
            elif op == OP_DBLADD:
                reg[dst] = F.add(F.add(x, x), y)
            else:
                assert op == OP_MULADD
                reg[dst] = F.add(reg[dst], F.mul(x, y))
    return out


BASE = SimpleNamespace(zero=0, const=lambda v: int(v) % P, add=lambda a, b: (a + b) % P, sub=lambda a, b: (a - b) % P, mul=lambda a, b: a * b % P)
EXT = SimpleNamespace(zero=(0, 0), const=lambda v: (int(v) % P, 0), add=fo.e_add, sub=fo.e_sub, mul=fo.e_mul)


def program_degree(air, kind):
    """the degree bound of a program in the columns: a column 1, a sum the larger, a product the sum"""
    D = SimpleNamespace(zero=0, const=lambda v: 0, add=max, sub=max, mul=lambda a, b: a + b)
    got = emitted(air, kind, [1] * air.width, [1] * air.width, [0] * max(air.num_public_inputs, 1), D)
    return max(got) if got else 0


# ------------------------------------------------------------------ the three sample AIRs
def fibonacci_air():
    """width 2 (a, b): next a = b, next b = a + b; public inputs x0, x1 and the last row's b"""
    A = Air
    first = [insn(OP_SUB, 0, (WIRE, 0), (PI, 0)), insn(OP_EMIT, 0, (REG, 0)), insn(OP_SUB, 0, (WIRE, 1), (PI, 1)), insn(OP_EMIT, 0, (REG, 0))]
    trans = [insn(OP_SUB, 0, (WIRE, 2), (WIRE, 1)), insn(OP_EMIT, 0, (REG, 0)),
             insn(OP_ADD, 0, (WIRE, 0), (WIRE, 1)), insn(OP_SUB, 0, (WIRE, 3), (REG, 0)), insn(OP_EMIT, 0, (REG, 0))]
    last = [insn(OP_SUB, 0, (WIRE, 1), (PI, 2)), insn(OP_EMIT, 0, (REG, 0))]
    return A("fibonacci", 2, 3, 1, [first, trans, last])


def fibonacci_trace(log_n, x0=1, x1=1):
    n = 1 << log_n
    t = np.zeros((2, n), dtype=np.uint64)
    a, b = x0 % P, x1 % P
    for i in range(n):
        t[0, i], t[1, i] = a, b
        a, b = b, (a + b) % P
    return t, [x0 % P, x1 % P, int(t[1, n - 1])]


CUBIC_C = 0x123456789ABCDEF


def cubic_air():
    """width 3 (x, y, b): next x = x^3 + y c, next y = 2 y + b, next b = 1 - b (as b XOR 1), b boolean; degree 3.  Public inputs
    x0, y0 and x + y of the last row; b starts at 0."""
    first = [insn(OP_SUB, 0, (WIRE, 0), (PI, 0)), insn(OP_EMIT, 0, (REG, 0)), insn(OP_SUB, 0, (WIRE, 1), (PI, 1)), insn(OP_EMIT, 0, (REG, 0)),
             insn(OP_EMIT, 0, (WIRE, 2))]
    trans = [insn(OP_MUL, 0, (WIRE, 0), (WIRE, 0)), insn(OP_MUL, 1, (REG, 0), (WIRE, 0)), insn(OP_MULADD, 1, (WIRE, 1), (IMM, 0)),
             insn(OP_SUB, 2, (WIRE, 3), (REG, 1)), insn(OP_EMIT, 0, (REG, 2)),
             insn(OP_DBLADD, 0, (WIRE, 1), (WIRE, 2)), insn(OP_SUB, 0, (WIRE, 4), (REG, 0)), insn(OP_EMIT, 0, (REG, 0)),
             insn(OP_XOR, 0, (WIRE, 2), (IMM, 1)), insn(OP_SUB, 0, (WIRE, 5), (REG, 0)), insn(OP_EMIT, 0, (REG, 0)),
             insn(OP_EMITBOOL, 0, (WIRE, 2))]
    last = [insn(OP_ADD, 0, (WIRE, 0), (WIRE, 1)), insn(OP_SUB, 0, (REG, 0), (PI, 2)), insn(OP_EMIT, 0, (REG, 0)), insn(OP_EMITBOOL, 0, (WIRE, 2))]
    return Air("cubic", 3, 3, 3, [first, trans, last], imm=[CUBIC_C, 1])


def cubic_trace(log_n, x0=3, y0=5):
    n = 1 << log_n
    t = np.zeros((3, n), dtype=np.uint64)
    x, y, b = x0 % P, y0 % P, 0
    for i in range(n):
        t[0, i], t[1, i], t[2, i] = x, y, b
        x, y, b = (pow(x, 3, P) + y * CUBIC_C) % P, (2 * y + b) % P, 1 - b
    return t, [x0 % P, y0 % P, (int(t[0, n - 1]) + int(t[1, n - 1])) % P]


POSEIDON_RC = [(0x9E3779B97F4A7C15 * (j + 1)) % P for j in range(12)]


def poseidon_round_air():
    """width 12: the next row is the MDS layer (plus the 12 immediates) of the S-boxes of the local row; degree 7.  Public inputs:
    the first row, then the last row."""
    first = [i for j in range(12) for i in (insn(OP_SUB, 12, (WIRE, j), (PI, j)), insn(OP_EMIT, 0, (REG, 12)))]
    trans = [insn(OP_SBOX, j, (WIRE, j)) for j in range(12)] + [insn(OP_PMDS, 0, (REG, 0), (IMM, 0))]
    trans += [i for j in range(12) for i in (insn(OP_SUB, 12, (WIRE, 12 + j), (REG, j)), insn(OP_EMIT, 0, (REG, 12)))]
    last = [i for j in range(12) for i in (insn(OP_SUB, 12, (WIRE, j), (PI, 12 + j)), insn(OP_EMIT, 0, (REG, 12)))]
    return Air("poseidon_round", 12, 24, 13, [first, trans, last], imm=POSEIDON_RC)


def poseidon_round_trace(log_n, seed=1):
    n = 1 << log_n
    t = np.zeros((12, n), dtype=np.uint64)
    state = [(seed * 0x1000003 + 17 * j + 1) % P for j in range(12)]
    for i in range(n):
        t[:, i] = state
        s = [pow(v, 7, P) for v in state]
        state = [(sum(s[(k + r) % 12] * MDS_CIRC[k] for k in range(12)) + s[r] * MDS_DIAG[r] + POSEIDON_RC[r]) % P for r in range(12)]
    return t, [int(v) for v in t[:, 0]] + [int(v) for v in t[:, n - 1]]


AIRS = {"fibonacci": (fibonacci_air, fibonacci_trace), "cubic": (cubic_air, cubic_trace), "poseidon_round": (poseidon_round_air, poseidon_round_trace)}


# ------------------------------------------------------------------ sample AIRs with a permutation argument
def _shuffled(n, mul, add):
    """row i of the rhs holds row (mul i + add) mod n of the lhs (mul odd: a bijection)"""
    return [(mul * i + add) % n for i in range(n)]


def shuffle_air():
    """width 2, no constraints of its own: column 1 is a permutation of column 0"""
    return Air("shuffle", 2, 0, 0, [[], [], []])


def shuffle_trace(log_n, seed=5):
    n = 1 << log_n
    t = np.zeros((2, n), dtype=np.uint64)
    for i in range(n):
        t[0, i] = (seed * 0x9E3779B97F4A7C15 + i * i * 0x1000003 + 3 * i + 1) % P
    t[1] = t[0][_shuffled(n, 5, 3)]
    return t, []


def shuffle_perm(batch_size=1):
    return Permutation([[(0, 1)]], batch_size)


def range_check_air():
    """width 2 (a, b): b is a sorted - a permutation of a (the argument) that starts at public input 0, ends at public input 1 and
    grows by 0 or 1 per row: (b' - b)(b' - b - 1) = 0.  Every a then lies in [pi_0, pi_1].  Degree 2."""
    first = [insn(OP_SUB, 0, (WIRE, 1), (PI, 0)), insn(OP_EMIT, 0, (REG, 0))]
    trans = [insn(OP_SUB, 0, (WIRE, 3), (WIRE, 1)), insn(OP_SUB, 1, (REG, 0), (IMM, 0)), insn(OP_MUL, 0, (REG, 0), (REG, 1)), insn(OP_EMIT, 0, (REG, 0))]
    last = [insn(OP_SUB, 0, (WIRE, 1), (PI, 1)), insn(OP_EMIT, 0, (REG, 0))]
    return Air("range_check", 2, 2, 2, [first, trans, last], imm=[1])


def range_check_trace(log_n, lo=1000):
    n = 1 << log_n
    t = np.zeros((2, n), dtype=np.uint64)
    for i in range(n):
        t[1, i] = lo + (3 * i) // 4
    t[0] = t[1][_shuffled(n, 5, 3)]
    return t, [int(t[1, 0]), int(t[1, n - 1])]


def range_check_perm(batch_size=1):
    return Permutation([[(0, 1)]], batch_size)


def tuples_air():
    """width 12, no constraints of its own: three pairs of 1, 2 and 3 columns - the rows of columns (0), (1, 2), (3, 4, 5) are
    permutations, each its own, of the rows of columns (6), (7, 8), (9, 10, 11)"""
    return Air("tuples", 12, 0, 0, [[], [], []])


def tuples_trace(log_n, seed=9):
    n = 1 << log_n
    t = np.zeros((12, n), dtype=np.uint64)
    for c in range(6):
        for i in range(n):
            t[c, i] = (seed * 0x9E3779B97F4A7C15 + (c + 1) * 0x123456789 * (i + 1) + i * i) % P
    t[6] = t[0][_shuffled(n, 3, 1)]
    t[7:9] = t[1:3][:, _shuffled(n, 5, 0)]
    t[9:12] = t[3:6][:, _shuffled(n, 7, 5)]
    return t, []


def tuples_perm(batch_size=1):
    return Permutation([[(0, 6)], [(1, 7), (2, 8)], [(3, 9), (4, 10), (5, 11)]], batch_size)


# name -> (air, trace, permutation(batch_size))
PERM_AIRS = {"shuffle": (shuffle_air, shuffle_trace, shuffle_perm), "range_check": (range_check_air, range_check_trace, range_check_perm),
             "tuples": (tuples_air, tuples_trace, tuples_perm)}


# ------------------------------------------------------------------ permutation arguments
class Permutation:
    """pairs: per pair the list of its (lhs column, rhs column); batch_size: B, the instances multiplied into one Z"""

    def __init__(self, pairs, batch_size):
        self.pairs, self.batch_size = [[(int(l), int(r)) for l, r in pair] for pair in pairs], int(batch_size)

    def instances(self, num_challenges):
        """the ordered list of (pair, challenge): pair major"""
        return [(p, c) for p in range(len(self.pairs)) for c in range(num_challenges)]

    def num_z(self, num_challenges):
        return -(-len(self.pairs) * num_challenges // self.batch_size)

    def batches(self, num_challenges):
        """per Z column the list of its (pair, challenge, position in the batch)"""
        inst, B = self.instances(num_challenges), self.batch_size
        return [[(p, c, i) for i, (p, c) in enumerate(inst[z * B:(z + 1) * B])] for z in range(self.num_z(num_challenges))]


def _on(perm):
    return perm is not None and len(perm.pairs) > 0


def pack_stark_perm(perm):
    """the lcp2_stark_perm of a Permutation; the pair and column arrays live in the result"""
    from .binding import StarkPerm
    sp = StarkPerm()
    runs, cols = [], []
    for pair in perm.pairs:
        runs += [len(cols), len(pair)]
        cols += list(pair)
    sp._pairs = np.array(runs if runs else [0, 0], dtype=np.uint32)
    sp._columns = np.array(cols if cols else [(0, 0)], dtype=np.uint32).reshape(-1, 2)
    sp.num_pairs, sp.pairs, sp.columns, sp.num_column_pairs, sp.batch_size = len(perm.pairs), sp._pairs.ctypes.data, sp._columns.ctypes.data, len(cols), perm.batch_size
    return sp


def draw_challenge_sets(perm, num_challenges, challenger):
    """B sets of num_challenges (beta, gamma): set 0 first, inside a set beta then gamma per challenge"""
    sets = []
    for _ in range(perm.batch_size):
        sets.append([])
        for _ in range(num_challenges):
            beta = challenger.get()
            sets[-1].append((beta, challenger.get()))
    return sets


def perm_products(perm, batch, challenge_sets, row, F):
    """(prod lhs, prod rhs) over the instances of one Z column on one row (row[column], elements of F)"""
    num, den = F.const(1), F.const(1)
    for p, c, i in batch:
        beta, gamma = challenge_sets[i][c]
        lhs, rhs, power = F.const(gamma), F.const(gamma), F.const(1)
        for l, r in perm.pairs[p]:
            lhs, rhs = F.add(lhs, F.mul(power, row[l])), F.add(rhs, F.mul(power, row[r]))
            power = F.mul(power, F.const(beta))
        num, den = F.mul(num, lhs), F.mul(den, rhs)
    return num, den


def perm_ratios(trace, perm, challenge_sets):
    """[numZ][n] (numpy object arrays of Python integers): prod lhs / prod rhs per row, whole columns at a time; the inverse of 0 is 0"""
    num_challenges = len(challenge_sets[0])
    cols = [np.array([int(v) % P for v in col], dtype=object) for col in trace]
    inverse = np.frompyfunc(lambda v: pow(v, P - 2, P), 1, 1)
    out = []
    for batch in perm.batches(num_challenges):
        num, den = 1, 1
        for p, c, i in batch:
            beta, gamma = challenge_sets[i][c]
            lhs, rhs, power = gamma, gamma, 1
            for l, r in perm.pairs[p]:
                lhs, rhs, power = (lhs + power * cols[l]) % P, (rhs + power * cols[r]) % P, power * beta % P
            num, den = num * lhs % P, den * rhs % P
        out.append(num * inverse(den) % P)
    return out


def perm_z_columns(trace, perm, challenge_sets):
    """the grand-product columns [numZ][n] (uint64): Z[0] = 1, Z[r + 1] = Z[r] ratio[r]"""
    n = len(trace[0])
    out = np.zeros((perm.num_z(len(challenge_sets[0])), n), dtype=np.uint64)
    for z, ratio in enumerate(perm_ratios(trace, perm, challenge_sets)):
        acc = 1
        for r in range(n):
            out[z, r] = acc
            acc = acc * ratio[r] % P
    return out


def perm_open_z(trace, perm, challenge_sets):
    """None, or the smallest z whose running product does not return to 1 after row n - 1"""
    zs, n = perm_z_columns(trace, perm, challenge_sets), len(trace[0])
    for z, ratio in enumerate(perm_ratios(trace, perm, challenge_sets)):
        if int(zs[z, n - 1]) * ratio[n - 1] % P != 1:
            return z
    return None


# ------------------------------------------------------------------ description, layout
def instance_of(air, num_challenges, q, perm=None):
    """(oracle_cols, points_ranges) of the opening instance: zeta: all trace and quotient columns; g zeta: all trace columns.  With
    a permutation the Z columns are oracle 1, opened at both points, and the quotient is oracle 2"""
    if _on(perm):
        cols = [air.width, perm.num_z(num_challenges), num_challenges << q]
        return cols, [[(0, 0, cols[0]), (1, 0, cols[1]), (2, 0, cols[2])], [(0, 0, cols[0]), (1, 0, cols[1])]]
    cols = [air.width, num_challenges << q]
    return cols, [[(0, 0, cols[0]), (1, 0, cols[1])], [(0, 0, cols[0])]]


def layout(air, cfg, log_n, q, num_challenges, perm=None):
    cols, pr = instance_of(air, num_challenges, q, perm)
    L = fo.layout(cfg, log_n, cols, pr)
    capw, num_z = 4 << cfg.cap_height, cols[1] if _on(perm) else 0
    caps = len(cols) * capw
    return SimpleNamespace(fo=L, capw=capw, trace_cap=0, z_cap=capw if num_z else None, quot_cap=caps - capw, openings=caps, op_local=caps,
                           op_z=caps + 2 * air.width, op_quotient=caps + 2 * air.width + 2 * num_z, op_next=caps + L.point_off[1],
                           op_z_next=caps + L.point_off[1] + 2 * air.width, Q=1 << q, num_z=num_z, total=caps + L.total, cols=cols, points_ranges=pr)


def sections(L):
    """(name, first word, words) of every section of the proof"""
    caps = [("trace_cap", 0, L.capw)] + ([("z_cap", L.z_cap, L.capw)] if L.num_z else []) + [("quotient_cap", L.quot_cap, L.capw)]
    return caps + [(name, L.openings + first, words) for name, first, words in fo.sections(L.fo)]


def pack_stark_desc(air, cfg, log_n, q, num_challenges):
    """the lcp2_stark_desc of an Air; the code and immediate arrays live in the result"""
    from .binding import StarkDesc, StarkProgram
    d = StarkDesc()
    d.log_n, d.width, d.num_public_inputs, d.num_challenges, d.quotient_degree_bits = log_n, air.width, air.num_public_inputs, num_challenges, q
    ctypes.memmove(ctypes.byref(d.fri), ctypes.byref(cfg), ctypes.sizeof(cfg))
    d.first_row, d.transition, d.last_row = (StarkProgram(*p) for p in air.programs)
    d._code = np.array(air.code if air.code else [0, 0], dtype=np.uint32)
    d._imm = np.array(air.imm if air.imm else [0], dtype=np.uint64)
    d.code, d.code_words, d.imm, d.num_imm, d.num_regs = d._code.ctypes.data, len(air.code), d._imm.ctypes.data, len(air.imm), air.num_regs
    return d


# ------------------------------------------------------------------ the witness check
def check_trace(air, trace, pis, perm=None, challenge_sets=None):
    """None, or (kind, constraint, row) of the violation with the smallest (row, index in the list).  With a permutation and its
    challenge sets: behind the AIR's own check, (3, z, n - 1) for the smallest Z column whose running product does not close"""
    n = len(trace[0])
    rows = [[int(trace[c][i]) % P for c in range(air.width)] for i in range(n)]
    for i in range(n):
        for kind in range(3):
            if (kind == 0 and i != 0) or (kind == 1 and i == n - 1) or (kind == 2 and i != n - 1):
                continue
            for k, v in enumerate(emitted(air, kind, rows[i], rows[(i + 1) % n], pis, BASE)):
                if v:
                    return kind, k, i
    if _on(perm) and challenge_sets is not None:
        z = perm_open_z(trace, perm, challenge_sets)
        if z is not None:
            return KIND_PERM, z, n - 1
    return None


# ------------------------------------------------------------------ transforms over Python integers
def _ntt(a, w):
    """[sum_j a[j] w^(j k)] for k < len(a), w a primitive len(a)-th root"""
    n = len(a)
    if n == 1:
        return list(a)
    w2 = w * w % P
    even, odd = _ntt(a[0::2], w2), _ntt(a[1::2], w2)
    out, t = [0] * n, 1
    for k in range(n // 2):
        o = odd[k] * t % P
        out[k], out[k + n // 2] = (even[k] + o) % P, (even[k] - o) % P
        t = t * w % P
    return out


def interpolate(values):
    """coefficients of the polynomial with these values on H in natural order"""
    n = len(values)
    lg = n.bit_length() - 1
    inv = pow(n, P - 2, P)
    return [v * inv % P for v in _ntt([int(v) % P for v in values], pow(fo.root_of_unity(lg), P - 2, P))]


def coset_values(coeffs, lg, shift=fo.GENERATOR):
    """values on shift H_{2^lg} in leaf order: out[i] = C(shift w^bitrev(i))"""
    a, s = [0] * (1 << lg), 1
    for j, c in enumerate(coeffs):
        a[j] = int(c) * s % P
        s = s * shift % P
    v = _ntt(a, fo.root_of_unity(lg))
    return [v[fo.bitrev(i, lg)] for i in range(1 << lg)]


def coset_interpolate(leaf_values, lg, shift=fo.GENERATOR):
    """the inverse of coset_values"""
    v = [leaf_values[fo.bitrev(k, lg)] for k in range(1 << lg)]
    inv, sinv = pow(1 << lg, P - 2, P), pow(shift, P - 2, P)
    c, out, s = _ntt(v, pow(fo.root_of_unity(lg), P - 2, P)), [], inv
    for x in c:
        out.append(x * s % P)
        s = s * sinv % P
    return out


def commit(coeff_cols, log_n, rate_bits, cap_height):
    """fri_openings.commit with the transform above: (leaves in leaf order, Merkle levels)"""
    vals = [coset_values(col, log_n + rate_bits) for col in coeff_cols]
    leaves = [[v[i] for v in vals] for i in range(1 << (log_n + rate_bits))]
    return leaves, fo.merkle_tree(leaves, cap_height)


def cap_of(oracle):
    return [w for d in oracle[1][-1] for w in d]


# ------------------------------------------------------------------ quotient, prover, verifier
def filters(x, log_n, F):
    """(L_first(x), x - g^-1, L_last(x), Z_H(x)) over the field F, x an element of F"""
    n = 1 << log_n
    g_inv, n_inv = pow(fo.root_of_unity(log_n), P - 2, P), pow(n, P - 2, P)
    xn = x
    for _ in range(log_n):
        xn = F.mul(xn, xn)
    zh = F.sub(xn, F.const(1))
    inv = (lambda v: pow(v, P - 2, P)) if F is BASE else fo.e_inv
    first = F.mul(F.mul(zh, inv(F.sub(x, F.const(1)))), F.const(n_inv))
    last = F.mul(F.mul(zh, inv(F.sub(x, F.const(g_inv)))), F.const(n_inv * g_inv))
    return first, F.sub(x, F.const(g_inv)), last, zh


def vanishing(air, log_n, x, local, nxt, pis, alphas, F, perm=None, challenge_sets=None, z_local=None, z_next=None):
    """per challenge the Horner pass over the list of filtered constraints, and Z_H(x).  With a permutation the list goes on with
    Z_z - 1 under L_first for every z, then Z_z(next) prod rhs - Z_z prod lhs for every z with no filter (z_local, z_next: the Z
    columns at x and at g x)"""
    f = filters(x, log_n, F)
    acc = [F.zero] * len(alphas)

    def push(fc):
        return [F.add(F.mul(a, F.const(al)), fc) for a, al in zip(acc, alphas)]

    for kind in range(3):
        for c in emitted(air, kind, local, nxt, pis, F):
            acc = push(F.mul(f[kind], c))
    if _on(perm):
        for z in range(len(z_local)):
            acc = push(F.mul(f[0], F.sub(z_local[z], F.const(1))))
        for z, batch in enumerate(perm.batches(len(alphas))):
            num, den = perm_products(perm, batch, challenge_sets, local, F)
            acc = push(F.sub(F.mul(z_next[z], den), F.mul(z_local[z], num)))
    return acc, f[3]


def quotient_values(air, log_n, rate_bits, q, trace_leaves, pis, alphas, perm=None, challenge_sets=None, z_leaves=None):
    """[num_challenges][2^q n] values of the quotient on the first 2^q n leaves of the trace LDE (trace_leaves[i] = the leaf of
    width values at leaf i; z_leaves likewise for the Z columns of a permutation); the next row of a point x is the leaf whose
    point is g x"""
    lgN, M = log_n + rate_bits, 1 << (log_n + q)
    w, g = fo.root_of_unity(lgN), fo.root_of_unity(log_n)
    xs = [fo.GENERATOR * pow(w, fo.bitrev(i, lgN), P) % P for i in range(1 << lgN)]
    at = {x: i for i, x in enumerate(xs)}
    out = [[0] * M for _ in alphas]
    for i in range(M):
        nx = at[xs[i] * g % P]
        acc, zh = vanishing(air, log_n, xs[i], trace_leaves[i], trace_leaves[nx], pis, alphas, BASE, perm, challenge_sets,
                            z_leaves[i] if z_leaves else None, z_leaves[nx] if z_leaves else None)
        zinv = pow(zh, P - 2, P)
        for c, a in enumerate(acc):
            out[c][i] = a * zinv % P
    return out


def prove(air, cfg, log_n, q, num_challenges, trace, pis, challenger, perm=None):
    """the proof words (numpy); the challenger ends as the opening layer leaves it.  ValueError((kind, constraint, row)) for a
    trace that violates a constraint (the challenger is a copy's then: the caller's is untouched)"""
    bad = check_trace(air, trace, pis)
    if bad is not None:
        raise ValueError(bad)
    L = layout(air, cfg, log_n, q, num_challenges, perm)
    n, ch = 1 << log_n, fo.Challenger()
    ch.sponge, ch.inp, ch.out = challenger.words()
    pis = [int(v) % P for v in pis]
    trace_coeffs = [interpolate(trace[c]) for c in range(air.width)]
    trace_oracle = commit(trace_coeffs, log_n, cfg.rate_bits, cfg.cap_height)
    ch.observe(pis)
    ch.observe(cap_of(trace_oracle))
    coeffs, oracles, sets, z_leaves = [trace_coeffs], [trace_oracle], None, None
    if _on(perm):
        sets = draw_challenge_sets(perm, num_challenges, ch)
        z = perm_open_z(trace, perm, sets)
        if z is not None:
            raise ValueError((KIND_PERM, z, n - 1))
        z_coeffs = [interpolate(col) for col in perm_z_columns(trace, perm, sets)]
        z_oracle = commit(z_coeffs, log_n, cfg.rate_bits, cfg.cap_height)
        ch.observe(cap_of(z_oracle))
        coeffs.append(z_coeffs)
        oracles.append(z_oracle)
        z_leaves = z_oracle[0]
    alphas = [ch.get() for _ in range(num_challenges)]
    qv = quotient_values(air, log_n, cfg.rate_bits, q, trace_oracle[0], pis, alphas, perm, sets, z_leaves)
    quot_coeffs = []
    for c in range(num_challenges):
        cs = coset_interpolate(qv[c], log_n + q)
        quot_coeffs += [cs[k * n:(k + 1) * n] for k in range(1 << q)]
    quot_oracle = commit(quot_coeffs, log_n, cfg.rate_bits, cfg.cap_height)
    ch.observe(cap_of(quot_oracle))
    zeta = ch.get_ext()
    g = fo.root_of_unity(log_n)
    points = [zeta, (zeta[0] * g % P, zeta[1] * g % P)]
    coeffs.append(quot_coeffs)
    oracles.append(quot_oracle)
    opening, _ = fo.prove(coeffs, cfg, log_n, L.points_ranges, points, ch, oracles=oracles)
    challenger.sponge, challenger.inp, challenger.out = ch.words()
    return np.array([w for o in oracles for w in cap_of(o)] + [int(w) for w in opening], dtype=np.uint64)


def verify(air, cfg, log_n, q, num_challenges, pis, challenger, proof, perm=None):
    """0 if accepted, else the failed check (CHECKS), in the order 8, the opening layer's 1 and 2, 9, the rest of the opening layer"""
    L = layout(air, cfg, log_n, q, num_challenges, perm)
    proof = [int(w) for w in proof]
    assert len(proof) == L.total
    if any(w >= P for w in proof[:L.openings]):
        return 8
    pis, ch, n = [int(v) % P for v in pis], challenger, 1 << log_n
    ch.observe(pis)
    ch.observe(proof[:L.capw])
    sets = None
    if L.num_z:
        sets = draw_challenge_sets(perm, num_challenges, ch)
        ch.observe(proof[L.z_cap:L.z_cap + L.capw])
    alphas = [ch.get() for _ in range(num_challenges)]
    ch.observe(proof[L.quot_cap:L.quot_cap + L.capw])
    zeta = ch.get_ext()
    g = fo.root_of_unity(log_n)
    points = [zeta, (zeta[0] * g % P, zeta[1] * g % P)]
    caps = [np.array(proof[o * L.capw:(o + 1) * L.capw], dtype=np.uint64) for o in range(len(L.cols))]
    opening = proof[L.openings:]
    # the opening layer's checks 1 and 2 come before the identity: a first pass on a copy of the transcript tells them apart
    trial = fo.Challenger()
    trial.sponge, trial.inp, trial.out = ch.words()
    first = fo.verify(caps, cfg, log_n, L.cols, L.points_ranges, points, trial, opening)
    if first in (1, 2):
        fo.verify(caps, cfg, log_n, L.cols, L.points_ranges, points, ch, opening)
        return first
    ext = lambda at: (proof[at], proof[at + 1])
    local = [ext(L.op_local + 2 * j) for j in range(air.width)]
    nxt = [ext(L.op_next + 2 * j) for j in range(air.width)]
    z_local = [ext(L.op_z + 2 * z) for z in range(L.num_z)]
    z_next = [ext(L.op_z_next + 2 * z) for z in range(L.num_z)]
    acc, zh = vanishing(air, log_n, zeta, local, nxt, pis, alphas, EXT, perm, sets, z_local, z_next)
    zeta_n = fo.e_pow(zeta, n)
    identity = all(acc[c] == fo.e_mul(zh, fo.e_horner([ext(L.op_quotient + 2 * (c * L.Q + k)) for k in range(L.Q)], zeta_n)) for c in range(num_challenges))
    rest = fo.verify(caps, cfg, log_n, L.cols, L.points_ranges, points, ch, opening)
    return rest if identity else 9
