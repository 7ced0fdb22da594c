"""The gate-program format of include/lcp2.h restated over Python integers: one decoder, the constraints a program emits and its
degree bound.  The tests hold csrc/gate_program.hpp (and through it the verifier, the recursion gadget and the degrees) to this
module, so it shares nothing with that header."""
P = 0xFFFFFFFF00000001
OP_ADD, OP_SUB, OP_MUL, OP_EMIT, OP_XOR, OP_DBLADD, OP_EMITBOOL, OP_MULADD, OP_SBOX, OP_PMDS = range(10)
KIND_REG, KIND_WIRE, KIND_CONST, KIND_IMM, KIND_PI = range(5)
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8] + [0] * 11
DEGREE_CAP = 1 << 20   # where the library's degrees saturate (prover_build.hip)


def decode(words):
    """[(op, dst, (kind_a, kind_b), (idx_a, idx_b))] of a flat list of two-word instructions"""
    out = []
    for pc in range(0, len(words), 2):
        w0, w1 = int(words[pc]), int(words[pc + 1])
        out.append((w0 & 0xF, (w0 >> 8) & 0xFF, ((w0 >> 16) & 0xF, (w0 >> 20) & 0xF), (w1 & 0xFFFF, w1 >> 16)))
    return out


def num_sources(op):
    """operands an instruction reads as single values (a PMDS reads a register window and a block of immediates instead)"""
    return 0 if op == OP_PMDS else 1 if op in (OP_EMIT, OP_EMITBOOL, OP_SBOX) else 2


def emitted_constraints(words, imm, wires, consts, pis):
    """the constraints in program order, mod P.  consts: the gate constants (after the selector columns)"""
    reg, emitted = [0] * 256, []

    def operand(kind, idx):
        return int((reg, wires, consts, imm, pis)[kind][idx])

    for op, dst, kinds, idx in decode(words):
        if op == OP_PMDS:
            src = reg[idx[0]:idx[0] + 12]
            for r in range(12):
                reg[dst + r] = (sum(src[(i + r) % 12] * MDS_CIRC[i] for i in range(12)) + src[r] * MDS_DIAG[r] + int(imm[idx[1] + r])) % P
            continue
        x = operand(kinds[0], idx[0])
        if op == OP_EMIT:
            emitted.append(x % P)
        elif op == OP_EMITBOOL:
            emitted.append((x * x - x) % P)
        elif op == OP_SBOX:
            reg[dst] = pow(x, 7, P)
        else:
            y = operand(kinds[1], idx[1])
            reg[dst] = {OP_ADD: x + y, OP_SUB: x - y, OP_MUL: x * y, OP_XOR: x + y - 2 * x * y, OP_DBLADD: 2 * x + y, OP_MULADD: reg[dst] + x * y}[op] % P
    return emitted


def program_degree(words, num_regs=64):
    """degree bound of a program: WIRE / CONST 1, IMM / PI 0, ADD / SUB / DBLADD max, MUL / XOR sum, MULADD max(dst, sum), SBOX 7 x,
    PMDS max of its window, EMIT the operand, EMITBOOL twice; max over the emits.  Every product saturates at DEGREE_CAP."""
    reg, deg = [0] * max(num_regs, 1), 0
    for op, dst, kinds, idx in decode(words):
        def of(k):
            return reg[idx[k]] if kinds[k] == KIND_REG else 1 if kinds[k] in (KIND_WIRE, KIND_CONST) else 0
        if op == OP_PMDS:
            reg[dst:dst + 12] = [max(reg[idx[0]:idx[0] + 12])] * 12
        elif op == OP_EMIT:
            deg = max(deg, of(0))
        elif op == OP_EMITBOOL:
            deg = max(deg, min(2 * of(0), DEGREE_CAP))
        elif op == OP_SBOX:
            reg[dst] = min(7 * of(0), DEGREE_CAP)
        elif op in (OP_MUL, OP_XOR):
            reg[dst] = min(of(0) + of(1), DEGREE_CAP)
        elif op == OP_MULADD:
            reg[dst] = max(reg[dst], min(of(0) + of(1), DEGREE_CAP))
        else:
            reg[dst] = max(of(0), of(1))
    return deg
