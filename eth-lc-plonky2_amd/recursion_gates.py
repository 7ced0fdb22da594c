"""More of plonky2's gate library as constraint programs: the gates its recursion circuits are built from
(plonky2 0.1.4 gates/arithmetic_extension.rs, multiplication_extension.rs, reducing.rs, reducing_extension.rs, random_access.rs,
exponentiation.rs, poseidon_mds.rs;
[RECALL] of the published source: wire layouts and the order of eval_unfiltered, D = 2, standard_recursion_config).  They run
on the device as generated straight-line evaluators (csrc/generated_gates_rec*.hpp; `native=False`: through the interpreter of K6) and through
the host verifier like any other program; the
recursive verifier of this repository (host/recursion.cpp) does not need them - it is made of ArithmeticGate operations - they
are here so that a fork can hand a circuit that contains them to lcp2_circuit_create.

Each gate comes with the generator that fills one of its rows (Python integers), used by the tests to check that the program
vanishes on a valid row and does not on a perturbed one, and by `recursion_gates_circuit` to build a small provable circuit.
"""
import numpy as np

from . import gl_np as gl
from .circuit import (GATE_EMIT_FORWARD, K_REG, Circuit, GateSet, W, C, gate_noop, sigma_values)

P = gl.P
EXT_W = 7  # F[X] / (X^2 - 7)

ARITH_EXT_OPS = 10       # num_routed_wires / (4 D)
MUL_EXT_OPS = 13         # num_routed_wires / (3 D)
REDUCING_COEFFS = 43     # min(num_routed - 3 D, (num_wires - 2 D) / (D + 1))
RANDOM_ACCESS_BITS, RANDOM_ACCESS_COPIES, RANDOM_ACCESS_EXTRA = 4, 4, 2
EXP_POWER_BITS = 66      # min(num_routed - 3, (num_wires - 2) / 2)
REDUCING_EXT_COEFFS = 32 # min((num_routed - 3 D) / D, (num_wires - 2 D) / (2 D))
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8] + [0] * 11


# ---------------------------------------------------------------- extension arithmetic inside a program
def _ext_mul(asm, a, b):
    """(a0 + a1 X)(b0 + b1 X) -> two fresh registers"""
    t0 = asm.mul(a[0], b[0])
    t1 = asm.mul(a[1], b[1])
    asm.mul(t1, asm.imm(EXT_W), dst=t1[1])
    asm.add(t0, t1, dst=t0[1])
    asm.release(t1)
    u = asm.mul(a[0], b[1])
    asm.muladd(u, a[1], b[0])
    return t0, u


def _ext_scale(asm, a, s):
    return asm.mul(a[0], s), asm.mul(a[1], s)


def _emit_ext_diff(asm, x, y):
    """constraints x - y, component by component"""
    for k in range(2):
        d = asm.sub(x[k], y[k])
        asm.emit(d)
        asm.release(d)


def gate_arithmetic_extension(asm):
    """ArithmeticExtensionGate { num_ops: 10 }: wires 8i .. 8i+7 = multiplicand_0, multiplicand_1, addend, output (2 each);
    constraints output - (c0 * m0 * m1 + c1 * addend)"""
    asm.flags |= GATE_EMIT_FORWARD
    for i in range(ARITH_EXT_OPS):
        w = [(W(8 * i + 2 * k), W(8 * i + 2 * k + 1)) for k in range(4)]
        prod = _ext_mul(asm, w[0], w[1])
        for k in range(2):
            asm.mul(prod[k], C(0), dst=prod[k][1])
            asm.muladd(prod[k], w[2][k], C(1))
        _emit_ext_diff(asm, w[3], prod)
        asm.release(*prod)


def gate_mul_extension(asm):
    """MulExtensionGate { num_ops: 13 }: wires 6i .. 6i+5 = multiplicand_0, multiplicand_1, output; constraints output - c0 * m0 * m1"""
    asm.flags |= GATE_EMIT_FORWARD
    for i in range(MUL_EXT_OPS):
        w = [(W(6 * i + 2 * k), W(6 * i + 2 * k + 1)) for k in range(3)]
        prod = _ext_mul(asm, w[0], w[1])
        for k in range(2):
            asm.mul(prod[k], C(0), dst=prod[k][1])
        _emit_ext_diff(asm, w[2], prod)
        asm.release(*prod)


def _reducing_wires():
    out, alpha, old = (W(0), W(1)), (W(2), W(3)), (W(4), W(5))
    coeffs = [W(6 + i) for i in range(REDUCING_COEFFS)]
    start = 6 + REDUCING_COEFFS
    accs = [(W(start + 2 * i), W(start + 2 * i + 1)) for i in range(REDUCING_COEFFS - 1)] + [out]
    return out, alpha, old, coeffs, accs


def gate_reducing(asm):
    """ReducingGate<2> { num_coeffs: 43 }: output, alpha, old_acc (2 wires each), 43 base-field coefficients, 42 intermediate
    accumulators; constraints acc_i - (acc_{i-1} * alpha + coeff_i), acc_{-1} = old_acc, acc_42 = output"""
    asm.flags |= GATE_EMIT_FORWARD
    out, alpha, old, coeffs, accs = _reducing_wires()
    prev = old
    for i in range(REDUCING_COEFFS):
        t = _ext_mul(asm, prev, alpha)
        asm.add(t[0], coeffs[i], dst=t[0][1])
        _emit_ext_diff(asm, accs[i], t)
        asm.release(*t)
        prev = accs[i]


def gate_reducing_extension(asm):
    """ReducingExtensionGate<2> { num_coeffs: 32 }: as ReducingGate with extension-field coefficients (2 wires each)"""
    asm.flags |= GATE_EMIT_FORWARD
    out, alpha, prev = (W(0), W(1)), (W(2), W(3)), (W(4), W(5))
    start = 6 + 2 * REDUCING_EXT_COEFFS
    for i in range(REDUCING_EXT_COEFFS):
        t = _ext_mul(asm, prev, alpha)
        for k in range(2):
            asm.add(t[k], W(6 + 2 * i + k), dst=t[k][1])
        acc = (W(start + 2 * i), W(start + 2 * i + 1)) if i < REDUCING_EXT_COEFFS - 1 else out
        _emit_ext_diff(asm, acc, t)
        asm.release(*t)
        prev = acc


def gate_poseidon_mds(asm):
    """PoseidonMdsGate: 12 extension inputs (wires 2i, 2i+1), 12 extension outputs (wires 24 + 2i, 25 + 2i); constraints
    output - MDS(input).  The MDS layer is base-field linear, so it acts on each component: the PMDS instruction with zero
    constants on the components' register window; the constraints are listed output by output, as plonky2 lists them."""
    asm.flags |= GATE_EMIT_FORWARD
    asm.reserve(0, 48)
    zero = asm.imm(0)
    for k in range(2):
        for i in range(12):
            asm.add(W(2 * i + k), zero, dst=i)
        asm.pmds(12, 0, [0] * 12)
        for i in range(12):
            asm.sub(W(24 + 2 * i + k), (K_REG, 12 + i), dst=24 + 12 * k + i)
    for i in range(12):
        asm.emit((K_REG, 24 + i))
        asm.emit((K_REG, 36 + i))


def gate_random_access(asm):
    """RandomAccessGate { bits: 4, num_copies: 4, num_extra_constants: 2 }: per copy access_index, claimed_element and 16 list items
    (routed), then the 2 extra constants (routed), then 4 bit wires per copy.  Constraints per copy: the bits are boolean, they
    recompose to access_index, and folding the list by the bits leaves claimed_element; last constants - their wires."""
    asm.flags |= GATE_EMIT_FORWARD
    vec = 1 << RANDOM_ACCESS_BITS
    routed = (2 + vec) * RANDOM_ACCESS_COPIES + RANDOM_ACCESS_EXTRA
    for c in range(RANDOM_ACCESS_COPIES):
        base = (2 + vec) * c
        bits = [W(routed + RANDOM_ACCESS_BITS * c + i) for i in range(RANDOM_ACCESS_BITS)]
        for b in bits:
            asm.emit_bool(b)
        acc = asm.dbladd(bits[3], bits[2])
        asm.dbladd(acc, bits[1], dst=acc[1])
        asm.dbladd(acc, bits[0], dst=acc[1])
        asm.sub(acc, W(base), dst=acc[1])
        asm.emit(acc)
        asm.release(acc)
        items = [W(base + 2 + i) for i in range(vec)]
        for b in bits:
            nxt = []
            for k in range(0, len(items), 2):
                x, y = items[k], items[k + 1]
                d = asm.sub(y, x)
                asm.mul(d, b, dst=d[1])
                asm.add(d, x, dst=d[1])
                nxt.append(d)
            asm.release(*items)
            items = nxt
        asm.sub(items[0], W(base + 1), dst=items[0][1])
        asm.emit(items[0])
        asm.release(items[0])
    for i in range(RANDOM_ACCESS_EXTRA):
        d = asm.sub(C(i), W((2 + vec) * RANDOM_ACCESS_COPIES + i))
        asm.emit(d)
        asm.release(d)


def gate_exponentiation(asm):
    """ExponentiationGate { num_power_bits: 66 }: base (wire 0), 66 power bits little endian, output, 66 intermediate values;
    constraints intermediate'_i - intermediate_i with intermediate'_i = (i = 0 ? 1 : intermediate_{i-1}^2) * (bit * base + 1 - bit)
    over the bits from the top one down, last output - intermediate_65"""
    asm.flags |= GATE_EMIT_FORWARD
    n = EXP_POWER_BITS
    base, out = W(0), W(1 + n)
    inter = [W(2 + n + i) for i in range(n)]
    one = asm.imm(1)
    for i in range(n):
        bit = W(1 + (n - 1 - i))
        m = asm.sub(base, one)       # bit * base + 1 - bit = bit * (base - 1) + 1
        asm.mul(m, bit, dst=m[1])
        asm.add(m, one, dst=m[1])
        if i:
            sq = asm.mul(inter[i - 1], inter[i - 1])
            asm.mul(m, sq, dst=m[1])
            asm.release(sq)
        asm.sub(m, inter[i], dst=m[1])
        asm.emit(m)
        asm.release(m)
    d = asm.sub(out, inter[n - 1])
    asm.emit(d)
    asm.release(d)


def recursion_gateset(native=True):
    """sorted by (degree, name) as plonky2 sorts a gate set; two selector groups under max_degree 9.  native: claim the generated
    straight-line device evaluators (checked at build()); False: everything runs through the K6 interpreter"""
    return GateSet([
        ("NoopGate", 0, gate_noop),
        ("PoseidonMdsGate", 1, gate_poseidon_mds),
        ("ReducingExtensionGate", 2, gate_reducing_extension),
        ("ReducingGate", 2, gate_reducing),
        ("ArithmeticExtensionGate", 3, gate_arithmetic_extension),
        ("MulExtensionGate", 3, gate_mul_extension),
        ("ExponentiationGate", 4, gate_exponentiation),
        ("RandomAccessGate", 5, gate_random_access),
    ], native=native)


# ---------------------------------------------------------------- row generators (Python integers)
def _emul(a, b):
    return ((a[0] * b[0] + EXT_W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def row_arithmetic_extension(rng, c0, c1, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    for i in range(ARITH_EXT_OPS):
        m0, m1, ad = (w[8 * i], w[8 * i + 1]), (w[8 * i + 2], w[8 * i + 3]), (w[8 * i + 4], w[8 * i + 5])
        pr = _emul(m0, m1)
        w[8 * i + 6], w[8 * i + 7] = (c0 * pr[0] + c1 * ad[0]) % P, (c0 * pr[1] + c1 * ad[1]) % P
    return w


def row_mul_extension(rng, c0, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    for i in range(MUL_EXT_OPS):
        pr = _emul((w[6 * i], w[6 * i + 1]), (w[6 * i + 2], w[6 * i + 3]))
        w[6 * i + 4], w[6 * i + 5] = c0 * pr[0] % P, c0 * pr[1] % P
    return w


def row_reducing(rng, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    alpha, acc = (w[2], w[3]), (w[4], w[5])
    start = 6 + REDUCING_COEFFS
    for i in range(REDUCING_COEFFS):
        t = _emul(acc, alpha)
        acc = ((t[0] + w[6 + i]) % P, t[1])
        if i < REDUCING_COEFFS - 1:
            w[start + 2 * i], w[start + 2 * i + 1] = acc
        else:
            w[0], w[1] = acc
    return w


def row_reducing_extension(rng, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    alpha, acc = (w[2], w[3]), (w[4], w[5])
    start = 6 + 2 * REDUCING_EXT_COEFFS
    for i in range(REDUCING_EXT_COEFFS):
        t = _emul(acc, alpha)
        acc = ((t[0] + w[6 + 2 * i]) % P, (t[1] + w[7 + 2 * i]) % P)
        if i < REDUCING_EXT_COEFFS - 1:
            w[start + 2 * i], w[start + 2 * i + 1] = acc
        else:
            w[0], w[1] = acc
    return w


def row_poseidon_mds(rng, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    for k in range(2):
        s = [w[2 * i + k] for i in range(12)]
        for r in range(12):
            w[24 + 2 * r + k] = (sum(s[(i + r) % 12] * MDS_CIRC[i] for i in range(12)) + s[r] * MDS_DIAG[r]) % P
    return w


def row_random_access(rng, c0, c1, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    vec = 1 << RANDOM_ACCESS_BITS
    routed = (2 + vec) * RANDOM_ACCESS_COPIES + RANDOM_ACCESS_EXTRA
    for c in range(RANDOM_ACCESS_COPIES):
        base = (2 + vec) * c
        idx = int(rng.integers(0, vec))
        w[base] = idx
        w[base + 1] = w[base + 2 + idx]
        for i in range(RANDOM_ACCESS_BITS):
            w[routed + RANDOM_ACCESS_BITS * c + i] = (idx >> i) & 1
    w[(2 + vec) * RANDOM_ACCESS_COPIES], w[(2 + vec) * RANDOM_ACCESS_COPIES + 1] = c0, c1
    return w


def row_exponentiation(rng, num_wires=135):
    w = [int(v) for v in rng.integers(0, P, size=num_wires, dtype=np.uint64)]
    n = EXP_POWER_BITS
    base = w[0]
    power = int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 16)) << 62)
    cur = 1
    for i in range(n):
        w[1 + i] = (power >> i) & 1
    for i in range(n):
        bit = (power >> (n - 1 - i)) & 1
        cur = (cur * cur if i else 1) % P * (base if bit else 1) % P
        w[2 + n + i] = cur
    w[1 + n] = cur
    assert cur == pow(base, power, P)
    return w


def recursion_gates_circuit(params, seed, native=True):
    """A provable circuit whose rows cycle through the seven gates (no copy constraints: identity permutation, no public inputs).
    Returns (Circuit, wires [num_wires][n], public_inputs = [])."""
    rng = np.random.default_rng(seed)
    gs = recursion_gateset(native)
    n, Wn, NR = 1 << params.degree_bits, params.num_wires, params.num_routed_wires
    assert params.num_constants == gs.num_selectors + 2 and Wn >= 135 and NR >= 80
    kinds = ["ReducingGate", "ArithmeticExtensionGate", "MulExtensionGate", "ExponentiationGate", "RandomAccessGate", "ReducingExtensionGate",
             "PoseidonMdsGate"]
    gate_of_row = np.zeros(n, dtype=np.int64)  # NoopGate
    wires = np.zeros((Wn, n), dtype=np.uint64)
    c0 = rng.integers(0, P, size=n, dtype=np.uint64)
    c1 = rng.integers(0, P, size=n, dtype=np.uint64)
    for r in range(n - min(4, n // 4)):
        kind = kinds[r % len(kinds)]
        gate_of_row[r] = gs.index(kind)
        a, b = int(c0[r]), int(c1[r])
        row = {"ReducingExtensionGate": lambda: row_reducing_extension(rng, Wn), "PoseidonMdsGate": lambda: row_poseidon_mds(rng, Wn),
               "ReducingGate": lambda: row_reducing(rng, Wn), "ArithmeticExtensionGate": lambda: row_arithmetic_extension(rng, a, b, Wn),
               "MulExtensionGate": lambda: row_mul_extension(rng, a, Wn), "ExponentiationGate": lambda: row_exponentiation(rng, Wn),
               "RandomAccessGate": lambda: row_random_access(rng, a, b, Wn)}[kind]()
        wires[:, r] = np.array(row, dtype=np.uint64)
    rows = np.arange(n)
    k_is = gl.powers(7, NR)
    sig = sigma_values(np.tile(rows, (NR, 1)), np.tile(np.arange(NR)[:, None], (1, n)), k_is, params.degree_bits)
    cs = np.concatenate([gs.selector_columns(gate_of_row), c0[None, :], c1[None, :], sig])
    return Circuit(params, gs, cs, k_is, 0), wires, np.zeros(0, dtype=np.uint64)


# ---------------------------------------------------------------- jobs of lcp2_rec_gate_rows: one operation of one row each
from types import SimpleNamespace  # noqa: E402

from .binding import (REC_ARITHMETIC, REC_ARITHMETIC_EXT, REC_BASE_SUM, REC_CELL, REC_COSET_INTERPOLATION, REC_EXPONENTIATION,  # noqa: E402
                      REC_IMM, REC_JOB_DTYPE, REC_MUL_EXT, REC_OPERAND_DTYPE, REC_POSEIDON_MDS, REC_RANDOM_ACCESS, REC_REDUCING,
                      REC_REDUCING_EXT)
from .circuit import ARITH_OPS, BASE_SUM_LIMBS, gate_arithmetic, gate_base_sum  # noqa: E402

RA_VEC = 1 << RANDOM_ACCESS_BITS
RA_ROUTED = (2 + RA_VEC) * RANDOM_ACCESS_COPIES + RANDOM_ACCESS_EXTRA
REC_ROW_COLUMNS = 135
# kind -> (gate name, operations per row, operands of operation `op`)
REC_JOB_KINDS = {
    REC_ARITHMETIC: ("ArithmeticGate", ARITH_OPS, lambda op: 5),
    REC_BASE_SUM: ("BaseSumGate", 1, lambda op: 1),
    REC_ARITHMETIC_EXT: ("ArithmeticExtensionGate", ARITH_EXT_OPS, lambda op: 8),
    REC_MUL_EXT: ("MulExtensionGate", MUL_EXT_OPS, lambda op: 5),
    REC_REDUCING: ("ReducingGate", 1, lambda op: 4 + REDUCING_COEFFS),
    REC_REDUCING_EXT: ("ReducingExtensionGate", 1, lambda op: 4 + 2 * REDUCING_EXT_COEFFS),
    REC_POSEIDON_MDS: ("PoseidonMdsGate", 1, lambda op: 24),
    REC_RANDOM_ACCESS: ("RandomAccessGate", RANDOM_ACCESS_COPIES + 1, lambda op: 1 + RA_VEC if op < RANDOM_ACCESS_COPIES else RANDOM_ACCESS_EXTRA),
    REC_EXPONENTIATION: ("ExponentiationGate", 1, lambda op: 3),
    REC_COSET_INTERPOLATION: ("CosetInterpolationGate", 1, lambda op: 35),
}


def job_columns(kind, op):
    """the columns (wires) one job of lcp2_rec_gate_rows owns: every cell of operation `op` of a row of gate `kind`"""
    name, ops, _ = REC_JOB_KINDS[kind]
    assert 0 <= op < ops, (name, op)
    if kind == REC_ARITHMETIC:
        return list(range(4 * op, 4 * op + 4))
    if kind == REC_BASE_SUM:
        return list(range(1 + BASE_SUM_LIMBS))
    if kind == REC_ARITHMETIC_EXT:
        return list(range(8 * op, 8 * op + 8))
    if kind == REC_MUL_EXT:
        return list(range(6 * op, 6 * op + 6))
    if kind == REC_REDUCING:
        return list(range(6 + REDUCING_COEFFS + 2 * (REDUCING_COEFFS - 1)))
    if kind == REC_REDUCING_EXT:
        return list(range(6 + 2 * REDUCING_EXT_COEFFS + 2 * (REDUCING_EXT_COEFFS - 1)))
    if kind == REC_POSEIDON_MDS:
        return list(range(48))
    if kind == REC_RANDOM_ACCESS:
        if op == RANDOM_ACCESS_COPIES:
            return [RA_ROUTED - 2, RA_ROUTED - 1]
        return list(range((2 + RA_VEC) * op, (2 + RA_VEC) * (op + 1))) + list(range(RA_ROUTED + RANDOM_ACCESS_BITS * op, RA_ROUTED + RANDOM_ACCESS_BITS * (op + 1)))
    if kind == REC_EXPONENTIATION:
        return list(range(2 + 2 * EXP_POWER_BITS))
    return list(range(1 + 2 * 16 + 4 + 4 * 2 + 2))   # CosetInterpolationGate: shift, 16 values, point, value, 2 x (eval, prod), shifted point


def job_cells(kind, op, vals):
    """{column: value} of one job in Python integers: run_once of operation `op` of gate `kind` on the operand values `vals` (any
    u64 each, reduced here; the two power words of EXPONENTIATION are bit strings and are not)"""
    from . import u32_gates as ug
    raw, v, out = [int(x) for x in vals], [int(x) % P for x in vals], {}
    assert len(v) == REC_JOB_KINDS[kind][2](op)

    def pair(k):
        return (v[k], v[k + 1])

    def put2(col, x):
        out[col], out[col + 1] = x

    if kind == REC_ARITHMETIC:
        c0, c1, m0, m1, ad = v
        out.update({4 * op: m0, 4 * op + 1: m1, 4 * op + 2: ad, 4 * op + 3: (c0 * m0 * m1 + c1 * ad) % P})
    elif kind == REC_BASE_SUM:
        assert v[0] < 1 << BASE_SUM_LIMBS
        out[0] = v[0]
        for i in range(BASE_SUM_LIMBS):
            out[1 + i] = (v[0] >> i) & 1
    elif kind == REC_ARITHMETIC_EXT:
        c0, c1, m0, m1, ad = v[0], v[1], pair(2), pair(4), pair(6)
        pr = _emul(m0, m1)
        for k, x in enumerate((m0, m1, ad, ((c0 * pr[0] + c1 * ad[0]) % P, (c0 * pr[1] + c1 * ad[1]) % P))):
            put2(8 * op + 2 * k, x)
    elif kind == REC_MUL_EXT:
        pr = _emul(pair(1), pair(3))
        for k, x in enumerate((pair(1), pair(3), (v[0] * pr[0] % P, v[0] * pr[1] % P))):
            put2(6 * op + 2 * k, x)
    elif kind in (REC_REDUCING, REC_REDUCING_EXT):
        ext = kind == REC_REDUCING_EXT
        count = REDUCING_EXT_COEFFS if ext else REDUCING_COEFFS
        alpha, acc = pair(0), pair(2)
        put2(2, alpha)
        put2(4, acc)
        start = 6 + (2 if ext else 1) * count
        for i in range(count):
            c = pair(4 + 2 * i) if ext else (v[4 + i], 0)
            if ext:
                put2(6 + 2 * i, c)
            else:
                out[6 + i] = c[0]
            t = _emul(acc, alpha)
            acc = ((t[0] + c[0]) % P, (t[1] + c[1]) % P)
            put2(start + 2 * i if i < count - 1 else 0, acc)
    elif kind == REC_POSEIDON_MDS:
        for k in range(2):
            s = [v[2 * i + k] for i in range(12)]
            for r in range(12):
                out[2 * r + k] = s[r]
                out[24 + 2 * r + k] = (sum(s[(i + r) % 12] * MDS_CIRC[i] for i in range(12)) + s[r] * MDS_DIAG[r]) % P
    elif kind == REC_RANDOM_ACCESS:
        if op == RANDOM_ACCESS_COPIES:
            out[RA_ROUTED - 2], out[RA_ROUTED - 1] = v
        else:
            base, idx = (2 + RA_VEC) * op, v[0]
            assert idx < RA_VEC
            out[base], out[base + 1] = idx, v[1 + idx]
            for i in range(RA_VEC):
                out[base + 2 + i] = v[1 + i]
            for i in range(RANDOM_ACCESS_BITS):
                out[RA_ROUTED + RANDOM_ACCESS_BITS * op + i] = (idx >> i) & 1
    elif kind == REC_EXPONENTIATION:
        n = EXP_POWER_BITS
        assert v[2] <= 3
        base, power = v[0], raw[1] | (v[2] << 64)
        out[0] = base
        cur = 1
        for i in range(n):
            out[1 + i] = (power >> i) & 1
        for i in range(n):
            bit = (power >> (n - 1 - i)) & 1
            cur = (cur * cur if i else 1) % P * (base if bit else 1) % P
            out[2 + n + i] = cur
        out[1 + n] = cur
    else:
        domain = ug._coset_domain()
        weights = ug._barycentric_weights(domain)
        shift, values, point = v[0], [pair(1 + 2 * i) for i in range(ug.COSET_POINTS)], pair(33)
        assert shift
        inv_shift = pow(shift, P - 2, P)
        x = (point[0] * inv_shift % P, point[1] * inv_shift % P)
        out[0] = shift
        for i, val in enumerate(values):
            put2(1 + 2 * i, val)
        put2(33, point)
        ev, pr, pinned = (0, 0), (1, 0), 0
        for i in range(ug.COSET_POINTS):
            term = ((x[0] - domain[i]) % P, x[1])
            wv = (values[i][0] * weights[i] % P, values[i][1] * weights[i] % P)
            e1, e2 = _emul(ev, term), _emul(wv, pr)
            ev, pr = ((e1[0] + e2[0]) % P, (e1[1] + e2[1]) % P), _emul(pr, term)
            if i + 1 in (ug.COSET_DEGREE, 2 * ug.COSET_DEGREE - 1):
                put2(37 + 2 * pinned, ev)
                put2(41 + 2 * pinned, pr)
                pinned += 1
        put2(35, ev)
        put2(45, x)
    return out


def job_inputs(kind, op, w, c0=0, c1=0):
    """the operand values of operation `op` read back from a filled row `w` (a sequence of wire values) and the row's gate constants"""
    w = [int(x) for x in w[:REC_ROW_COLUMNS]]
    if kind == REC_ARITHMETIC:
        return [c0, c1] + w[4 * op:4 * op + 3]
    if kind == REC_BASE_SUM:
        return [w[0]]
    if kind == REC_ARITHMETIC_EXT:
        return [c0, c1] + w[8 * op:8 * op + 6]
    if kind == REC_MUL_EXT:
        return [c0] + w[6 * op:6 * op + 4]
    if kind == REC_REDUCING:
        return w[2:6 + REDUCING_COEFFS]
    if kind == REC_REDUCING_EXT:
        return w[2:6 + 2 * REDUCING_EXT_COEFFS]
    if kind == REC_POSEIDON_MDS:
        return w[:24]
    if kind == REC_RANDOM_ACCESS:
        base = (2 + RA_VEC) * op
        return [c0, c1] if op == RANDOM_ACCESS_COPIES else [w[base]] + w[base + 2:base + 2 + RA_VEC]
    if kind == REC_EXPONENTIATION:
        return [w[0], sum(w[1 + i] << i for i in range(64)), w[65] | (w[66] << 1)]
    return w[:35]


IMM = lambda v: (int(v), 0, REC_IMM)          # noqa: E731
CELL = lambda row, col: (int(row), int(col), REC_CELL)   # noqa: E731


def pack_plan(levels):
    """levels: [[(row, kind, op, [IMM(..) / CELL(..), ..]), ..], ..] -> (jobs, operands, level_ends) as record arrays, every level
    sorted by (kind, op, row): the order in which lcp2_rec_gate_rows stores contiguously.  The witness plan without chains"""
    plan = pack_witness_plan([(level, []) for level in levels])
    return plan.rec_jobs, plan.operands, plan.rec_level_ends


def run_plan(jobs, operands, level_ends, ncols, n, start=None):
    """lcp2_rec_gate_rows in Python integers: the matrix [ncols][n] after the plan ran on `start` (zeros by default)"""
    out = np.zeros((ncols, n), dtype=np.uint64) if start is None else start.copy()
    for j in jobs[:int(level_ends[-1]) if len(level_ends) else 0]:
        kind, op, first = int(j["kind"]), int(j["op"]), int(j["first_operand"])
        vals = []
        for o in operands[first:first + REC_JOB_KINDS[kind][2](op)]:
            vals.append(int(out[int(o["col"]), int(o["v"])]) % P if o["src"] == REC_CELL else int(o["v"]))
        for col, v in job_cells(kind, op, vals).items():
            out[col, int(j["row"])] = v
    return out


def witness_jobs(wires, gate_of_row, G, consts=None):
    """The IMM jobs that regenerate every owned cell of the recursion-gate rows of a filled host witness, in ONE level: the operands
    of each operation read out of `wires` [num_wires][n] and the rows' gate constants consts = (c0 [n], c1 [n]).  Operation slots
    whose cells are all zero get no job (a zero slot satisfies its gate, as a slot no generator ran on does).
    Returns (jobs, operands, level_ends)."""
    level = []
    for kind, (name, ops, _) in REC_JOB_KINDS.items():
        if name not in G:
            continue
        for r in np.nonzero(gate_of_row == G[name])[0]:
            w = wires[:, r]
            c0, c1 = (int(consts[0][r]), int(consts[1][r])) if consts is not None else (0, 0)
            for op in range(ops):
                if ops > 1 and not w[job_columns(kind, op)].any():
                    continue
                level.append((int(r), kind, op, [IMM(v) for v in job_inputs(kind, op, w, c0, c1)]))
    return pack_plan([level])


# ---------------------------------------------------------------- a chained plan over all ten gates
CHAIN_ORDER = [REC_ARITHMETIC, REC_BASE_SUM, REC_ARITHMETIC_EXT, REC_MUL_EXT, REC_REDUCING, REC_REDUCING_EXT, REC_POSEIDON_MDS,
               REC_RANDOM_ACCESS, REC_EXPONENTIATION, REC_COSET_INTERPOLATION]


def chain_gateset(native=True):
    """all ten gates and NoopGate, sorted by (degree, name) as plonky2 sorts a gate set: three selector groups under max_degree 9"""
    from . import u32_gates as ug
    return GateSet([
        ("NoopGate", 0, gate_noop),
        ("PoseidonMdsGate", 1, gate_poseidon_mds),
        ("BaseSumGate", 2, gate_base_sum(BASE_SUM_LIMBS)),
        ("ReducingExtensionGate", 2, gate_reducing_extension),
        ("ReducingGate", 2, gate_reducing),
        ("ArithmeticExtensionGate", 3, gate_arithmetic_extension),
        ("ArithmeticGate", 3, gate_arithmetic),
        ("MulExtensionGate", 3, gate_mul_extension),
        ("ExponentiationGate", 4, gate_exponentiation),
        ("RandomAccessGate", 5, gate_random_access),
        ("CosetInterpolationGate", 8, ug.gate_coset_interpolation),
    ], native=native)


def chain_plan(n, seed, levels=None):
    """A deterministic plan over n rows in which every level feeds the next.  Every level holds `width` groups of ten rows, one row of
    each gate; level 0 is IMM only (values drawn from `seed`), and every operand of a later level that is not a gate constant is a
    CELL of a row of the level before:
      ARITHMETIC        row constants (2, 1).  op 0, 1: lo = 2 b1 + b0 and hi = 2 b3 + b2 from the bit wires of the BASE_SUM row;
                        op 2: 4 hi + lo (as 2 hi 2 + lo) from the ARITHMETIC row - the low 4 bits of a BASE_SUM value, two levels on;
                        op 3: 2 index r + s (index: op 2 of the level before, r < 2^40 and s < 2^50 immediates), below 2^63
      BASE_SUM          the value is op 3 of the ARITHMETIC row
      ARITHMETIC_EXT    m0 = MUL_EXT output, m1 = REDUCING output, addend = a POSEIDON_MDS output
      MUL_EXT           m0 = ARITHMETIC_EXT output, m1 = COSET_INTERPOLATION evaluation_value
      REDUCING          alpha = MUL_EXT output, old_acc = ARITHMETIC_EXT output, coefficients = POSEIDON_MDS cells
      REDUCING_EXT      alpha = REDUCING output, old_acc = ARITHMETIC_EXT output, coefficients = REDUCING accumulators
      POSEIDON_MDS      inputs = REDUCING_EXT accumulators
      RANDOM_ACCESS     copy 0: index = op 2 of the ARITHMETIC row, items = POSEIDON_MDS outputs; op 4: the row's constants
      EXPONENTIATION    base = REDUCING output c0, power = (BASE_SUM value, a RANDOM_ACCESS bit)
      COSET_INTERPOLATION  shift = EXPONENTIATION output, values = REDUCING_EXT coefficients, point = MUL_EXT output
    levels = None: width 1 and as many levels as fit (at least 6 from n = 64); else that many levels, as wide as fit.  The gate
    constants and the immediates of the later levels depend on n only, so two seeds give the same plan but for level 0's values.
    Returns a namespace: jobs, operands, level_ends, expected (the matrix [135][n] in Python integers, from a zero matrix),
    gate_of_row (indices into chain_gateset()), c0, c1 (the gate constants of every row).  Level 0's operands come first in the
    operand list: they end where the first job of level 1 has its first_operand."""
    rng, fixed = np.random.default_rng(seed), np.random.default_rng(0xC4A1 + n)
    usable = n - min(4, n // 4)
    nk = len(CHAIN_ORDER)
    if levels is None:
        levels, width = usable // nk, 1
    else:
        width = usable // (nk * levels)
    assert levels >= 1 and width >= 1
    gs = chain_gateset()
    gate_of_row = np.zeros(n, dtype=np.int64)
    c0, c1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)

    def row_of(level, kind, j):
        return (level * nk + CHAIN_ORDER.index(kind)) * width + j

    def f(r=None):
        return int((r or fixed).integers(0, P, dtype=np.uint64))

    plan = []
    for lv in range(levels):
        jobs = []
        for j in range(width):
            R = {kind: row_of(lv, kind, j) for kind in CHAIN_ORDER}
            Q = {kind: row_of(lv - 1, kind, j) for kind in CHAIN_ORDER}
            for kind, r in R.items():
                gate_of_row[r] = gs.index(REC_JOB_KINDS[kind][0])
                c0[r], c1[r] = (2, 1) if kind == REC_ARITHMETIC else (f(), f())
            k = {kind: (IMM(c0[r]), IMM(c1[r])) for kind, r in R.items()}

            def cells(kind, cols):
                return [CELL(Q[kind], c) for c in cols]

            def leaf(count, hi=P):
                return [IMM(rng.integers(0, hi, dtype=np.uint64)) for _ in range(count)]

            first = lv == 0
            A, B = R[REC_ARITHMETIC], Q[REC_ARITHMETIC]
            bit = (lambda i: leaf(1, 2)[0]) if first else (lambda i: CELL(Q[REC_BASE_SUM], 1 + i))
            jobs.append((A, REC_ARITHMETIC, 0, [*k[REC_ARITHMETIC], bit(1), IMM(1), bit(0)]))
            jobs.append((A, REC_ARITHMETIC, 1, [*k[REC_ARITHMETIC], bit(3), IMM(1), bit(2)]))
            jobs.append((A, REC_ARITHMETIC, 2, [*k[REC_ARITHMETIC], *(leaf(1, 4) if first else [CELL(B, 7)]), IMM(2), *(leaf(1, 4) if first else [CELL(B, 3)])]))
            jobs.append((A, REC_ARITHMETIC, 3, [*k[REC_ARITHMETIC], *(leaf(1, 16) if first else [CELL(B, 11)]), IMM(fixed.integers(0, 1 << 40)), IMM(fixed.integers(0, 1 << 50))]))
            jobs.append((R[REC_BASE_SUM], REC_BASE_SUM, 0, leaf(1, 1 << 63) if first else [CELL(B, 15)]))
            jobs.append((R[REC_ARITHMETIC_EXT], REC_ARITHMETIC_EXT, 0, [*k[REC_ARITHMETIC_EXT], *(leaf(6) if first else
                         cells(REC_MUL_EXT, (4, 5)) + cells(REC_REDUCING, (0, 1)) + cells(REC_POSEIDON_MDS, (24, 25)))]))
            jobs.append((R[REC_MUL_EXT], REC_MUL_EXT, 0, [k[REC_MUL_EXT][0], *(leaf(4) if first else
                         cells(REC_ARITHMETIC_EXT, (6, 7)) + cells(REC_COSET_INTERPOLATION, (35, 36)))]))
            jobs.append((R[REC_REDUCING], REC_REDUCING, 0, leaf(47) if first else
                         cells(REC_MUL_EXT, (4, 5)) + cells(REC_ARITHMETIC_EXT, (6, 7)) + cells(REC_POSEIDON_MDS, range(REDUCING_COEFFS))))
            jobs.append((R[REC_REDUCING_EXT], REC_REDUCING_EXT, 0, leaf(68) if first else
                         cells(REC_REDUCING, (0, 1)) + cells(REC_ARITHMETIC_EXT, (6, 7)) + cells(REC_REDUCING, range(49, 49 + 2 * REDUCING_EXT_COEFFS))))
            jobs.append((R[REC_POSEIDON_MDS], REC_POSEIDON_MDS, 0, leaf(24) if first else cells(REC_REDUCING_EXT, range(70, 94))))
            jobs.append((R[REC_RANDOM_ACCESS], REC_RANDOM_ACCESS, 0, leaf(1, 16) + leaf(16) if first else
                         [CELL(B, 11)] + cells(REC_POSEIDON_MDS, range(24, 40))))
            jobs.append((R[REC_RANDOM_ACCESS], REC_RANDOM_ACCESS, RANDOM_ACCESS_COPIES, list(k[REC_RANDOM_ACCESS])))
            jobs.append((R[REC_EXPONENTIATION], REC_EXPONENTIATION, 0, leaf(1) + leaf(1, 1 << 64) + leaf(1, 4) if first else
                         cells(REC_REDUCING, (0,)) + cells(REC_BASE_SUM, (0,)) + cells(REC_RANDOM_ACCESS, (RA_ROUTED,))))
            jobs.append((R[REC_COSET_INTERPOLATION], REC_COSET_INTERPOLATION, 0, leaf(1, P - 1) + leaf(34) if first else
                         cells(REC_EXPONENTIATION, (1 + EXP_POWER_BITS,)) + cells(REC_REDUCING_EXT, range(6, 38)) + cells(REC_MUL_EXT, (4, 5))))
        plan.append(jobs)
    jobs, operands, level_ends = pack_plan(plan)
    expected = run_plan(jobs, operands, level_ends, REC_ROW_COLUMNS, n)
    return SimpleNamespace(jobs=jobs, operands=operands, level_ends=level_ends, expected=expected, gate_of_row=gate_of_row, c0=c0, c1=c1)


def chain_circuit(params, plan, native=True):
    """the circuit a chain_plan fills: its rows' gates and constants, no copy constraints (identity permutation), no public inputs"""
    gs = chain_gateset(native)
    n, NR = 1 << params.degree_bits, params.num_routed_wires
    assert n == plan.gate_of_row.size and params.num_constants == gs.num_selectors + 2 and params.num_wires >= REC_ROW_COLUMNS and NR >= 80
    rows = np.arange(n)
    k_is = gl.powers(7, NR)
    sig = sigma_values(np.tile(rows, (NR, 1)), np.tile(np.arange(NR)[:, None], (1, n)), k_is, params.degree_bits)
    cs = np.concatenate([gs.selector_columns(plan.gate_of_row), plan.c0[None, :], plan.c1[None, :], sig])
    return Circuit(params, gs, cs, k_is, 0), np.zeros(0, dtype=np.uint64)


# ---------------------------------------------------------------- witness plans that hold PoseidonGate rows (lcp2_witness_plan_rows)
from .binding import PLAN_PREV, POS_JOB_DTYPE  # noqa: E402

PREV = lambda j: (0, int(j), PLAN_PREV)   # noqa: E731  output j of the previous job of the same chain
POS_PLAN_OPERANDS = 13


def pack_witness_plan(levels):
    """levels: [(rec items, chains), ..]: rec items as in pack_plan, a chain a list of (row, swap operand, [12 input operands])
    -> a namespace of the six lists of lcp2_witness_plan_rows: rec_jobs, pos_jobs, chain_ends, operands, rec_level_ends,
    pos_level_ends.  The operands of a level follow those of the level before (rec jobs, sorted by (kind, op, row), then the
    chains in order), so level 0's operands come first; `leaves` is their number."""
    rec_items = [sorted(rec, key=lambda it: (it[1], it[2], it[0])) for rec, _ in levels]
    rec_jobs = np.zeros(sum(len(rec) for rec in rec_items), dtype=REC_JOB_DTYPE)
    pos_jobs = np.zeros(sum(len(chain) for _, chains in levels for chain in chains), dtype=POS_JOB_DTYPE)
    count = sum(len(it[3]) for rec in rec_items for it in rec) + POS_PLAN_OPERANDS * pos_jobs.size
    ops = np.zeros(count, dtype=REC_OPERAND_DTYPE)
    at = kr = kp = 0
    chain_ends, rec_ends, pos_ends, leaves = [], [], [], None
    for rec, (_, chains) in zip(rec_items, levels):
        for row, kind, op, operands in rec:
            assert len(operands) == REC_JOB_KINDS[kind][2](op), (kind, op, len(operands))
            rec_jobs[kr] = (row, kind, op, at, 0)
            for v, col, src in operands:
                ops[at] = (v % (1 << 64), col, src)
                at += 1
            kr += 1
        for chain in chains:
            for row, swap, inputs in chain:
                assert len(inputs) == 12
                pos_jobs[kp] = (row, at)
                for v, col, src in [swap] + list(inputs):
                    ops[at] = (v % (1 << 64), col, src)
                    at += 1
                kp += 1
            chain_ends.append(kp)
        rec_ends.append(kr)
        pos_ends.append(len(chain_ends))
        leaves = at if leaves is None else leaves
    u32 = lambda a: np.array(a, dtype=np.uint32)   # noqa: E731
    return SimpleNamespace(rec_jobs=rec_jobs, pos_jobs=pos_jobs, chain_ends=u32(chain_ends), operands=ops, rec_level_ends=u32(rec_ends),
                           pos_level_ends=u32(pos_ends), leaves=leaves or 0)


def run_witness_plan(plan, ncols, n, start=None, levels=None):
    """lcp2_witness_plan_rows in Python integers: the matrix [ncols][n] after the plan (its first `levels` levels) ran on `start`
    (zeros by default).  The rec jobs of a level through run_plan, then its chains row by row through poseidon_py.gate_row"""
    out = np.zeros((ncols, n), dtype=np.uint64) if start is None else start.copy()
    nlevels = len(plan.rec_level_ends) if levels is None else levels
    for lv in range(nlevels):
        rb, re = (int(plan.rec_level_ends[lv - 1]) if lv else 0), int(plan.rec_level_ends[lv])
        out = run_plan(plan.rec_jobs[rb:re], plan.operands, [re - rb], ncols, n, start=out)
        run_level_chains(plan, lv, out)
    return out


def run_level_chains(plan, lv, out):
    """the PoseidonGate chains of level `lv` of a witness plan, row by row, into the matrix `out` (in place)"""
    from . import poseidon_py as pp
    for g in range(int(plan.pos_level_ends[lv - 1]) if lv else 0, int(plan.pos_level_ends[lv])):
        prev = None
        for j in plan.pos_jobs[(int(plan.chain_ends[g - 1]) if g else 0):int(plan.chain_ends[g])]:
            vals = []
            for o in plan.operands[int(j["first_operand"]):int(j["first_operand"]) + POS_PLAN_OPERANDS]:
                src = int(o["src"])
                vals.append(int(out[int(o["col"]), int(o["v"])]) % P if src == REC_CELL else prev[int(o["col"])] if src == PLAN_PREV
                            else int(o["v"]) % P)
            assert vals[0] in (0, 1)
            row = pp.gate_row(vals[1:], vals[0])
            out[:pp.NUM_WIRES, int(j["row"])] = np.array(row, dtype=np.uint64)
            prev = row[pp.W_OUTPUT:pp.W_OUTPUT + 12]


def verifier_gateset(native=True):
    """chain_gateset with PoseidonGate added, sorted by (degree, name)"""
    from . import u32_gates as ug
    from .circuit import gate_poseidon
    return GateSet([
        ("NoopGate", 0, gate_noop),
        ("PoseidonMdsGate", 1, gate_poseidon_mds),
        ("BaseSumGate", 2, gate_base_sum(BASE_SUM_LIMBS)),
        ("ReducingExtensionGate", 2, gate_reducing_extension),
        ("ReducingGate", 2, gate_reducing),
        ("ArithmeticExtensionGate", 3, gate_arithmetic_extension),
        ("ArithmeticGate", 3, gate_arithmetic),
        ("MulExtensionGate", 3, gate_mul_extension),
        ("ExponentiationGate", 4, gate_exponentiation),
        ("RandomAccessGate", 5, gate_random_access),
        ("PoseidonGate", 7, gate_poseidon),
        ("CosetInterpolationGate", 8, ug.gate_coset_interpolation),
    ], native=native)


MERKLE_DEPTHS = [2, 3, 5, 1, 4]


def verifier_plan(n, seed, paths=None, sponge=None, expected=True):
    """A deterministic plan over n rows shaped like the Poseidon work of verify_proof, in five levels:
      0  rec     per path one BASE_SUM row (the query index, below 2^63) and ARITHMETIC leaves (op k: 1 * a * b + 1 * c): the only
                 per-proof immediates (drawn from `seed`); level 0's operands come first in the operand list
      1  chains  one Merkle path per BASE_SUM row, depths MERKLE_DEPTHS in turn: row k takes the digest so far - the head four
                 ARITHMETIC outputs as CELLs, later rows PREV 0..3 -, an immediate sibling and zeros, and its swap flag is the
                 CELL of limb k of the path's index
      2  chains  ONE sponge: 8 new inputs per row, IMM and CELL in turn (CELLs of ARITHMETIC leaves and of Merkle roots), the capacity
                 PREV 8..11
      3  rec     an ARITHMETIC and an ARITHMETIC_EXT row over CELLs of the sponge's and the paths' outputs
      4  chains  a second generation: each head reads eight of those cells, every later row takes PREV 0..11 (a Challenger that
                 keeps permuting)
    paths / sponge: the number of Merkle paths and the sponge's rows (defaults: n // 24, at least 3; what is left of 7/8 of the rows).
    The immediates of the later levels depend on n only, so two seeds give the same lists but for the first `leaves` operands.
    Returns pack_witness_plan's namespace plus expected (the matrix [135][n] from a zero matrix; None with expected=False),
    gate_of_row (indices into verifier_gateset()), c0, c1."""
    rng, fixed = np.random.default_rng(seed), np.random.default_rng(0x9E1F + n)
    npaths = max(3, n // 24) if paths is None else paths
    depths = [MERKLE_DEPTHS[i % len(MERKLE_DEPTHS)] for i in range(npaths)]
    second = [2 + (i & 1) for i in range(max(2, npaths // 2))]
    leaf_rows = (4 * npaths + 8 + ARITH_OPS - 1) // ARITH_OPS   # four digest elements per path and eight cells for the sponge
    used = npaths + leaf_rows + sum(depths) + 2 + sum(second)
    nsponge = n - n // 8 - used if sponge is None else sponge
    assert nsponge >= 2 and used + nsponge <= n, "the plan does not fit the rows"
    gs = verifier_gateset()
    G = {name: gs.index(name) for name in ("BaseSumGate", "ArithmeticGate", "ArithmeticExtensionGate", "PoseidonGate")}
    gate_of_row = np.full(n, gs.index("NoopGate"), dtype=np.int64)
    c0, c1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    rows = iter(range(n))

    def take(count, gate, consts=(0, 0)):
        out = [next(rows) for _ in range(count)]
        gate_of_row[out] = G[gate]
        c0[out], c1[out] = consts
        return out

    def f(r):
        return int(r.integers(0, P, dtype=np.uint64))

    ZERO, ONE = IMM(0), IMM(1)
    index_rows, arith_rows = take(npaths, "BaseSumGate"), take(leaf_rows, "ArithmeticGate", (1, 1))
    leaf = [(arith_rows[k // ARITH_OPS], k % ARITH_OPS) for k in range(4 * npaths + 8)]   # (row, op) of every leaf value
    leaf_cell = lambda k: CELL(leaf[k][0], 4 * leaf[k][1] + 3)   # noqa: E731
    level0 = [(r, REC_BASE_SUM, 0, [IMM(rng.integers(0, 1 << 63, dtype=np.uint64))]) for r in index_rows]
    level0 += [(r, REC_ARITHMETIC, op, [ONE, ONE, IMM(f(rng)), IMM(f(rng)), IMM(f(rng))]) for r, op in leaf]
    merkle, roots = [], []
    for p, depth in enumerate(depths):
        chain = []
        for k, r in enumerate(take(depth, "PoseidonGate")):
            digest = [leaf_cell(4 * p + i) for i in range(4)] if k == 0 else [PREV(i) for i in range(4)]
            chain.append((r, CELL(index_rows[p], 1 + k), digest + [IMM(f(fixed)) for _ in range(4)] + [ZERO] * 4))
        merkle.append(chain)
        roots.append(chain[-1][0])
    sponge_rows = take(nsponge, "PoseidonGate")
    cells = [leaf_cell(4 * npaths + i) for i in range(8)] + [CELL(r, 12 + i) for r in roots for i in range(4)]
    sponge_chain = []
    for k, r in enumerate(sponge_rows):
        fresh = [cells[(8 * k + i) % len(cells)] if (k + i) & 1 else IMM(f(fixed)) for i in range(8)]
        sponge_chain.append((r, ZERO, fresh + ([ZERO] * 4 if k == 0 else [PREV(8 + i) for i in range(4)])))
    (arow,), (xrow,) = take(1, "ArithmeticGate", (f(fixed), f(fixed))), take(1, "ArithmeticExtensionGate", (f(fixed), f(fixed)))
    last = sponge_rows[-1]
    out_cell = lambda k: CELL(roots[(k // 4) % npaths], 12 + k % 4) if k % 3 else CELL(last, 12 + k % 12)   # noqa: E731
    level3 = [(arow, REC_ARITHMETIC, op, [IMM(c0[arow]), IMM(c1[arow]), out_cell(3 * op), out_cell(3 * op + 1), out_cell(3 * op + 2)])
              for op in range(ARITH_OPS)]
    level3 += [(xrow, REC_ARITHMETIC_EXT, op, [IMM(c0[xrow]), IMM(c1[xrow])] + [out_cell(6 * op + i) for i in range(6)]) for op in range(ARITH_EXT_OPS)]
    later = []
    for g, length in enumerate(second):
        chain = []
        for k, r in enumerate(take(length, "PoseidonGate")):
            head = [CELL(arow, 4 * ((8 * g + i) % ARITH_OPS) + 3) if i & 1 else CELL(xrow, 8 * ((g + i) % ARITH_EXT_OPS) + 6 + (i >> 1 & 1)) for i in range(8)]
            chain.append((r, IMM(g & 1) if k == 0 else ZERO, head + [ZERO] * 4 if k == 0 else [PREV(i) for i in range(12)]))
        later.append(chain)
    plan = pack_witness_plan([(level0, []), ([], merkle), ([], [sponge_chain]), (level3, []), ([], later)])
    plan.expected = run_witness_plan(plan, REC_ROW_COLUMNS, n) if expected else None
    plan.gate_of_row, plan.c0, plan.c1 = gate_of_row, c0, c1
    return plan


def verifier_plan_circuit(params, plan, native=True):
    """the circuit a verifier_plan fills, like chain_circuit: its rows' gates and constants over verifier_gateset(), no copy
    constraints, no public inputs"""
    gs = verifier_gateset(native)
    n, NR = 1 << params.degree_bits, params.num_routed_wires
    assert n == plan.gate_of_row.size and params.num_constants == gs.num_selectors + 2 and params.num_wires >= REC_ROW_COLUMNS and NR >= 80
    rows = np.arange(n)
    k_is = gl.powers(7, NR)
    sig = sigma_values(np.tile(rows, (NR, 1)), np.tile(np.arange(NR)[:, None], (1, n)), k_is, params.degree_bits)
    cs = np.concatenate([gs.selector_columns(plan.gate_of_row), plan.c0[None, :], plan.c1[None, :], sig])
    return Circuit(params, gs, cs, k_is, 0), np.zeros(0, dtype=np.uint64)
