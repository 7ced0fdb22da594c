"""The degree the library derives from a gate program (lcp2_gate_program_degree, host only): it alone decides which gates K6
evaluates on half of the quotient coset, so it is held to plonky2's degrees of the gates this repository describes in Python
and to hand-written programs for the rules that those gates do not reach.  The light-client gate set of host/gates.cpp (the
four SHA-256 gates among it) is reached through tests/cpp/test_tiers.cpp, which calls the same function on its programs."""
import ctypes

import numpy as np
import pytest

import tier_lib


def _degree(m, words, num_regs=64):
    w = np.ascontiguousarray(np.array(words, dtype=np.uint32))
    out = ctypes.c_uint32(0xFFFFFFFF)
    rc = m.load_library().lcp2_gate_program_degree(w.ctypes.data_as(ctypes.c_void_p), w.size // 2, num_regs, ctypes.byref(out))
    return rc, out.value


def _gatesets(m):
    from eth_lc_plonky2_amd import recursion_gates as rg
    from eth_lc_plonky2_amd import u32_gates as ug
    return {"standard": m.circuit.standard_gateset(), "u32": ug.reference_gateset(native=False), "recursion": rg.recursion_gateset(native=False)}


@pytest.mark.parametrize("which", ["standard", "u32", "recursion"])
def test_derived_degree_is_the_declared_gate_degree(which):
    """every gate of the Python gate sets: the library's number equals the restatement in tier_lib and the degree the gate set
    declares (plonky2's Gate::degree(), by which the selector groups are formed)"""
    import eth_lc_plonky2_amd as m
    gs = _gatesets(m)[which]
    want = tier_lib.gateset_degrees(gs)
    for g, G in enumerate(gs.gates):
        rc, got = _degree(m, gs.code[2 * G.code_offset:2 * (G.code_offset + G.code_len)], gs.max_regs)
        print(which, gs.names[g], "declared", gs.degrees[g], "derived", got)
        assert rc == 0 and got == want[g], gs.names[g]
        assert got == gs.degrees[g], gs.names[g]


def test_named_gates():
    import eth_lc_plonky2_amd as m
    gs = m.circuit.standard_gateset()
    deg = dict(zip(gs.names, tier_lib.gateset_degrees(gs)))
    assert deg == {"NoopGate": 0, "ConstantGate": 1, "PublicInputGate": 1, "BaseSumGate": 2, "ArithmeticGate": 3, "PoseidonGate": 7}


def test_hand_written_rules():
    import eth_lc_plonky2_amd as m
    cm = m.circuit
    R, W, C, PI = cm.R, cm.W, cm.C, cm.PI

    def prog(build):
        asm = cm.GateAsm(cm.ImmTable())
        build(asm)
        return asm.words

    def sbox_of_product(a):
        a.sbox(a.mul(W(0), W(1)), 5)
        a.emit(R(5))
    assert _degree(m, prog(sbox_of_product)) == (0, 14)

    def muladd_keeps_the_larger(a):   # dst of degree 3, product of degree 2; then dst of degree 1, product of degree 2
        r = a.mul(a.mul(W(0), W(1)), C(0))
        a.muladd(r, W(2), W(3))
        a.emit(r)
    assert _degree(m, prog(muladd_keeps_the_larger)) == (0, 3)

    def muladd_takes_the_product(a):
        r = a.add(W(0), PI(1))
        a.muladd(r, W(2), W(3))
        a.emit(r)
    assert _degree(m, prog(muladd_takes_the_product)) == (0, 2)

    def emitbool_doubles(a):
        a.emit(W(0))
        a.emit_bool(a.mul(W(1), W(2)))
    assert _degree(m, prog(emitbool_doubles)) == (0, 4)

    def xor_is_a_product(a):
        a.emit(a.xor(a.xor(W(0), W(1)), W(2)))
    assert _degree(m, prog(xor_is_a_product)) == (0, 3)

    def constants_only(a):
        a.emit(a.dbladd(a.imm(5), PI(0)))
    assert _degree(m, prog(constants_only)) == (0, 0)
    assert _degree(m, [])[0] == 0
    assert _degree(m, [15, 0])[0] != 0                                  # no such op
    assert _degree(m, [cm.OP_ADD | 9 << 8, 0], num_regs=4)[0] != 0       # destination past the registers
    for t in (sbox_of_product, emitbool_doubles, muladd_keeps_the_larger):
        assert tier_lib.program_degree(prog(t)) == _degree(m, prog(t))[1]

    # saturation: degrees stop at 2^20.  7^7 = 823543 is the last power of 7 below it; the expected numbers are tier_lib's
    def sbox_chain(n, then):
        def build(a):
            x = W(0)
            for _ in range(n):
                x = a.sbox(x, 5)
            then(a, x)
        return build

    def muladd_into_saturated(a, x):   # dst at the cap, product of degree 2: the cap stays
        a.muladd(x, W(1), W(2))
        a.emit(x)

    def product_of_saturated(a, x):    # cap + cap, and the XOR of the result with a wire
        a.emit(a.xor(a.mul(x, x), W(1)))
    cap = 1 << 20
    for build, want in [(sbox_chain(7, lambda a, x: a.emit(x)), 7 ** 7),                   # below the cap: exact
                        (sbox_chain(7, lambda a, x: a.emit_bool(x)), cap),                 # 2 * 7^7 is past it
                        (sbox_chain(8, lambda a, x: a.emit(x)), cap),                      # 7^8 is past it
                        (sbox_chain(8, lambda a, x: a.emit_bool(x)), cap),                 # twice the cap is the cap
                        (sbox_chain(12, lambda a, x: a.emit_bool(x)), cap),                # and stays there (7^12 would pass 2^32)
                        (sbox_chain(8, muladd_into_saturated), cap),
                        (sbox_chain(8, product_of_saturated), cap),
                        (sbox_chain(2, muladd_into_saturated), 49)]:                       # MULADD into a register of a higher degree
        assert tier_lib.program_degree(prog(build)) == want
        assert _degree(m, prog(build)) == (0, want)


def test_host_layer_gate_set_against_gate_degree():
    """host/gates.cpp: the derived degree of every program of build_gate_set equals GATE_DEGREE, the four SHA-256 gates (XOR, EMITBOOL
    and DBLADD chains of a hundred constraints) at 2, 3, 3, 3"""
    r = tier_lib.run_tiers_binary("degrees")
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("degree ")]
    got = {name: int(d) for _, name, d, _ in rows}
    declared = {name: int(d) for _, name, _, d in rows}
    print(got)
    assert got == declared
    assert got == {"NoopGate": 0, "ConstantGate": 1, "PublicInputGate": 1, "ShaAddGate": 2, "ArithmeticGate": 3, "ShaRoundAGate": 3,
                   "ShaRoundEGate": 3, "ShaScheduleGate": 3, "PoseidonGate": 7}
