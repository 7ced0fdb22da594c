"""ctypes binding of the C ABI declared in include/lcp2.h.

This is the same shape of stub a Rust `plonky2` fork would write with `extern "C"`
(see INTEGRATION.md); Python is used here only because the image has no Rust
toolchain.  There is no CPU fallback: if liblcp2.so is missing or no HIP device
is usable, calls raise `Lcp2Error`.
"""
import ctypes
import os

import numpy as np

from . import build as _build

u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)
MEM_HOST, MEM_DEVICE = 0, 1
VERIFY_HEADS = {"host": 0, "device": 1}  # LCP2_VERIFY_HEAD_HOST, LCP2_VERIFY_HEAD_DEVICE
E_UNSAT = -5
SECTION_OPENINGS, SECTION_FRI_CAP0, SECTION_AFTER_CAPS = 0, 1, 2

K_INTT, K_LDE, K_LEAF_HASH, K_MERKLE, K_PERM_Z, K_QUOTIENT, K_OPENINGS, K_FRI, K_POW, K_SHA256, K_OTHER = range(11)
KERNEL_FAMILIES = ["intt", "lde", "leaf_hash", "merkle", "perm_z", "quotient", "openings", "fri", "pow", "sha256", "other"]

GOLDILOCKS_P = 0xFFFFFFFF00000001


class Lcp2Error(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"lcp2 status {status}: {message}")
        self.status = status


class Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "degree_bits", "num_wires", "num_routed_wires", "num_constants", "rate_bits", "cap_height",
        "num_challenges", "quotient_degree_factor", "proof_of_work_bits", "num_query_rounds", "num_fri_layers")]
    _fields_.append(("fri_arity_bits", ctypes.c_uint32 * 8))


class CircuitDesc(ctypes.Structure):
    _fields_ = [("params", Params), ("constants_sigmas", ctypes.c_void_p), ("constants_sigmas_mem", ctypes.c_int),
                ("k_is", ctypes.c_void_p), ("num_selectors", ctypes.c_uint32), ("num_gates", ctypes.c_uint32),
                ("gates", ctypes.c_void_p), ("code", ctypes.c_void_p), ("code_words", ctypes.c_size_t),
                ("imm", ctypes.c_void_p), ("num_imm", ctypes.c_size_t), ("num_public_inputs", ctypes.c_uint32),
                ("num_regs", ctypes.c_uint32)]


class CircuitRows(ctypes.Structure):
    """lcp2_circuit_rows: what lcp2_circuit_rows_expand / lcp2_circuit_create_from_rows build the preprocessed columns from"""
    _fields_ = [("gate_of_row", ctypes.c_void_p), ("num_rows", ctypes.c_size_t), ("pad_gate", ctypes.c_uint32), ("row_constants", ctypes.c_void_p),
                ("bindings", ctypes.c_void_p), ("num_bindings", ctypes.c_size_t), ("bindings_mem", ctypes.c_int), ("num_classes", ctypes.c_uint32)]


BINDING_DTYPE = np.dtype([("row", "<u4"), ("col", "<u4"), ("cls", "<u4")])   # lcp2_copy_binding as a numpy record
assert BINDING_DTYPE.itemsize == 12


class ProofLayout(ctypes.Structure):
    """lcp2_proof_layout: word offsets of every field of the flat proof"""
    _fields_ = ([(n, ctypes.c_uint64) for n in ("cap_words", "wires_cap", "zs_cap", "quot_cap", "op_constants", "op_sigmas", "op_wires", "op_zs",
                                                "op_zs_next", "op_partial_products", "op_quotient", "fri_caps", "queries", "query_words")]
                + [("q_init_off", ctypes.c_uint64 * 4), ("q_init_cols", ctypes.c_uint64 * 4), ("q_init_sib", ctypes.c_uint64),
                   ("q_step_off", ctypes.c_uint64 * 8), ("q_step_sib", ctypes.c_uint64 * 8)]
                + [(n, ctypes.c_uint64) for n in ("final_poly", "final_len", "pow_witness", "total")])


class U32Job(ctypes.Structure):
    """lcp2_u32_job: one operation of a plonky2_u32 / comparison row (lcp2_u32_gate_rows)"""
    _fields_ = [("row", ctypes.c_uint32), ("kind", ctypes.c_uint16), ("op", ctypes.c_uint16), ("inputs", ctypes.c_uint32 * 4)]


U32_ARITHMETIC, U32_ADD_MANY, U32_SUBTRACTION, U32_RANGE_CHECK, U32_COMPARISON = range(5)
U32_JOB_DTYPE = np.dtype([("row", "<u4"), ("kind", "<u2"), ("op", "<u2"), ("in", "<u4", (4,))])   # U32Job as a numpy record
assert U32_JOB_DTYPE.itemsize == ctypes.sizeof(U32Job) == 24
POSEIDON_ROW_DTYPE = np.dtype([("row", "<u4"), ("swap", "<u4"), ("in", "<u8", (12,))])   # lcp2_poseidon_row as a numpy record
assert POSEIDON_ROW_DTYPE.itemsize == 104
SHA_JOB_DTYPE = np.dtype([("first_row", "<u4"), ("in_src", "<i4", (16,))])   # lcp2_sha_job as a numpy record
CELL_DTYPE = np.dtype([("row", "<u4"), ("col", "<u4"), ("value", "<u8")])      # lcp2_cell as a numpy record
CELL_REF_DTYPE = np.dtype([("row", "<u4"), ("col", "<u4")])                      # lcp2_cell_ref as a numpy record
assert SHA_JOB_DTYPE.itemsize == 68 and CELL_DTYPE.itemsize == 16 and CELL_REF_DTYPE.itemsize == 8
SHA_ROWS, SHA_ROW_COLUMNS = 310, 108   # rows of one two_to_one_sha256, columns lcp2_sha256_witness writes in each

class RecOperand(ctypes.Structure):
    """lcp2_rec_operand: an immediate value, or a cell (row v, column col) of the witness matrix (lcp2_rec_gate_rows)"""
    _fields_ = [("v", ctypes.c_uint64), ("col", ctypes.c_uint32), ("src", ctypes.c_uint32)]


class RecJob(ctypes.Structure):
    """lcp2_rec_job: one operation of a recursion-gate row; its operands start at operands[first_operand]"""
    _fields_ = [("row", ctypes.c_uint32), ("kind", ctypes.c_uint16), ("op", ctypes.c_uint16), ("first_operand", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


(REC_ARITHMETIC, REC_BASE_SUM, REC_ARITHMETIC_EXT, REC_MUL_EXT, REC_REDUCING, REC_REDUCING_EXT, REC_POSEIDON_MDS, REC_RANDOM_ACCESS,
 REC_EXPONENTIATION, REC_COSET_INTERPOLATION, REC_KINDS) = range(11)
REC_IMM, REC_CELL = 0, 1
REC_OPERAND_DTYPE = np.dtype([("v", "<u8"), ("col", "<u4"), ("src", "<u4")])   # RecOperand as a numpy record
REC_JOB_DTYPE = np.dtype([("row", "<u4"), ("kind", "<u2"), ("op", "<u2"), ("first_operand", "<u4"), ("reserved", "<u4")])
assert REC_OPERAND_DTYPE.itemsize == ctypes.sizeof(RecOperand) == 16 and REC_JOB_DTYPE.itemsize == ctypes.sizeof(RecJob) == 16
PLAN_IMM, PLAN_CELL, PLAN_PREV = 0, 1, 2   # src of a PoseidonGate operand of a witness plan; PREV: output `col` of the chain's previous job
POS_JOB_DTYPE = np.dtype([("row", "<u4"), ("first_operand", "<u4")])   # lcp2_pos_job: 13 operands, swap then in[0..11]
assert POS_JOB_DTYPE.itemsize == 8


class WitnessPlan(ctypes.Structure):
    """lcp2_witness_plan: rec jobs and PoseidonGate chains over one operand list, in levels (lcp2_witness_plan_rows)"""
    _fields_ = [("rec_jobs", ctypes.c_void_p), ("nrec", ctypes.c_size_t), ("rec_level_ends", ctypes.c_void_p),
                ("pos_jobs", ctypes.c_void_p), ("npos", ctypes.c_size_t), ("chain_ends", ctypes.c_void_p), ("nchains", ctypes.c_size_t),
                ("pos_level_ends", ctypes.c_void_p), ("operands", ctypes.c_void_p), ("noperands", ctypes.c_size_t), ("nlevels", ctypes.c_size_t)]


class U32PlanJob(ctypes.Structure):
    """lcp2_u32_plan_job: one operation of a plonky2_u32 / comparison row whose inputs are operands[first_operand ..] of a plan"""
    _fields_ = [("row", ctypes.c_uint32), ("kind", ctypes.c_uint16), ("op", ctypes.c_uint16), ("first_operand", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


U32_PLAN_JOB_DTYPE = REC_JOB_DTYPE   # the same 16-byte record; kind is U32_*
U32_PLAN_OPERANDS = {U32_ARITHMETIC: 3, U32_ADD_MANY: 4, U32_SUBTRACTION: 3, U32_RANGE_CHECK: 1, U32_COMPARISON: 2}
assert ctypes.sizeof(U32PlanJob) == U32_PLAN_JOB_DTYPE.itemsize == 16


class WitnessPlanU32(ctypes.Structure):
    """lcp2_witness_plan_u32: a witness plan that also holds u32 jobs, in the same levels (lcp2_witness_plan_rows_u32)"""
    _fields_ = [("base", WitnessPlan), ("u32_jobs", ctypes.c_void_p), ("nu32", ctypes.c_size_t), ("u32_level_ends", ctypes.c_void_p)]


SHA_PLAN_JOB_DTYPE = np.dtype([("first_row", "<u4"), ("first_operand", "<u4")])   # lcp2_sha_plan_job: 16 operands, W0..W15
SHA_PLAN_OPERANDS = 16
assert SHA_PLAN_JOB_DTYPE.itemsize == 8


class WitnessPlanSha(ctypes.Structure):
    """lcp2_witness_plan_sha: a witness plan that also holds SHA-256 jobs, in the same levels (lcp2_witness_plan_rows_sha)"""
    _fields_ = [("base", WitnessPlanU32), ("sha_jobs", ctypes.c_void_p), ("nsha", ctypes.c_size_t), ("sha_level_ends", ctypes.c_void_p)]


_lib = None


class WitnessReport(ctypes.Structure):
    """lcp2_witness_report: what lcp2_check_witness found (include/lcp2.h)"""
    _fields_ = [("gate_violations", ctypes.c_uint64), ("gate_row", ctypes.c_uint64), ("gate_index", ctypes.c_uint32), ("gate_constraint", ctypes.c_uint32),
                ("copy_violations", ctypes.c_uint64), ("copy_row", ctypes.c_uint64), ("copy_wire", ctypes.c_uint32),
                ("copy_to_row", ctypes.c_uint64), ("copy_to_wire", ctypes.c_uint32), ("noncanonical_cells", ctypes.c_uint64)]
    per_gate = None   # gate_violations split by gate (numpy, num_gates), when it was asked for

    @property
    def ok(self):
        """no gate and no copy violation"""
        return self.gate_violations == 0 and self.copy_violations == 0

    def __repr__(self):
        return "WitnessReport(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class FillReport(ctypes.Structure):
    """lcp2_fill_report: what lcp2_witness_fill_copies did (include/lcp2.h)"""
    _fields_ = [(f, ctypes.c_uint64) for f in ("num_classes", "classes_set", "cells_filled", "conflicts", "conflict_index", "owner_index")]
    unsat = False   # the call returned LCP2_E_UNSAT: conflicts > 0, the classes hold their owners' values
    message = ""    # lcp2_last_error of such a call: both list indices, both cells

    def __repr__(self):
        return "FillReport(%s, unsat=%s)" % (", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_), self.unsat)


class ChallengerState(ctypes.Structure):
    """lcp2_challenger: plonky2's Challenger { sponge_state, input_buffer, output_buffer } by value"""
    _fields_ = [("sponge", ctypes.c_uint64 * 12), ("input", ctypes.c_uint64 * 8), ("output", ctypes.c_uint64 * 8),
                ("input_len", ctypes.c_uint32), ("output_len", ctypes.c_uint32)]


class FriConfig(ctypes.Structure):
    """lcp2_fri_config: a FriConfig with its reduction schedule"""
    _fields_ = [("rate_bits", ctypes.c_uint32), ("cap_height", ctypes.c_uint32), ("proof_of_work_bits", ctypes.c_uint32),
                ("num_query_rounds", ctypes.c_uint32), ("num_fri_layers", ctypes.c_uint32), ("fri_arity_bits", ctypes.c_uint32 * 8)]


class FriRange(ctypes.Structure):
    _fields_ = [("oracle", ctypes.c_uint32), ("first_poly", ctypes.c_uint32), ("num_polys", ctypes.c_uint32)]


class FriInstance(ctypes.Structure):
    """lcp2_fri_instance (plonky2 FriInstanceInfo): build one with fri_instance(), which keeps the range arrays alive"""
    _fields_ = [("num_oracles", ctypes.c_uint32), ("num_points", ctypes.c_uint32), ("num_ranges", ctypes.c_uint32 * 4),
                ("ranges", ctypes.POINTER(FriRange) * 4)]


class StarkProgram(ctypes.Structure):
    _fields_ = [("code_offset", ctypes.c_uint32), ("code_len", ctypes.c_uint32), ("num_constraints", ctypes.c_uint32)]


class StarkDesc(ctypes.Structure):
    """lcp2_stark_desc: build one with stark.pack_stark_desc(), which keeps the code and immediate arrays alive"""
    _fields_ = [("log_n", ctypes.c_uint32), ("width", ctypes.c_uint32), ("num_public_inputs", ctypes.c_uint32), ("num_challenges", ctypes.c_uint32),
                ("quotient_degree_bits", ctypes.c_uint32), ("fri", FriConfig), ("first_row", StarkProgram), ("transition", StarkProgram),
                ("last_row", StarkProgram), ("code", ctypes.c_void_p), ("code_words", ctypes.c_size_t), ("imm", ctypes.c_void_p),
                ("num_imm", ctypes.c_size_t), ("num_regs", ctypes.c_uint32)]


class StarkViolation(ctypes.Structure):
    """lcp2_stark_violation: kind 0 first / 1 transition / 2 last, the constraint's index within its program, the row; kind 3: the
    running product of Z number `constraint` of a permutation argument does not close (row n - 1)"""
    _fields_ = [("kind", ctypes.c_uint32), ("constraint", ctypes.c_uint32), ("row", ctypes.c_uint64)]


class StarkPermPair(ctypes.Structure):
    _fields_ = [("first", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class StarkPerm(ctypes.Structure):
    """lcp2_stark_perm: build one with stark.pack_stark_perm(), which keeps the pair and column arrays alive"""
    _fields_ = [("num_pairs", ctypes.c_uint32), ("pairs", ctypes.c_void_p), ("columns", ctypes.c_void_p), ("num_column_pairs", ctypes.c_size_t),
                ("batch_size", ctypes.c_uint32)]


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so.  Two HIP runtimes in one
    process cannot both own the GPU, and torch tensors / streams are only meaningful to the runtime that made
    them, so when torch is installed its runtime is loaded first (RTLD_GLOBAL): liblcp2.so's dependency on
    SONAME libamdhip64.so.7 then binds to that same copy.  Without torch the system ROCm runtime is used."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        cand = os.path.join(libdir, name)
        if os.path.exists(cand):
            try:
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                return


def load_library():
    """Loads (building if the sources are newer) eth-lc-plonky2_amd/liblcp2.so."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if not os.path.exists(path):
        path = _build.build_native()
    _share_torch_hip_runtime()
    lib = ctypes.CDLL(path)
    c = ctypes
    sigs = {
        "lcp2_status_str": (c.c_char_p, [c.c_int]),
        "lcp2_abi_version": (c.c_int, []),
        "lcp2_device_count": (c.c_int, []),
        "lcp2_params_standard": (c.c_int, [c.c_uint32, c.c_uint32, c.POINTER(Params)]),
        "lcp2_params_config": (c.c_int, [c.c_uint32] * 8 + [c.POINTER(Params)]),
        "lcp2_ctx_create": (c.c_int, [c.c_int, c.c_void_p, c.POINTER(c.c_void_p)]),
        "lcp2_ctx_create_ex": (c.c_int, [c.c_int, c.c_void_p, c.c_uint32, c.POINTER(c.c_void_p)]),
        "lcp2_ctx_destroy": (None, [c.c_void_p]),
        "lcp2_ctx_sync": (c.c_int, [c.c_void_p]),
        "lcp2_ctx_stream": (c.c_void_p, [c.c_void_p]),
        "lcp2_last_error": (c.c_char_p, [c.c_void_p]),
        "lcp2_poseidon_permute_batch": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_int]),
        "lcp2_field_op_batch": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint32, c.c_int]),
        "lcp2_merkle_cap": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_uint32, c.c_int, c.c_void_p]),
        "lcp2_ntt_batch": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint32, c.c_int, c.c_uint64, c.c_int]),
        "lcp2_lde_batch": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint32, c.c_uint32, c.c_int]),
        "lcp2_sha256_tree": (c.c_int, [c.c_void_p, c.c_void_p, c.c_uint32, c.c_size_t, c.c_void_p, c.c_void_p, c.c_int]),
        "lcp2_sha256_witness": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint64, c.c_void_p]),
        "lcp2_scatter_cells": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint64]),
        "lcp2_poseidon_gate_rows": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint64]),
        "lcp2_u32_gate_rows": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p, c.c_uint64]),
        "lcp2_rec_gate_rows": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p,
                                         c.c_uint32, c.c_uint64]),
        "lcp2_witness_plan_rows": (c.c_int, [c.c_void_p, c.POINTER(WitnessPlan), c.c_int, c.c_void_p, c.c_uint32, c.c_uint64]),
        "lcp2_witness_plan_rows_u32": (c.c_int, [c.c_void_p, c.POINTER(WitnessPlanU32), c.c_int, c.c_void_p, c.c_uint32, c.c_uint64]),
        "lcp2_witness_plan_rows_sha": (c.c_int, [c.c_void_p, c.POINTER(WitnessPlanSha), c.c_int, c.c_void_p, c.c_uint32, c.c_uint64]),
        "lcp2_commit_wires_rows_begin": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_commit_wires_chunk": (c.c_int, [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32]),
        "lcp2_commit_wires_rows_finish": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_host_register": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t]),
        "lcp2_host_unregister": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_witness_stage": (c.c_int, [c.c_void_p, c.c_void_p, c.c_uint32]),
        "lcp2_prove_staged": (c.c_int, [c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]),
        "lcp2_buffer_alloc": (c.c_int, [c.c_void_p, c.c_size_t, c.POINTER(c.c_void_p)]),
        "lcp2_buffer_free": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_buffer_zero": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t]),
        "lcp2_buffer_read": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]),
        "lcp2_buffer_write": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]),
        "lcp2_buffer_copy": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]),
        "lcp2_buffer_copy_2d": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t]),
        "lcp2_commit_values": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.POINTER(c.c_void_p), c.c_void_p]),
        "lcp2_commit_coeffs": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.POINTER(c.c_void_p), c.c_void_p]),
        "lcp2_commit_cosets": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.POINTER(c.c_void_p), c.c_void_p]),
        "lcp2_oracle_destroy": (None, [c.c_void_p]),
        "lcp2_oracle_open": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]),
        "lcp2_oracle_read": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_circuit_create": (c.c_int, [c.c_void_p, c.POINTER(CircuitDesc), c.POINTER(c.c_void_p)]),
        "lcp2_circuit_rows_expand": (c.c_int, [c.c_void_p, c.POINTER(CircuitDesc), c.POINTER(CircuitRows), c.c_void_p]),
        "lcp2_circuit_create_from_rows": (c.c_int, [c.c_void_p, c.POINTER(CircuitDesc), c.POINTER(CircuitRows), c.POINTER(c.c_void_p)]),
        "lcp2_verifier_create": (c.c_int, [c.POINTER(CircuitDesc), c.c_void_p, c.c_void_p, c.POINTER(c.c_void_p)]),
        "lcp2_circuit_destroy": (None, [c.c_void_p]),
        "lcp2_circuit_digest": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_proof_words": (c.c_size_t, [c.POINTER(Params)]),
        "lcp2_proof_layout_of": (c.c_int, [c.POINTER(Params), c.POINTER(ProofLayout)]),
        "lcp2_prove": (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]),
        "lcp2_witness_fill_copies": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p, c.POINTER(FillReport)]),
        "lcp2_circuit_copy_classes": (c.c_int, [c.c_void_p, c.c_void_p, c.POINTER(c.c_uint64)]),
        "lcp2_witness_settle_copies": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p, c.POINTER(FillReport)]),
        "lcp2_check_witness": (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_size_t, c.POINTER(WitnessReport), c.c_void_p, c.c_uint32]),
        "lcp2_commit_wires": (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_void_p]),
        "lcp2_commit_wires_coeffs": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_commit_wires_rows": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_perm_zs_rows_begin": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_perm_zs_rows_finish": (c.c_int, [c.c_void_p, c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_size_t)]),
        "lcp2_perm_zs_commit": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_perm_zs": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_quotient": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_fri_open": (c.c_int, [c.c_void_p, c.c_void_p, c.POINTER(ChallengerState), c.c_void_p]),
        "lcp2_fri_open_begin": (c.c_int, [c.c_void_p, c.c_void_p, c.POINTER(ChallengerState), c.c_void_p]),
        "lcp2_fri_open_commit": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_fri_open_finish": (c.c_int, [c.c_void_p, c.POINTER(ChallengerState), c.c_void_p]),
        "lcp2_proof_section": (c.c_int, [c.c_void_p, c.c_int, c.POINTER(c.c_size_t), c.POINTER(c.c_size_t)]),
        "lcp2_challenger_init": (None, [c.POINTER(ChallengerState)]),
        "lcp2_challenger_observe": (c.c_int, [c.POINTER(ChallengerState), c.c_void_p, c.c_size_t]),
        "lcp2_challenger_get": (c.c_int, [c.POINTER(ChallengerState), c.c_void_p, c.c_size_t]),
        "lcp2_hash_no_pad": (c.c_int, [c.c_void_p, c.c_size_t, c.c_void_p]),
        "lcp2_fri_config_of": (c.c_int, [c.c_uint32] * 7 + [c.POINTER(FriConfig)]),
        "lcp2_oracle_eval": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]),
        "lcp2_fri_openings_words": (c.c_size_t, [c.POINTER(FriConfig), c.c_uint32, c.c_void_p, c.POINTER(FriInstance)]),
        "lcp2_fri_prove_openings": (c.c_int, [c.c_void_p, c.c_void_p, c.POINTER(FriInstance), c.c_void_p, c.POINTER(FriConfig),
                                              c.POINTER(ChallengerState), c.c_void_p, c.c_size_t]),
        "lcp2_fri_verify_openings": (c.c_int, [c.c_void_p, c.c_void_p, c.c_uint32, c.POINTER(FriInstance), c.c_void_p, c.POINTER(FriConfig),
                                               c.POINTER(ChallengerState), c.c_void_p, c.c_size_t, c.POINTER(c.c_int32)]),
        "lcp2_stark_proof_words": (c.c_size_t, [c.POINTER(StarkDesc)]),
        "lcp2_stark_prove": (c.c_int, [c.c_void_p, c.POINTER(StarkDesc), c.c_void_p, c.c_int, c.c_void_p, c.POINTER(ChallengerState), c.c_void_p,
                                       c.c_size_t, c.POINTER(StarkViolation)]),
        "lcp2_stark_verify": (c.c_int, [c.POINTER(StarkDesc), c.c_void_p, c.POINTER(ChallengerState), c.c_void_p, c.c_size_t, c.POINTER(c.c_int32)]),
        "lcp2_stark_perm_proof_words": (c.c_size_t, [c.POINTER(StarkDesc), c.POINTER(StarkPerm)]),
        "lcp2_stark_prove_perm": (c.c_int, [c.c_void_p, c.POINTER(StarkDesc), c.POINTER(StarkPerm), c.c_void_p, c.c_int, c.c_void_p, c.POINTER(ChallengerState),
                                            c.c_void_p, c.c_size_t, c.POINTER(StarkViolation)]),
        "lcp2_stark_verify_perm": (c.c_int, [c.POINTER(StarkDesc), c.POINTER(StarkPerm), c.c_void_p, c.POINTER(ChallengerState), c.c_void_p, c.c_size_t,
                                             c.POINTER(c.c_int32)]),
        "lcp2_circuit_create_sharded": (c.c_int, [c.c_void_p, c.POINTER(CircuitDesc), c.c_uint32, c.c_uint32, c.POINTER(c.c_void_p)]),
        "lcp2_circuit_set_constants_cap": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_quotient_values": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p]),
        "lcp2_quotient_buffer": (c.c_int, [c.c_void_p, c.POINTER(c.c_void_p), c.POINTER(c.c_size_t)]),
        "lcp2_quotient_commit": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_verify": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_int)]),
        "lcp2_verify_batch": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p]),
        "lcp2_verify_batch_ex": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p,
                                           c.c_uint32]),
        "lcp2_proof_compressed_words_max": (c.c_size_t, [c.POINTER(Params)]),
        "lcp2_proof_compress": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]),
        "lcp2_proof_decompress": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]),
        "lcp2_verify_batch_compressed": (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p,
                                                   c.c_uint32]),
        "lcp2_last_challenges": (c.c_int, [c.c_void_p, c.c_void_p]),
        "lcp2_gate_program_degree": (c.c_int, [c.c_void_p, c.c_size_t, c.c_uint32, c.POINTER(c.c_uint32)]),
        "lcp2_circuit_gate_tiers": (c.c_int, [c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p]),
        "lcp2_proof_bytes": (c.c_size_t, [c.POINTER(Params), c.c_size_t, c.c_uint32]),
        "lcp2_proof_to_bytes": (c.c_int, [c.POINTER(Params), c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_uint32, c.c_void_p, c.c_size_t]),
        "lcp2_proof_from_bytes": (c.c_int, [c.POINTER(Params), c.c_void_p, c.c_size_t, c.c_uint32, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]),
        "lcp2_verifier_data_to_bytes": (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t]),
        "lcp2_prof_enable": (c.c_int, [c.c_void_p, c.c_int]),
        "lcp2_prof_reset": (c.c_int, [c.c_void_p]),
        "lcp2_prof_get": (c.c_int, [c.c_void_p, c.c_int, c.POINTER(c.c_double), c.POINTER(c.c_uint64), c.POINTER(c.c_double)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError here = the library does not export what lcp2.h declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS = None  # filled by tests from include/lcp2.h


def _np_u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def standard_params(degree_bits, num_constants=4):
    lib = load_library()
    p = Params()
    rc = lib.lcp2_params_standard(degree_bits, num_constants, ctypes.byref(p))
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    return p


def params_config(degree_bits, num_constants=4, rate_bits=3, cap_height=4, proof_of_work_bits=16, num_query_rounds=28,
                  arity_bits=4, final_poly_bits=5):
    """lcp2_params_config: the standard wire shape under a FriConfig with ConstantArityBits(arity_bits, final_poly_bits)"""
    lib = load_library()
    p = Params()
    rc = lib.lcp2_params_config(degree_bits, num_constants, rate_bits, cap_height, proof_of_work_bits, num_query_rounds,
                                arity_bits, final_poly_bits, ctypes.byref(p))
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    return p


def fri_config(log_n, rate_bits=3, cap_height=4, proof_of_work_bits=16, num_query_rounds=28, arity_bits=4, final_poly_bits=5, schedule=None):
    """lcp2_fri_config_of: a FriConfig for polynomials of 2^log_n coefficients under ConstantArityBits(arity_bits, final_poly_bits);
    schedule: a list of arity bits to use instead of the derived one"""
    lib, cfg = load_library(), FriConfig()
    rc = lib.lcp2_fri_config_of(log_n, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, arity_bits, final_poly_bits, ctypes.byref(cfg))
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    if schedule is not None:
        cfg.num_fri_layers = len(schedule)
        for i in range(8):
            cfg.fri_arity_bits[i] = schedule[i] if i < len(schedule) else 0
    return cfg


def fri_instance(num_oracles, points_ranges):
    """lcp2_fri_instance from points_ranges = [[(oracle, first_poly, num_polys), ...] per point]; the arrays live in the result"""
    inst = FriInstance()
    inst.num_oracles, inst.num_points = num_oracles, len(points_ranges)
    inst._keep = []
    for b, ranges in enumerate(points_ranges[:4]):
        arr = (FriRange * max(len(ranges), 1))(*[FriRange(*r) for r in ranges])
        inst._keep.append(arr)
        inst.num_ranges[b] = len(ranges)
        inst.ranges[b] = ctypes.cast(arr, ctypes.POINTER(FriRange))
    return inst


def fri_openings_words(cfg, log_n, oracle_cols, inst):
    """lcp2_fri_openings_words: the length of the proof of lcp2_fri_prove_openings, 0 for a refused shape"""
    cols = np.ascontiguousarray(oracle_cols, dtype=np.uint32)
    return load_library().lcp2_fri_openings_words(ctypes.byref(cfg), log_n, _ptr(cols), ctypes.byref(inst))


def fri_verify_openings(caps, oracle_cols, log_n, inst, points, cfg, challenger_state, proof):
    """lcp2_fri_verify_openings (host only): 0 if accepted, else the failed check 1..7; Lcp2Error for a refused call.
    challenger_state is updated to the state after the query indices."""
    lib = load_library()
    caps = [np.ascontiguousarray(np.asarray(c, dtype=np.uint64).ravel()) for c in caps]
    cap_ptrs = (ctypes.c_void_p * len(caps))(*[c.ctypes.data for c in caps])
    cols = np.ascontiguousarray(oracle_cols, dtype=np.uint32)
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).ravel())
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    failed = ctypes.c_int32(0)
    rc = lib.lcp2_fri_verify_openings(cap_ptrs, _ptr(cols), log_n, ctypes.byref(inst), _ptr(pts), ctypes.byref(cfg), ctypes.byref(challenger_state),
                                      _ptr(pr), pr.size, ctypes.byref(failed))
    if rc == 0:
        return 0
    if rc == -7:
        return failed.value
    raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())


def stark_proof_words(desc, perm=None):
    """lcp2_stark_proof_words (with perm, a StarkPerm: lcp2_stark_perm_proof_words): the length of the proof of lcp2_stark_prove, 0 for
    a refused description"""
    if perm is None:
        return load_library().lcp2_stark_proof_words(ctypes.byref(desc))
    return load_library().lcp2_stark_perm_proof_words(ctypes.byref(desc), ctypes.byref(perm))


def stark_verify(desc, public_inputs, challenger_state, proof, perm=None):
    """lcp2_stark_verify (with perm, a StarkPerm: lcp2_stark_verify_perm; host only): 0 if accepted, else the failed check 1..9;
    Lcp2Error for a refused call.  challenger_state is updated as the verifier leaves it."""
    lib = load_library()
    pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    failed = ctypes.c_int32(0)
    if perm is None:
        rc = lib.lcp2_stark_verify(ctypes.byref(desc), _ptr(pis), ctypes.byref(challenger_state), _ptr(pr), pr.size, ctypes.byref(failed))
    else:
        rc = lib.lcp2_stark_verify_perm(ctypes.byref(desc), ctypes.byref(perm), _ptr(pis), ctypes.byref(challenger_state), _ptr(pr), pr.size, ctypes.byref(failed))
    if rc == 0:
        return 0
    if rc == -7:
        return failed.value
    raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())


class Oracle:
    """PolynomialBatch handle (device resident)."""

    def __init__(self, ctx, handle, ncols, log_n, rate_bits, cap_height, cap):
        self.ctx, self.handle = ctx, handle
        self.ncols, self.log_n, self.rate_bits, self.cap_height = ncols, log_n, rate_bits, cap_height
        self.cap = cap
        self.block_first, self.block_count = 0, 1 << rate_bits  # a coset-sharded oracle holds fewer leaf blocks

    def open(self, indices):
        idx = _np_u64(indices)
        k = idx.size
        nsib = self.log_n + self.rate_bits - self.cap_height  # the same for a coset-sharded oracle: local cap = global cap slice
        leaves = np.zeros((k, self.ncols), dtype=np.uint64)
        sib = np.zeros((k, max(nsib, 0), 4), dtype=np.uint64)
        self.ctx._check(self.ctx.lib.lcp2_oracle_open(self.handle, _ptr(idx), k, _ptr(leaves), _ptr(sib)))
        return leaves, sib

    def eval(self, points):
        """lcp2_oracle_eval: every polynomial of the batch at the extension points [k][2] -> [k][ncols][2], canonical"""
        pts = _np_u64(points).reshape(-1, 2)
        out = np.zeros((pts.shape[0], self.ncols, 2), dtype=np.uint64)
        self.ctx._check(self.ctx.lib.lcp2_oracle_eval(self.handle, _ptr(pts), pts.shape[0], _ptr(out)))
        return out

    def read(self, coeffs=True, lde=True):
        n = 1 << self.log_n
        c = np.zeros((self.ncols, n), dtype=np.uint64) if coeffs else None
        l = np.zeros((self.ncols, n * self.block_count), dtype=np.uint64) if lde else None
        self.ctx._check(self.ctx.lib.lcp2_oracle_read(self.handle, _ptr(c), _ptr(l)))
        return c, l

    def close(self):
        if self.handle:
            self.ctx.lib.lcp2_oracle_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One prover context = one GPU + one HIP stream (lcp2_ctx).  stream: a raw hipStream_t, or None / 0 for a private
    non-blocking stream - torch.cuda.current_stream().cuda_stream is 0 for the default stream, so work queued there (a fill, an
    upload) is NOT ordered before the library's kernels: torch.cuda.synchronize() first, ctx.sync() before reading results - or
    pass order_with_default_stream=True (LCP2_CTX_ORDER_WITH_DEFAULT_STREAM): the private stream is then an ordinary blocking
    stream, which the runtime orders against stream 0 in both directions."""

    def __init__(self, device=0, stream=None, order_with_default_stream=False):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.lcp2_ctx_create_ex(device, stream, 1 if order_with_default_stream else 0, ctypes.byref(h))
        if rc:
            raise Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode())
        self.handle = h

    def _check(self, rc):
        if rc:
            msg = self.lib.lcp2_status_str(rc).decode()
            detail = self.lib.lcp2_last_error(self.handle)
            raise Lcp2Error(rc, msg + (": " + detail.decode() if detail else ""))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lcp2_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.lib.lcp2_ctx_sync(self.handle))

    def stream_ptr(self):
        """the hipStream_t the context runs on (an integer; torch.cuda.ExternalStream(ptr) wraps it)"""
        return self.lib.lcp2_ctx_stream(self.handle) or 0

    # ---- primitives on host numpy arrays
    def poseidon_permute_batch(self, states):
        s = _np_u64(states).reshape(-1, 12)
        out = np.empty_like(s)
        self._check(self.lib.lcp2_poseidon_permute_batch(self.handle, _ptr(s), _ptr(out), s.shape[0], MEM_HOST))
        return out

    FIELD_OPS = {"mul": 0, "pow7": 1, "add": 2, "sub": 3, "canon": 4, "add_lazy": 5, "sub_lazy": 6, "shl32_lazy": 24, "mul_u32": 25,
                 **{"shl%d" % (12 * k): 16 + k for k in range(1, 8)}}

    def field_op_batch(self, op, a, b=None):
        """elementwise field arithmetic with the device functions of csrc/gl64.hpp (LCP2_FIELD_*); operands any u64, results canonical"""
        a = _np_u64(a).reshape(-1)
        out = np.empty_like(a)
        if b is not None:
            b = _np_u64(b).reshape(-1)
            assert a.shape == b.shape
        self._check(self.lib.lcp2_field_op_batch(self.handle, _ptr(a), _ptr(b) if b is not None else None, _ptr(out), a.shape[0],
                                                 self.FIELD_OPS[op], MEM_HOST))
        return out

    def merkle_cap(self, leaves, cap_height):
        l = _np_u64(leaves)
        assert l.ndim == 2
        cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
        self._check(self.lib.lcp2_merkle_cap(self.handle, _ptr(l), l.shape[0], l.shape[1], cap_height, MEM_HOST, _ptr(cap)))
        return cap

    def ntt_batch(self, cols, inverse=False, shift=1):
        c = _np_u64(cols).copy()
        assert c.ndim == 2
        log_n = int(c.shape[1]).bit_length() - 1
        assert 1 << log_n == c.shape[1]
        self._check(self.lib.lcp2_ntt_batch(self.handle, _ptr(c), c.shape[0], log_n, int(inverse), shift, MEM_HOST))
        return c

    def lde_batch(self, coeffs, rate_bits=3):
        c = _np_u64(coeffs)
        log_n = int(c.shape[1]).bit_length() - 1
        out = np.zeros((c.shape[0], c.shape[1] << rate_bits), dtype=np.uint64)
        self._check(self.lib.lcp2_lde_batch(self.handle, _ptr(c), _ptr(out), c.shape[0], log_n, rate_bits, MEM_HOST))
        return out

    def sha256_tree(self, leaves, height, trees=1, trace=False):
        l = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(trees, 1 << height, 32)
        nodes = np.zeros((trees, (2 << height) - 1, 32), dtype=np.uint8)
        tr = np.zeros((trees, (1 << height) - 1, 2, 176), dtype=np.uint32) if trace else None
        self._check(self.lib.lcp2_sha256_tree(self.handle, _ptr(l), height, trees, _ptr(nodes), _ptr(tr), MEM_HOST))
        return (nodes, tr) if trace else nodes

    def _commit(self, fn, cols, rate_bits, cap_height, mem, shape):
        if mem == MEM_HOST:
            c = _np_u64(cols)
            ncols, n = c.shape
            p = _ptr(c)
        else:
            ncols, n = shape
            p = ctypes.c_void_p(cols)
        log_n = int(n).bit_length() - 1
        cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
        h = ctypes.c_void_p()
        self._check(fn(self.handle, p, ncols, log_n, rate_bits, cap_height, mem, ctypes.byref(h), _ptr(cap)))
        return Oracle(self, h, ncols, log_n, rate_bits, cap_height, cap)

    def commit_values(self, cols, rate_bits=3, cap_height=4, mem=MEM_HOST, shape=None):
        """PolynomialBatch::from_values.  cols: numpy [ncols][n] or a device pointer with shape=(ncols, n)."""
        return self._commit(self.lib.lcp2_commit_values, cols, rate_bits, cap_height, mem, shape)

    def commit_coeffs(self, cols, rate_bits=3, cap_height=4, mem=MEM_HOST, shape=None):
        return self._commit(self.lib.lcp2_commit_coeffs, cols, rate_bits, cap_height, mem, shape)

    def commit_cosets(self, coeffs, block_first, block_count, rate_bits=3, cap_height=4, mem=MEM_HOST, shape=None):
        """One rank's share of a coset-sharded commitment: coefficients of all columns in, its leaf blocks + cap part out."""
        if mem == MEM_HOST:
            c = _np_u64(coeffs)
            ncols, n = c.shape
            p = _ptr(c)
        else:
            ncols, n = shape
            p = ctypes.c_void_p(coeffs)
        log_n = int(n).bit_length() - 1
        cap = np.zeros((block_count << (cap_height - rate_bits), 4), dtype=np.uint64)
        h = ctypes.c_void_p()
        self._check(self.lib.lcp2_commit_cosets(self.handle, p, ncols, log_n, rate_bits, cap_height, block_first, block_count, mem,
                                                ctypes.byref(h), _ptr(cap)))
        o = Oracle(self, h, ncols, log_n, rate_bits, cap_height, cap)
        o.block_first, o.block_count = block_first, block_count
        return o

    def fri_prove_openings(self, oracles, inst, points, cfg, challenger_state):
        """lcp2_fri_prove_openings (PolynomialBatch::prove_openings for a bare FriInstanceInfo): the proof - the openings, then a
        FriProof; challenger_state is updated to the state after the query indices"""
        handles = (ctypes.c_void_p * len(oracles))(*[o.handle for o in oracles])
        cols = np.array([o.ncols for o in oracles], dtype=np.uint32)
        words = self.lib.lcp2_fri_openings_words(ctypes.byref(cfg), oracles[0].log_n if oracles else 0, _ptr(cols), ctypes.byref(inst))
        proof = np.zeros(max(words, 1), dtype=np.uint64)
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).ravel())
        self._check(self.lib.lcp2_fri_prove_openings(self.handle, handles, ctypes.byref(inst), _ptr(pts), ctypes.byref(cfg),
                                                     ctypes.byref(challenger_state), _ptr(proof), words))
        return proof[:words]

    def stark_prove(self, desc, trace, public_inputs, challenger_state, mem=MEM_HOST, perm=None):
        """lcp2_stark_prove (with perm, a StarkPerm of stark.pack_stark_perm: lcp2_stark_prove_perm): the proof of the AIR `desc`
        (stark.pack_stark_desc) for trace [width][n] - a numpy array, or a device pointer with mem=MEM_DEVICE; challenger_state is
        updated as the opening layer leaves it.  A violated constraint raises Lcp2Error with status -5 and the StarkViolation in its
        `violation` attribute."""
        words = stark_proof_words(desc, perm)
        proof = np.zeros(max(words, 1), dtype=np.uint64)
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if mem == MEM_HOST:
            trace = _np_u64(trace)
            tp = _ptr(trace)
        else:
            tp = ctypes.c_void_p(trace)
        violation = StarkViolation()
        if perm is None:
            rc = self.lib.lcp2_stark_prove(self.handle, ctypes.byref(desc), tp, mem, _ptr(pis), ctypes.byref(challenger_state), _ptr(proof), words,
                                           ctypes.byref(violation))
        else:
            rc = self.lib.lcp2_stark_prove_perm(self.handle, ctypes.byref(desc), ctypes.byref(perm), tp, mem, _ptr(pis), ctypes.byref(challenger_state),
                                                _ptr(proof), words, ctypes.byref(violation))
        if rc == -5:
            detail = self.lib.lcp2_last_error(self.handle)
            e = Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode() + (": " + detail.decode() if detail else ""))
            e.violation = violation
            raise e
        self._check(rc)
        return proof[:words]

    # ---- device buffers
    def buffer_zero(self, dev_ptr, words):
        self._check(self.lib.lcp2_buffer_zero(self.handle, ctypes.c_void_p(dev_ptr), int(words) * 8))

    def sha256_witness(self, jobs, level_start, words_in, wires_dev, n, digests=True):
        """lcp2_sha256_witness: fills columns 0..107 of the 310 rows of every two_to_one_sha256 of `jobs` (a numpy array of
        SHA_JOB_DTYPE records: first row, 16 sources; validated before anything runs) in the device witness matrix `wires_dev` (a
        pointer, [>= 108][n] column-major; n need not be a power of two).  level_start: nlevels + 1 job indices, jobs of a level
        read words_in (source s >= 0) or digest word (~s) & 7 of job (~s) >> 3 of any earlier level; a level may be empty.
        Returns the digests [njobs][8] (u32), or None with digests=False (the library then copies nothing back)."""
        if not isinstance(jobs, np.ndarray) or jobs.dtype != SHA_JOB_DTYPE:
            raise Lcp2Error(-1, "jobs must be an array of SHA_JOB_DTYPE records")
        j = np.ascontiguousarray(jobs).ravel()
        levels = np.ascontiguousarray(level_start, dtype=np.uint32).ravel()
        words = np.ascontiguousarray(words_in, dtype=np.uint32).ravel()
        out = np.zeros((j.size, 8), dtype=np.uint32) if digests else None
        self._check(self.lib.lcp2_sha256_witness(self.handle, _ptr(j) if j.size else None, j.size, _ptr(levels) if levels.size else None,
                                                 max(levels.size, 1) - 1, _ptr(words) if words.size else None, words.size,
                                                 ctypes.c_void_p(wires_dev), int(n), _ptr(out) if digests and j.size else None))
        return out

    def scatter_cells(self, cells, wires_dev, n):
        """lcp2_scatter_cells: wires[col][row] = value for every record of `cells` (a numpy array of CELL_DTYPE records) in the device
        witness matrix `wires_dev` (a pointer, column-major with n rows).  Rows are validated before anything runs; the COLUMN is
        the caller's duty (the call does not know how many the matrix has); values are stored as given, canonical or not."""
        if not isinstance(cells, np.ndarray) or cells.dtype != CELL_DTYPE:
            raise Lcp2Error(-1, "cells must be an array of CELL_DTYPE records")
        c = np.ascontiguousarray(cells).ravel()
        self._check(self.lib.lcp2_scatter_cells(self.handle, _ptr(c) if c.size else None, c.size, ctypes.c_void_p(wires_dev), int(n)))

    def poseidon_gate_rows(self, rows, wires_dev, n):
        """lcp2_poseidon_gate_rows: writes all 135 cells of every PoseidonGate row of `rows` (a numpy array of POSEIDON_ROW_DTYPE
        records: row, swap flag, 12 inputs; validated before anything runs) into the device witness matrix `wires_dev` (a
        pointer, [>= 135][n] column-major)."""
        if not isinstance(rows, np.ndarray) or rows.dtype != POSEIDON_ROW_DTYPE:
            raise Lcp2Error(-1, "rows must be an array of POSEIDON_ROW_DTYPE records")
        r = np.ascontiguousarray(rows).ravel()
        self._check(self.lib.lcp2_poseidon_gate_rows(self.handle, _ptr(r), r.size, ctypes.c_void_p(wires_dev), n))

    def u32_gate_rows(self, jobs, wires_dev, n, njobs=None):
        """lcp2_u32_gate_rows: writes the cells of every job into the device witness matrix `wires_dev` (a pointer, [>= 126][n]
        column-major).  jobs: a numpy array of U32_JOB_DTYPE records (a host list: validated before anything runs), or a device
        pointer to `njobs` lcp2_u32_job records (validated by the kernel).  Sorted by (kind, op, row) is the fast order
        (u32_gates.witness_jobs returns it); any order is correct."""
        if isinstance(jobs, np.ndarray):
            if jobs.dtype != U32_JOB_DTYPE:
                raise Lcp2Error(-1, "jobs must be an array of U32_JOB_DTYPE records")
            j = np.ascontiguousarray(jobs).ravel()
            count, p, mem = j.size, _ptr(j), MEM_HOST
        else:
            if njobs is None:
                raise Lcp2Error(-1, "a device job list needs njobs")
            count, p, mem = int(njobs), ctypes.c_void_p(jobs), MEM_DEVICE
        self._check(self.lib.lcp2_u32_gate_rows(self.handle, p, count, mem, ctypes.c_void_p(wires_dev), n))

    def rec_gate_rows(self, jobs, operands, level_ends, wires_dev, ncols, n, njobs=None, noperands=None):
        """lcp2_rec_gate_rows: runs the recorded plan level by level on the device witness matrix `wires_dev` (a pointer,
        [ncols >= 135][n] column-major).  jobs / operands: numpy arrays of REC_JOB_DTYPE / REC_OPERAND_DTYPE records (host lists:
        validated before anything runs), or two device pointers with `njobs` and `noperands` (validated by the kernel).
        level_ends: the index after the last job of every level, always on the host.  recursion_gates.witness_jobs and
        chain_plan return such lists in the fast order (kind, op, row) inside each level."""
        ends = np.ascontiguousarray(level_ends, dtype=np.uint32).ravel()
        if isinstance(jobs, np.ndarray) != isinstance(operands, np.ndarray):
            raise Lcp2Error(-1, "jobs and operands must both be host arrays or both be device pointers")
        if isinstance(jobs, np.ndarray):
            if jobs.dtype != REC_JOB_DTYPE or operands.dtype != REC_OPERAND_DTYPE:
                raise Lcp2Error(-1, "jobs / operands must be arrays of REC_JOB_DTYPE / REC_OPERAND_DTYPE records")
            j, o = np.ascontiguousarray(jobs).ravel(), np.ascontiguousarray(operands).ravel()
            nj, no, pj, po, mem = j.size, o.size, _ptr(j), _ptr(o), MEM_HOST
        else:
            if njobs is None or noperands is None:
                raise Lcp2Error(-1, "device lists need njobs and noperands")
            nj, no, pj, po, mem = int(njobs), int(noperands), ctypes.c_void_p(jobs), ctypes.c_void_p(operands), MEM_DEVICE
        self._check(self.lib.lcp2_rec_gate_rows(self.handle, pj, nj, po, no, _ptr(ends) if ends.size else None, ends.size, mem,
                                                ctypes.c_void_p(wires_dev), int(ncols), int(n)))

    def witness_plan_rows(self, rec_jobs, pos_jobs, chain_ends, operands, rec_level_ends, pos_level_ends, wires_dev, ncols, n,
                          nrec=None, npos=None, nchains=None, noperands=None):
        """lcp2_witness_plan_rows: runs a recorded plan of rec jobs and PoseidonGate chains level by level on the device witness
        matrix `wires_dev` (a pointer, [ncols >= 135][n] column-major).  rec_jobs / pos_jobs / chain_ends / operands: numpy arrays
        of REC_JOB_DTYPE / POS_JOB_DTYPE / uint32 / REC_OPERAND_DTYPE (host lists: validated before anything runs), or four device
        pointers with nrec, npos, nchains and noperands (validated by the kernels).  rec_level_ends / pos_level_ends: the index
        after the last rec job / the last CHAIN of every level, always on the host and equally long.
        recursion_gates.pack_witness_plan returns all six."""
        rends = np.ascontiguousarray(rec_level_ends, dtype=np.uint32).ravel()
        pends = np.ascontiguousarray(pos_level_ends, dtype=np.uint32).ravel()
        if rends.size != pends.size:
            raise Lcp2Error(-1, "rec_level_ends and pos_level_ends must have one entry per level each")
        lists = (rec_jobs, pos_jobs, chain_ends, operands)
        on_host = [isinstance(a, np.ndarray) for a in lists]
        if any(on_host) != all(on_host):
            raise Lcp2Error(-1, "the four lists must all be host arrays or all be device pointers")
        if all(on_host):
            if (rec_jobs.dtype, pos_jobs.dtype, chain_ends.dtype, operands.dtype) != (REC_JOB_DTYPE, POS_JOB_DTYPE, np.dtype(np.uint32), REC_OPERAND_DTYPE):
                raise Lcp2Error(-1, "the lists must be arrays of REC_JOB_DTYPE / POS_JOB_DTYPE / uint32 / REC_OPERAND_DTYPE records")
            keep = [np.ascontiguousarray(a).ravel() for a in lists]
            counts, ptrs, mem = [a.size for a in keep], [a.ctypes.data if a.size else None for a in keep], MEM_HOST
        else:
            if None in (nrec, npos, nchains, noperands):
                raise Lcp2Error(-1, "device lists need nrec, npos, nchains and noperands")
            counts, ptrs, mem = [int(nrec), int(npos), int(nchains), int(noperands)], [a or None for a in lists], MEM_DEVICE
        plan = WitnessPlan(ptrs[0], counts[0], rends.ctypes.data if rends.size else None, ptrs[1], counts[1], ptrs[2], counts[2],
                           pends.ctypes.data if pends.size else None, ptrs[3], counts[3], rends.size)
        self._check(self.lib.lcp2_witness_plan_rows(self.handle, ctypes.byref(plan), mem, ctypes.c_void_p(wires_dev), int(ncols), int(n)))

    def witness_plan_rows_u32(self, u32_jobs, rec_jobs, pos_jobs, chain_ends, operands, u32_level_ends, rec_level_ends, pos_level_ends,
                              wires_dev, ncols, n, nu32=None, nrec=None, npos=None, nchains=None, noperands=None):
        """lcp2_witness_plan_rows_u32: witness_plan_rows for a plan that also holds plonky2_u32 / comparison jobs, whose inputs are
        operands of the plan (IMM or CELL).  u32_jobs: U32_PLAN_JOB_DTYPE records, with the other four lists either all numpy arrays
        (host lists: validated before anything runs) or all device pointers with nu32, nrec, npos, nchains and noperands.  The three
        level tables are always on the host and equally long.  u32_gates.pack_u32_plan returns all eight."""
        ends = [np.ascontiguousarray(e, dtype=np.uint32).ravel() for e in (u32_level_ends, rec_level_ends, pos_level_ends)]
        if len({e.size for e in ends}) != 1:
            raise Lcp2Error(-1, "u32_level_ends, rec_level_ends and pos_level_ends must have one entry per level each")
        lists = (u32_jobs, rec_jobs, pos_jobs, chain_ends, operands)
        on_host = [isinstance(a, np.ndarray) for a in lists]
        if any(on_host) != all(on_host):
            raise Lcp2Error(-1, "the five lists must all be host arrays or all be device pointers")
        if all(on_host):
            if [a.dtype for a in lists] != [U32_PLAN_JOB_DTYPE, REC_JOB_DTYPE, POS_JOB_DTYPE, np.dtype(np.uint32), REC_OPERAND_DTYPE]:
                raise Lcp2Error(-1, "the lists must be arrays of U32_PLAN_JOB_DTYPE / REC_JOB_DTYPE / POS_JOB_DTYPE / uint32 / REC_OPERAND_DTYPE records")
            keep = [np.ascontiguousarray(a).ravel() for a in lists]
            counts, ptrs, mem = [a.size for a in keep], [a.ctypes.data if a.size else None for a in keep], MEM_HOST
        else:
            if None in (nu32, nrec, npos, nchains, noperands):
                raise Lcp2Error(-1, "device lists need nu32, nrec, npos, nchains and noperands")
            counts, ptrs, mem = [int(nu32), int(nrec), int(npos), int(nchains), int(noperands)], [a or None for a in lists], MEM_DEVICE
        end_ptrs = [e.ctypes.data if e.size else None for e in ends]
        base = WitnessPlan(ptrs[1], counts[1], end_ptrs[1], ptrs[2], counts[2], ptrs[3], counts[3], end_ptrs[2], ptrs[4], counts[4], ends[0].size)
        plan = WitnessPlanU32(base, ptrs[0], counts[0], end_ptrs[0])
        self._check(self.lib.lcp2_witness_plan_rows_u32(self.handle, ctypes.byref(plan), mem, ctypes.c_void_p(wires_dev), int(ncols), int(n)))

    def witness_plan_rows_sha(self, sha_jobs, u32_jobs, rec_jobs, pos_jobs, chain_ends, operands, sha_level_ends, u32_level_ends, rec_level_ends,
                              pos_level_ends, wires_dev, ncols, n, nsha=None, nu32=None, nrec=None, npos=None, nchains=None, noperands=None):
        """lcp2_witness_plan_rows_sha: witness_plan_rows_u32 for a plan that also holds SHA-256 jobs (310 rows each, columns 0..107),
        whose 16 message words are operands of the plan (IMM or CELL); digests are read from the matrix (sha_plan.digest_cell).
        sha_jobs: SHA_PLAN_JOB_DTYPE records, with the other five lists either all numpy arrays (host lists: validated before
        anything runs) or all device pointers with nsha, nu32, nrec, npos, nchains and noperands.  The four level tables are always
        on the host and equally long.  sha_plan.pack_sha_plan returns all ten."""
        ends = [np.ascontiguousarray(e, dtype=np.uint32).ravel() for e in (sha_level_ends, u32_level_ends, rec_level_ends, pos_level_ends)]
        if len({e.size for e in ends}) != 1:
            raise Lcp2Error(-1, "sha_level_ends, u32_level_ends, rec_level_ends and pos_level_ends must have one entry per level each")
        lists = (sha_jobs, u32_jobs, rec_jobs, pos_jobs, chain_ends, operands)
        on_host = [isinstance(a, np.ndarray) for a in lists]
        if any(on_host) != all(on_host):
            raise Lcp2Error(-1, "the six lists must all be host arrays or all be device pointers")
        if all(on_host):
            if [a.dtype for a in lists] != [SHA_PLAN_JOB_DTYPE, U32_PLAN_JOB_DTYPE, REC_JOB_DTYPE, POS_JOB_DTYPE, np.dtype(np.uint32), REC_OPERAND_DTYPE]:
                raise Lcp2Error(-1, "the lists must be arrays of SHA_PLAN_JOB_DTYPE / U32_PLAN_JOB_DTYPE / REC_JOB_DTYPE / POS_JOB_DTYPE / uint32 / "
                                    "REC_OPERAND_DTYPE records")
            keep = [np.ascontiguousarray(a).ravel() for a in lists]
            counts, ptrs, mem = [a.size for a in keep], [a.ctypes.data if a.size else None for a in keep], MEM_HOST
        else:
            if None in (nsha, nu32, nrec, npos, nchains, noperands):
                raise Lcp2Error(-1, "device lists need nsha, nu32, nrec, npos, nchains and noperands")
            counts, ptrs, mem = [int(nsha), int(nu32), int(nrec), int(npos), int(nchains), int(noperands)], [a or None for a in lists], MEM_DEVICE
        end_ptrs = [e.ctypes.data if e.size else None for e in ends]
        base = WitnessPlan(ptrs[2], counts[2], end_ptrs[2], ptrs[3], counts[3], ptrs[4], counts[4], end_ptrs[3], ptrs[5], counts[5], ends[0].size)
        plan = WitnessPlanSha(WitnessPlanU32(base, ptrs[1], counts[1], end_ptrs[1]), ptrs[0], counts[0], end_ptrs[0])
        self._check(self.lib.lcp2_witness_plan_rows_sha(self.handle, ctypes.byref(plan), mem, ctypes.c_void_p(wires_dev), int(ncols), int(n)))

    def verify_batch(self, circuit_data, proofs, public_inputs, mem=MEM_HOST, count=None, head="host"):
        """lcp2_verify_batch: data.verify for a batch of proofs of one circuit (any CircuitData, verifier-only ones included), Merkle
        paths and FRI queries on this context's device.  proofs: a (count, proof_words) array, or with mem=MEM_DEVICE a device pointer
        and `count`; public_inputs: (count, num_public_inputs), host.  head: "host" (transcript and vanishing identity on the host, one
        proof at a time) or "device" (lcp2_verify_batch_ex with LCP2_VERIFY_HEAD_DEVICE: on the device as well; the same verdicts).
        Returns the int32 array of failed checks (0 = accepted, 1..7 as ProofRejected.check); does not raise on rejection."""
        if head not in VERIFY_HEADS:
            raise Lcp2Error(-1, "head is 'host' or 'device'")
        words = circuit_data.proof_words
        if mem == MEM_HOST:
            pr = _np_u64(proofs)
            if pr.size % words:
                raise Lcp2Error(-1, "proofs is not a whole number of this circuit's proofs")
            count, ptr = pr.size // words, _ptr(pr)
        else:
            if count is None:
                raise Lcp2Error(-1, "device proofs need count")
            ptr = ctypes.c_void_p(proofs)
        if count == 0:
            return np.zeros(0, dtype=np.int32)
        pis = _np_u64(public_inputs).ravel()
        npi = pis.size // count
        if npi * count != pis.size:
            raise Lcp2Error(-1, "public_inputs is not count rows")
        checks = np.zeros(count, dtype=np.int32)
        if head == "host":
            rc = self.lib.lcp2_verify_batch(self.handle, circuit_data.handle, ptr, words, count, mem, _ptr(pis), npi, _ptr(checks))
        else:
            rc = self.lib.lcp2_verify_batch_ex(self.handle, circuit_data.handle, ptr, words, count, mem, _ptr(pis), npi, _ptr(checks), VERIFY_HEADS[head])
        if rc != -7:
            self._check(rc)
        return checks

    def expand_rows(self, circ, rows, bindings_ptr=None, num_bindings=None):
        """lcp2_circuit_rows_expand: the matrix [num_constants + num_routed_wires][n] that `rows` (circuit.Rows) describe for the
        parameters, gate set and coset shifts of `circ` - what circ.constants_sigmas would hold.  bindings_ptr / num_bindings: a device
        list of lcp2_copy_binding records instead of rows.bindings."""
        d, keep = _describe(circ, 0)
        r, keep_rows = _describe_rows(rows, bindings_ptr, num_bindings)
        shape = (circ.params.num_constants + circ.params.num_routed_wires, 1 << circ.params.degree_bits)
        ptr = self.buffer_alloc(shape[0] * shape[1])
        try:
            self._check(self.lib.lcp2_circuit_rows_expand(self.handle, ctypes.byref(d), ctypes.byref(r), ctypes.c_void_p(ptr)))
            return self.buffer_read(ptr, shape[0] * shape[1]).reshape(shape)
        finally:
            self.buffer_free(ptr)

    def buffer_alloc(self, words):
        p = ctypes.c_void_p()
        self._check(self.lib.lcp2_buffer_alloc(self.handle, int(words) * 8, ctypes.byref(p)))
        return p.value

    def buffer_free(self, dev_ptr):
        self._check(self.lib.lcp2_buffer_free(self.handle, ctypes.c_void_p(dev_ptr)))

    def buffer_read(self, dev_ptr, words):
        out = np.zeros(words, dtype=np.uint64)
        self._check(self.lib.lcp2_buffer_read(self.handle, _ptr(out), ctypes.c_void_p(dev_ptr), words * 8))
        return out

    def buffer_write(self, dev_ptr, arr):
        a = _np_u64(arr)
        self._check(self.lib.lcp2_buffer_write(self.handle, ctypes.c_void_p(dev_ptr), _ptr(a), a.size * 8))

    def buffer_copy(self, dst_ptr, src_ptr, words):
        self._check(self.lib.lcp2_buffer_copy(self.handle, ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), words * 8))

    def buffer_copy_2d(self, dst_ptr, dst_pitch_words, src_ptr, src_pitch_words, width_words, height):
        """`height` runs of `width_words`, the pitches apart (device to device)"""
        self._check(self.lib.lcp2_buffer_copy_2d(self.handle, ctypes.c_void_p(dst_ptr), dst_pitch_words * 8, ctypes.c_void_p(src_ptr),
                                                 src_pitch_words * 8, width_words * 8, height))

    # ---- timing
    def prof_enable(self, on=True):
        self._check(self.lib.lcp2_prof_enable(self.handle, int(on)))

    def prof_reset(self):
        self._check(self.lib.lcp2_prof_reset(self.handle))

    def prof_get(self):
        out = {}
        for i, name in enumerate(KERNEL_FAMILIES):
            ms, n, b = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_double()
            self._check(self.lib.lcp2_prof_get(self.handle, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(b)))
            out[name] = {"ms": ms.value, "launches": n.value, "bytes": b.value}
        return out


class Challenger:
    """plonky2's Challenger<F, PoseidonHash> on the host (lcp2_challenger_*): the transcript of a caller that drives the
    seams of data.prove() itself (staged or sharded proving)."""

    def __init__(self):
        self.lib = load_library()
        self.state = ChallengerState()
        self.lib.lcp2_challenger_init(ctypes.byref(self.state))

    def observe(self, values):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).ravel())
        rc = self.lib.lcp2_challenger_observe(ctypes.byref(self.state), _ptr(v), v.size)
        if rc:
            raise Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode())

    def get(self, count=1):
        out = np.zeros(count, dtype=np.uint64)
        rc = self.lib.lcp2_challenger_get(ctypes.byref(self.state), _ptr(out), count)
        if rc:
            raise Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode())
        return out


def hash_no_pad(values):
    """PoseidonHash::hash_no_pad on the host (public-input hash of the transcript)"""
    lib = load_library()
    v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).ravel())
    out = np.zeros(4, dtype=np.uint64)
    rc = lib.lcp2_hash_no_pad(_ptr(v) if v.size else None, v.size, _ptr(out))
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    return out


SER_PUBLIC_INPUT_COUNT = 1


def proof_layout(params):
    """where each field of plonky2's Proof / FriProof sits in the flat proof array (lcp2_proof_layout_of)"""
    lib, out = load_library(), ProofLayout()
    rc = lib.lcp2_proof_layout_of(ctypes.byref(params), ctypes.byref(out))
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    return out


def proof_to_bytes(params, proof, public_inputs, flags=SER_PUBLIC_INPUT_COUNT):
    """ProofWithPublicInputs::to_bytes (plonky2 util/serialization.rs layout, see include/lcp2.h; parity unpinned)"""
    lib = load_library()
    pr, pis = _np_u64(proof).ravel(), _np_u64(public_inputs).ravel()
    out = np.zeros(lib.lcp2_proof_bytes(ctypes.byref(params), pis.size, flags), dtype=np.uint8)
    rc = lib.lcp2_proof_to_bytes(ctypes.byref(params), _ptr(pr), pr.size, _ptr(pis), pis.size, flags, _ptr(out), out.size)
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    return out.tobytes()


def proof_from_bytes(params, data, num_public_inputs, flags=SER_PUBLIC_INPUT_COUNT):
    """-> (proof words, public inputs); Lcp2Error on a malformed buffer"""
    lib = load_library()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    proof = np.zeros(lib.lcp2_proof_words(ctypes.byref(params)), dtype=np.uint64)
    pis = np.zeros(num_public_inputs, dtype=np.uint64)
    rc = lib.lcp2_proof_from_bytes(ctypes.byref(params), _ptr(buf) if buf.size else None, buf.size, flags, _ptr(proof), proof.size, _ptr(pis), pis.size)
    if rc:
        raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
    return proof, pis


class ProofRejected(Lcp2Error):
    """data.verify(proof) failed; .check names the failed step (see lcp2_verify)."""

    def __init__(self, check):
        super().__init__(-7, f"proof rejected (check {check})")
        self.check = check


def _describe(circ, constants_sigmas_ptr=None, mem=MEM_HOST):
    """lcp2_circuit_desc for a circuit.Circuit; returns (desc, keepalive)"""
    gs = circ.gateset
    gates = circ.gates_array
    d = CircuitDesc()
    d.params = circ.params
    d.constants_sigmas = constants_sigmas_ptr if constants_sigmas_ptr is not None else circ.constants_sigmas.ctypes.data
    d.constants_sigmas_mem = mem
    d.k_is = circ.k_is.ctypes.data
    d.num_selectors, d.num_gates = gs.num_selectors, len(gs.gates)
    d.gates = ctypes.cast(gates, ctypes.c_void_p)
    d.code, d.code_words = gs.code.ctypes.data, gs.code_len
    d.imm, d.num_imm = gs.imm.ctypes.data, gs.imm.size
    d.num_public_inputs, d.num_regs = circ.num_public_inputs, gs.max_regs
    return d, (gates, gs, circ)


def _describe_rows(rows, bindings_ptr=None, num_bindings=None):
    """lcp2_circuit_rows for a circuit.Rows; a device binding list as (pointer, count) instead of rows.bindings.  Returns (struct, keepalive)"""
    gate_of_row = np.ascontiguousarray(rows.gate_of_row, dtype=np.uint32).ravel()
    consts = None if rows.row_constants is None else np.ascontiguousarray(rows.row_constants, dtype=np.uint64)
    r = CircuitRows()
    r.gate_of_row, r.num_rows, r.pad_gate = (gate_of_row.ctypes.data if gate_of_row.size else None), gate_of_row.size, rows.pad_gate
    r.row_constants = consts.ctypes.data if consts is not None and consts.size else None
    r.num_classes = rows.num_classes
    if bindings_ptr is not None:
        r.bindings, r.num_bindings, r.bindings_mem, b = bindings_ptr, int(num_bindings), MEM_DEVICE, None
    else:
        if not isinstance(rows.bindings, np.ndarray) or rows.bindings.dtype != BINDING_DTYPE:
            raise Lcp2Error(-1, "bindings must be an array of BINDING_DTYPE records")
        b = np.ascontiguousarray(rows.bindings).ravel()
        r.bindings, r.num_bindings, r.bindings_mem = (b.ctypes.data if b.size else None), b.size, MEM_HOST
    return r, (gate_of_row, consts, b)


class CircuitData:
    """builder.build::<C>() result: the handle `prove` and `verify` are called on
    (reference: eth-lc-plonky2/src/main.rs:227-233)."""

    def __init__(self, ctx, circ, handle, keep):
        self.ctx, self.circ, self.handle, self._keep = ctx, circ, handle, keep
        self.lib = load_library()
        self.proof_words = self.lib.lcp2_proof_words(ctypes.byref(circ.params))

    @classmethod
    def build(cls, ctx, circ, constants_sigmas_ptr=None, mem=MEM_HOST):
        d, keep = _describe(circ, constants_sigmas_ptr, mem)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.lcp2_circuit_create(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        return cls(ctx, circ, h, keep)

    @classmethod
    def build_from_rows(cls, ctx, circ, rows, bindings_ptr=None, num_bindings=None):
        """lcp2_circuit_create_from_rows: the handle of `circ` with its preprocessed columns built on the device from `rows`
        (circuit.Rows); circ.constants_sigmas is not looked at (the description goes in with a null matrix)."""
        d, keep = _describe(circ, 0)
        r, keep_rows = _describe_rows(rows, bindings_ptr, num_bindings)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.lcp2_circuit_create_from_rows(ctx.handle, ctypes.byref(d), ctypes.byref(r), ctypes.byref(h)))
        return cls(ctx, circ, h, keep)

    @classmethod
    def build_sharded(cls, ctx, circ, block_first, block_count, constants_sigmas_ptr=None, mem=MEM_HOST):
        """one rank's part of a coset-sharded circuit: holds the leaf blocks [block_first, block_first + block_count).
        The digest is valid after set_constants_cap(OR of every rank's digest()[1])."""
        d, keep = _describe(circ, constants_sigmas_ptr, mem)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.lcp2_circuit_create_sharded(ctx.handle, ctypes.byref(d), block_first, block_count, ctypes.byref(h)))
        return cls(ctx, circ, h, keep)

    def set_constants_cap(self, cap):
        cp = _np_u64(cap)
        self._check(self.lib.lcp2_circuit_set_constants_cap(self.handle, _ptr(cp)))

    def quotient_values(self, alphas, public_inputs_hash):
        a, h = _np_u64(alphas), _np_u64(public_inputs_hash)
        assert h.size == 4
        self._check(self.lib.lcp2_quotient_values(self.handle, _ptr(a), _ptr(h)))

    def quotient_buffer(self):
        """(device pointer, uint64 words) of the quotient values [num_challenges][8n]: the one bulk exchange of a sharded proof"""
        ptr, words = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.lcp2_quotient_buffer(self.handle, ctypes.byref(ptr), ctypes.byref(words)))
        return ptr.value, words.value

    def quotient_commit(self):
        cap = self._cap()
        self._check(self.lib.lcp2_quotient_commit(self.handle, _ptr(cap)))
        return cap

    @classmethod
    def verifier_only(cls, circ, digest, cap):
        lib = load_library()
        d, keep = _describe(circ, 0)
        h = ctypes.c_void_p()
        dg, cp = _np_u64(digest), _np_u64(cap)
        rc = lib.lcp2_verifier_create(ctypes.byref(d), _ptr(dg), _ptr(cp), ctypes.byref(h))
        if rc:
            raise Lcp2Error(rc, lib.lcp2_status_str(rc).decode())
        return cls(None, circ, h, keep)

    def _check(self, rc):
        if rc:
            if self.ctx is not None:
                self.ctx._check(rc)
            raise Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode())

    def digest(self):
        d = np.zeros(4, dtype=np.uint64)
        cap = np.zeros((1 << self.circ.params.cap_height, 4), dtype=np.uint64)
        self._check(self.lib.lcp2_circuit_digest(self.handle, _ptr(d), _ptr(cap)))
        return d, cap

    def prove(self, wires, public_inputs, mem=MEM_HOST):
        """data.prove(pw): wires = full witness [num_wires][n] (numpy, or a device pointer with mem=MEM_DEVICE)"""
        pis = _np_u64(public_inputs).ravel()
        proof = np.zeros(self.proof_words, dtype=np.uint64)
        if mem == MEM_HOST:
            w = _np_u64(wires)
            if w.shape != (self.circ.params.num_wires, 1 << self.circ.params.degree_bits):
                raise Lcp2Error(-1, "witness must be [num_wires][n]")
            wp = _ptr(w)
        else:
            wp = ctypes.c_void_p(wires)
        self._check(self.lib.lcp2_prove(self.handle, wp, mem, _ptr(pis), pis.size, _ptr(proof), proof.size))
        return proof

    def check_witness(self, wires, public_inputs, per_gate=False, mem=MEM_HOST):
        """lcp2_check_witness: where the witness violates gate and copy constraints, exactly (wires as for prove).  Returns a
        WitnessReport; per_gate=True also fills report.per_gate, the gate violations split by gate."""
        pis = _np_u64(public_inputs).ravel()
        if mem == MEM_HOST:
            w = _np_u64(wires)
            if w.shape != (self.circ.params.num_wires, 1 << self.circ.params.degree_bits):
                raise Lcp2Error(-1, "witness must be [num_wires][n]")
            wp = _ptr(w)
        else:
            wp = ctypes.c_void_p(wires)
        report = WitnessReport()
        ng = len(self.circ.gateset.gates)
        counts = np.zeros(ng, dtype=np.uint64) if per_gate else None
        self._check(self.lib.lcp2_check_witness(self.handle, wp, mem, _ptr(pis), pis.size, ctypes.byref(report), _ptr(counts), ng))
        report.per_gate = counts
        return report

    def fill_copies(self, cells, wires_ptr, mem=MEM_HOST, ncells=None):
        """lcp2_witness_fill_copies: every record of `cells` is written into the device matrix `wires_ptr` ([num_wires][n]), and the
        listed cell with the smallest list index of each copy class gives its value to every routed cell of the class.  cells: a numpy
        array of CELL_DTYPE records, or with mem=MEM_DEVICE a device pointer to `ncells` lcp2_cell records.  Returns the FillReport;
        conflicting values (LCP2_E_UNSAT) do not raise: report.unsat is set and report.message names the cells.  Every other status
        raises Lcp2Error."""
        return self._copies_call(self.lib.lcp2_witness_fill_copies, cells, CELL_DTYPE, "cells must be an array of CELL_DTYPE records", wires_ptr, mem, ncells)

    def settle_copies(self, sources, wires_ptr, mem=MEM_HOST, nsources=None):
        """lcp2_witness_settle_copies: the source with the smallest list index of each copy class gives the word the device matrix
        `wires_ptr` ([num_wires][n]) holds at its cell to every other routed cell of the class.  sources: a numpy array of
        CELL_REF_DTYPE records, or with mem=MEM_DEVICE a device pointer to `nsources` lcp2_cell_ref records.  Returns what
        fill_copies returns."""
        return self._copies_call(self.lib.lcp2_witness_settle_copies, sources, CELL_REF_DTYPE, "sources must be an array of CELL_REF_DTYPE records", wires_ptr, mem,
                                 nsources)

    def _copies_call(self, call, records, dtype, dtype_message, wires_ptr, mem, count):
        if mem == MEM_HOST:
            if not isinstance(records, np.ndarray) or records.dtype != dtype:
                raise Lcp2Error(-1, dtype_message)
            c = np.ascontiguousarray(records).ravel()
            p, count = (_ptr(c) if c.size else None), c.size
        else:
            p, count = ctypes.c_void_p(records), int(count)
        report = FillReport()
        rc = call(self.handle, p, count, mem, ctypes.c_void_p(wires_ptr), ctypes.byref(report))
        if rc == E_UNSAT:
            report.unsat = True
            report.message = self.lib.lcp2_last_error(self.ctx.handle).decode()
        else:
            self._check(rc)
        return report

    def copy_classes(self):
        """lcp2_circuit_copy_classes: (class_of [num_routed_wires][n] uint32 - 0xFFFFFFFF for a cell in no class -, num_classes)"""
        NR, n = self.circ.params.num_routed_wires, 1 << self.circ.params.degree_bits
        class_of, count = np.zeros((NR, n), dtype=np.uint32), ctypes.c_uint64()
        self._check(self.lib.lcp2_circuit_copy_classes(self.handle, _ptr(class_of), ctypes.byref(count)))
        return class_of, count.value

    # ---- host witnesses with the upload off the critical path (lcp2_witness_stage / lcp2_prove_staged)
    def stage_witness(self, wires, slot):
        """starts the upload of a host witness into staging slot 0 / 1; `wires` must stay alive and unchanged until prove_staged(slot) returned"""
        w = _np_u64(wires)
        if w.shape != (self.circ.params.num_wires, 1 << self.circ.params.degree_bits):
            raise Lcp2Error(-1, "witness must be [num_wires][n]")
        if not hasattr(self, "_staged"):
            self._staged = {}
        self._staged[slot] = w
        self._check(self.lib.lcp2_witness_stage(self.handle, _ptr(w), slot))

    def prove_staged(self, slot, public_inputs):
        pis = _np_u64(public_inputs).ravel()
        proof = np.zeros(self.proof_words, dtype=np.uint64)
        self._check(self.lib.lcp2_prove_staged(self.handle, slot, _ptr(pis), pis.size, _ptr(proof), proof.size))
        self._staged.pop(slot, None)
        return proof

    def host_witness_benchmark(self, wires, public_inputs, steps=4, reference_proof=None):
        """`steps` proofs from HOST witnesses (two pinned copies of `wires`, alternating): the plain way - lcp2_prove(MEM_HOST), the copy
        in front of every proof - and the staged way - the upload of witness i + 1 overlaps proof i.  Returns the per-proof times."""
        import time
        ctx = self.ctx
        bufs = [np.ascontiguousarray(wires, dtype=np.uint64), np.array(wires, dtype=np.uint64, order="C")]
        for b in bufs:
            ctx._check(ctx.lib.lcp2_host_register(ctx.handle, _ptr(b), b.nbytes))
        try:
            ctx.sync()
            t0 = time.perf_counter()
            plain = self.prove(bufs[0], public_inputs, mem=MEM_HOST)
            t_plain = time.perf_counter() - t0
            self.stage_witness(bufs[0], 0)
            times = []
            for i in range(steps):
                t0 = time.perf_counter()
                if i + 1 < steps:
                    self.stage_witness(bufs[(i + 1) % 2], (i + 1) % 2)
                proof = self.prove_staged(i % 2, public_inputs)
                times.append(time.perf_counter() - t0)
            ok = bool((proof == plain).all()) and (reference_proof is None or bool((proof == reference_proof).all()))
        finally:
            ctx.sync()
            for b in bufs:
                ctx.lib.lcp2_host_unregister(ctx.handle, _ptr(b))
        steady = times[1:-1] if len(times) > 2 else times  # the first proof waits for its own upload, the last one has nothing to overlap
        return {"workload": "lcp2_prove from HOST witnesses (%.2f GB each, pinned with lcp2_host_register): upload of witness i + 1 on the copy stream while "
                            "proof i runs (lcp2_witness_stage / lcp2_prove_staged)" % (bufs[0].nbytes / 1e9),
                "ms_per_proof_steady_state": 1e3 * min(steady), "ms_per_proof_all": [round(1e3 * t, 2) for t in times],
                "ms_plain_host_prove": 1e3 * t_plain, "proofs_equal_device_resident_proof": ok}

    # ---- the seams of data.prove() one by one (the caller runs the Fiat-Shamir transcript)
    def _cap(self):
        return np.zeros((1 << self.circ.params.cap_height, 4), dtype=np.uint64)

    def commit_wires(self, wires, mem=MEM_HOST):
        cap = self._cap()
        if mem == MEM_HOST:
            self._staged_wires = _np_u64(wires)  # stays alive until the proof is finished
            wp = _ptr(self._staged_wires)
        else:
            wp = ctypes.c_void_p(wires)
        self._check(self.lib.lcp2_commit_wires(self.handle, wp, mem, _ptr(cap)))
        return cap

    def commit_wires_coeffs(self, wires_ptr, coeffs_ptr):
        """commit_wires with the coefficients supplied (device pointers): the sharded proof's polynomial-parallel iNTT"""
        cap = self._cap()
        self._check(self.lib.lcp2_commit_wires_coeffs(self.handle, ctypes.c_void_p(wires_ptr), ctypes.c_void_p(coeffs_ptr), _ptr(cap)))
        return cap

    # row exchange form of a sharded proof (include/lcp2.h): the rank holds the witness values of its row block only
    def commit_wires_rows(self, rows_ptr, coeffs_ptr):
        cap = self._cap()
        self._check(self.lib.lcp2_commit_wires_rows(self.handle, ctypes.c_void_p(rows_ptr), ctypes.c_void_p(coeffs_ptr), _ptr(cap)))
        return cap

    def commit_wires_rows_begin(self, rows_ptr):
        self._check(self.lib.lcp2_commit_wires_rows_begin(self.handle, ctypes.c_void_p(rows_ptr)))

    def commit_wires_chunk(self, coeffs_ptr, first_col, ncols):
        self._check(self.lib.lcp2_commit_wires_chunk(self.handle, ctypes.c_void_p(coeffs_ptr), first_col, ncols))

    def commit_wires_rows_finish(self):
        cap = self._cap()
        self._check(self.lib.lcp2_commit_wires_rows_finish(self.handle, _ptr(cap)))
        return cap

    def perm_zs_rows_begin(self, betas, gammas, world):
        """this rank's share of the table [world][num_challenges] of row-block products"""
        out, b, g = np.zeros(world * self.circ.params.num_challenges, dtype=np.uint64), _np_u64(betas), _np_u64(gammas)
        self._check(self.lib.lcp2_perm_zs_rows_begin(self.handle, _ptr(b), _ptr(g), _ptr(out)))
        return out

    def perm_zs_rows_finish(self, block_products):
        """-> (device pointer, words) of the exchange buffer [world][columns][rows]; this rank's slot is filled"""
        bp = _np_u64(block_products)
        ptr, words = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.lcp2_perm_zs_rows_finish(self.handle, _ptr(bp), ctypes.byref(ptr), ctypes.byref(words)))
        return ptr.value, words.value

    def perm_zs_commit(self):
        cap = self._cap()
        self._check(self.lib.lcp2_perm_zs_commit(self.handle, _ptr(cap)))
        return cap

    def perm_zs(self, betas, gammas):
        cap, b, g = self._cap(), _np_u64(betas), _np_u64(gammas)
        self._check(self.lib.lcp2_perm_zs(self.handle, _ptr(b), _ptr(g), _ptr(cap)))
        return cap

    def quotient(self, alphas, public_inputs_hash):
        """compute_quotient_polys + commitment; takes public_inputs_hash (4 elements) as plonky2's function does"""
        cap, a, h = self._cap(), _np_u64(alphas), _np_u64(public_inputs_hash)
        assert h.size == 4
        self._check(self.lib.lcp2_quotient(self.handle, _ptr(a), _ptr(h), _ptr(cap)))
        return cap

    def fri_open(self, zeta, challenger_state, proof):
        """proof: uint64 array of proof_words; words from the openings on are written; challenger_state is updated"""
        z = _np_u64(zeta)
        assert proof.dtype == np.uint64 and proof.size == self.proof_words and proof.flags.c_contiguous
        self._check(self.lib.lcp2_fri_open(self.handle, _ptr(z), ctypes.byref(challenger_state), _ptr(proof)))

    # lcp2_fri_open in its three phases (the exchange points of a coset-sharded proof)
    def fri_open_begin(self, zeta, challenger_state, proof):
        z = _np_u64(zeta)
        assert proof.dtype == np.uint64 and proof.size == self.proof_words and proof.flags.c_contiguous
        self._check(self.lib.lcp2_fri_open_begin(self.handle, _ptr(z), ctypes.byref(challenger_state), _ptr(proof)))

    def fri_open_commit(self, proof):
        assert proof.dtype == np.uint64 and proof.size == self.proof_words and proof.flags.c_contiguous
        self._check(self.lib.lcp2_fri_open_commit(self.handle, _ptr(proof)))

    def fri_open_finish(self, proof, challenger_state=None):
        assert proof.dtype == np.uint64 and proof.size == self.proof_words and proof.flags.c_contiguous
        self._check(self.lib.lcp2_fri_open_finish(self.handle, ctypes.byref(challenger_state) if challenger_state is not None else None, _ptr(proof)))

    def proof_section(self, section):
        """(first word, word count) of SECTION_OPENINGS / SECTION_FRI_CAP0 / SECTION_AFTER_CAPS inside the proof array"""
        first, count = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(self.lib.lcp2_proof_section(self.handle, section, ctypes.byref(first), ctypes.byref(count)))
        return first.value, count.value

    def verify(self, proof, public_inputs):
        """data.verify(proof): raises ProofRejected like the reference's unwrap()"""
        failed = ctypes.c_int(0)
        pr, pis = _np_u64(proof).ravel(), _np_u64(public_inputs).ravel()
        # the lengths travel with the buffers: the library refuses a proof that is not exactly lcp2_proof_words() long
        rc = self.lib.lcp2_verify(self.handle, _ptr(pr), pr.size, _ptr(pis), pis.size, ctypes.byref(failed))
        if rc == -7:
            raise ProofRejected(failed.value)
        self._check(rc)

    def compress(self, proof, public_inputs):
        """lcp2_proof_compress: the compressed proof (pruned Merkle multiproofs, see include/lcp2.h; parity unpinned).  Host only.
        Lcp2Error with status -7 for a proof that could not be given back word for word."""
        pr, pis = _np_u64(proof).ravel(), _np_u64(public_inputs).ravel()
        out, words = np.zeros(self.lib.lcp2_proof_compressed_words_max(ctypes.byref(self.circ.params)), dtype=np.uint64), ctypes.c_size_t(0)
        rc = self.lib.lcp2_proof_compress(self.handle, _ptr(pr), pr.size, _ptr(pis), pis.size, _ptr(out), out.size, ctypes.byref(words))
        if rc:
            raise Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode())
        return out[:words.value].copy()

    def decompress(self, comp, public_inputs):
        """lcp2_proof_decompress: the full proof of a compressed one; Lcp2Error with status -1 for a word count that is not the one
        its query indices imply.  Host only."""
        cp, pis = _np_u64(comp).ravel(), _np_u64(public_inputs).ravel()
        out = np.zeros(self.proof_words, dtype=np.uint64)
        rc = self.lib.lcp2_proof_decompress(self.handle, _ptr(cp), cp.size, _ptr(pis), pis.size, _ptr(out), out.size)
        if rc:
            raise Lcp2Error(rc, self.lib.lcp2_status_str(rc).decode())
        return out

    def verify_batch_compressed(self, comps, public_inputs, head="host", ctx=None, offsets=None, mem=MEM_HOST):
        """lcp2_verify_batch_compressed on `ctx` (default: the handle's own context): comps is a list of compressed proofs, or with
        `offsets` (count + 1 word offsets) one array of them back to back - with mem=MEM_DEVICE a device pointer.  public_inputs:
        (count, num_public_inputs).  Returns the int32 array of failed checks, as Context.verify_batch does."""
        ctx = ctx or self.ctx
        if ctx is None:
            raise Lcp2Error(-1, "a verifier-only handle has no context: pass ctx")
        if head not in VERIFY_HEADS:
            raise Lcp2Error(-1, "head is 'host' or 'device'")
        if offsets is None:
            parts = [_np_u64(p).ravel() for p in comps]
            offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
            comps = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
        off = _np_u64(offsets).ravel()
        count = off.size - 1
        if count <= 0:
            return np.zeros(0, dtype=np.int32)
        if mem == MEM_HOST:
            keep = _np_u64(comps).ravel()
            if keep.size < int(off[-1]):
                raise Lcp2Error(-1, "offsets reach past comps")
            if not keep.size:
                keep = np.zeros(1, dtype=np.uint64)  # (empty proofs are still proofs: check 1)
            ptr = _ptr(keep)
        else:
            ptr = ctypes.c_void_p(comps)
        pis = _np_u64(public_inputs).ravel()
        npi = pis.size // count
        if npi * count != pis.size:
            raise Lcp2Error(-1, "public_inputs is not count rows")
        checks = np.zeros(count, dtype=np.int32)
        rc = self.lib.lcp2_verify_batch_compressed(ctx.handle, self.handle, ptr, _ptr(off), count, mem, _ptr(pis), npi, _ptr(checks), VERIFY_HEADS[head])
        if rc != -7:
            ctx._check(rc)
        return checks

    def verifier_data_bytes(self):
        """VerifierOnlyCircuitData::to_bytes: constants_sigmas_cap then circuit_digest"""
        out = np.zeros(((4 << self.circ.params.cap_height) + 4) * 8, dtype=np.uint8)
        self._check(self.lib.lcp2_verifier_data_to_bytes(self.handle, _ptr(out), out.size))
        return out.tobytes()

    def last_challenges(self):
        out = np.zeros(97, dtype=np.uint64)
        self._check(self.lib.lcp2_last_challenges(self.handle, _ptr(out)))
        return {"betas": out[0:4], "gammas": out[4:8], "alphas": out[8:12], "zeta": out[12:14], "fri_alpha": out[14:16],
                "fri_betas": out[16:32].reshape(8, 2), "pow_witness": int(out[32]), "query_indices": out[33:97]}

    def gate_tiers(self):
        """(degrees, bundles) per gate: the degree bound derived from the gate's program, and the bundle with which K6 evaluates the
        gate on half of the quotient coset (-1: on the whole coset)"""
        ng = len(self.circ.gateset.gates)
        deg, bun = np.zeros(ng, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
        self._check(self.lib.lcp2_circuit_gate_tiers(self.handle, ng, _ptr(deg), _ptr(bun)))
        return deg, bun

    def close(self):
        if self.handle:
            self.lib.lcp2_circuit_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
