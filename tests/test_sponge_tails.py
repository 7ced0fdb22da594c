"""The sponges of the leaf and Merkle kernels compute only the rows of the last linear layer that the next step reads
(csrc/poseidon.hpp: pos_sponge_absorb, pos_mds_tail<MASK>, the zero-capacity first round).  Digests must stay what the oracle's
hash_or_noop / two_to_one give, word for word:

* on the CPU, the same sponge text with the rows outside a tail's mask poisoned (tests/emu/emu_sponge.cpp), against the oracle
  and, as a stand-alone program under ASan + UBSan, against a plain sponge on the full permutation;
* on the GPU, ctx.merkle_cap for every leaf length class: one permutation (FINAL), CAPACITY -> FINAL, FULL -> ragged FINAL."""
import ctypes as c
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import P, merkle_cap, rand_field, vp
from rows_lib import EMU, ROOT, build_emu

LEAF_LENS = [5, 7, 8, 9, 15, 16, 17, 23, 24, 135]
_leaves = {}


def leaves_of(log_leaves, leaf_len):
    """random words, one in 16 of them not canonical, and four fixed leaves: all 0, all p - 1, only the last word, all 2^64 - 1"""
    key = (log_leaves, leaf_len)
    if key not in _leaves:
        a = rand_field(np.random.default_rng(7 * leaf_len + log_leaves), (1 << log_leaves, leaf_len), canonical=False)
        a[0] = 0
        a[1] = P - 1
        a[2] = 0
        a[2, -1] = 3
        a[3] = np.uint64(2 ** 64 - 1)
        a.setflags(write=False)
        _leaves[key] = a
    return _leaves[key]


@pytest.fixture(scope="module")
def emu_sponge():
    V, u64, u32 = c.c_void_p, c.c_uint64, c.c_uint
    return build_emu("emu_sponge", (
        ("emu_hash_leaves", None, [V, u64, u64, u32, u64, V]), ("emu_merkle_level", None, [V, V, u64]),
        ("emu_sponge_round_constants", c.POINTER(u64), []), ("emu_sponge_rc_words", u32, []), ("emu_sponge_rc_zero_cap", u32, [])))


def test_zero_capacity_constants(emu_sponge, oracle):
    rc, at = emu_sponge.emu_sponge_round_constants(), emu_sponge.emu_sponge_rc_zero_cap()
    assert at + 4 == emu_sponge.emu_sponge_rc_words()
    plain = oracle.orc_poseidon_round_constants()
    assert [rc[i] for i in range(360)] == [plain[i] for i in range(360)]
    assert [rc[at + i] for i in range(4)] == [pow(int(plain[8 + i]), 7, P) for i in range(4)]


@pytest.mark.parametrize("leaf_len", [1, 4] + LEAF_LENS)
def test_poisoned_sponge_emulation_equals_the_oracle(emu_sponge, oracle, leaf_len):
    leaves = leaves_of(5, leaf_len)
    digests = np.zeros((32, 4), dtype=np.uint64)
    emu_sponge.emu_hash_leaves(vp(leaves), leaf_len, 1, leaf_len, 32, vp(digests))
    assert (digests == merkle_cap(oracle, leaves, 5)).all()  # a cap as high as the tree: the leaf digests
    parents = np.zeros((16, 4), dtype=np.uint64)
    emu_sponge.emu_merkle_level(vp(digests), vp(parents), 16)
    assert (parents == merkle_cap(oracle, leaves, 4)).all()


def test_sponge_emulation_program_under_sanitizers(tmp_path):
    """tests/emu/sanitize_sponge_main.cpp as tests/checks/sponge_sanitize.sh builds and runs it: a stand-alone program (here with the
    sanitizers' runtimes linked in, so that it starts the same way whatever else the process loads)"""
    exe = str(tmp_path / "sanitize_sponge")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(EMU, "sanitize_sponge_main.cpp")], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("sanitize_sponge: ")


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
@pytest.mark.parametrize("log_leaves,cap_height", [(9, 0), (9, 4), (4, 4)])  # (4, 4) runs no Merkle level: the leaf tails alone
def test_merkle_cap_with_masked_tails(gpu_ctx, oracle, leaf_len, log_leaves, cap_height):
    leaves = leaves_of(log_leaves, leaf_len)
    got = gpu_ctx.merkle_cap(np.array(leaves), cap_height)
    assert (got == merkle_cap(oracle, leaves, cap_height)).all()
