"""CircuitBuilder::set_compact_build of the C++ host layer (tests/cpp/test_compact_build.cpp, built here as test_fill_copies is): for
ContractState and the SHA-256 Merkle gadget of height 2, the circuit built without the expanded matrix and attached through
lcp2_circuit_create_from_rows has the digest, the cap and the proof of the ordinary build, word for word, and the matrix it expands on
demand is the ordinary one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_compact_build")


def build_binary():
    import cpp_build
    cpp_build.build()   # liblcp2.so, golden_data.hpp
    srcs = [os.path.join(cpp_build.CPP, "test_compact_build.cpp")] + [os.path.join(cpp_build.HOST, f) for f in cpp_build.HOST_SOURCES]
    deps = srcs + [os.path.join(cpp_build.HOST, f) for f in os.listdir(cpp_build.HOST) if f.endswith(".hpp")] + cpp_build.SHARED_HEADERS + [
        os.path.join(cpp_build.CPP, "golden_data.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        pkg = os.path.join(ROOT, "eth-lc-plonky2_amd")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", BIN] + srcs + ["-L", pkg, "-llcp2", "-Wl,-rpath," + pkg], check=True)
    return BIN


def uploads(stdout):
    return dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in re.finditer(r"upload: (\S+) ordinary (\d+) compact (\d+) bytes", stdout))


def test_compact_description_expands_to_the_ordinary_matrix():
    """no device: the compact build holds no matrix, what it expands on demand is the ordinary build's, and its upload is far smaller"""
    r = subprocess.run([build_binary(), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_compact_build cpu ... ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert set(uploads(r.stdout)) == {"ContractState", "merkle_tree_height_2"}
    assert subprocess.run([BIN], capture_output=True, text=True, timeout=60).returncode == 2


@pytest.mark.gpu
def test_digest_cap_and_proof_equal_the_ordinary_build():
    r = subprocess.run([build_binary(), "gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "test_compact_build gpu ... ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for ordinary, compact in uploads(r.stdout).values():
        assert 0 < compact < ordinary // 4
