"""CircuitData::set_fill_copies of the C++ host layer (tests/cpp/test_fill_copies.cpp, built here as test_diagnose is): for
ContractState and a circuit with one two_to_one_sha256 the proof with the opt-in on - one host-written cell per variable class
through lcp2_witness_fill_copies - equals the proof with it off, word for word; the cells sent per proof are printed for both modes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_fill_copies")


def build_binary():
    import cpp_build
    cpp_build.build()   # liblcp2.so, golden_data.hpp
    srcs = [os.path.join(cpp_build.CPP, "test_fill_copies.cpp")] + [os.path.join(cpp_build.HOST, f) for f in cpp_build.HOST_SOURCES]
    deps = srcs + [os.path.join(cpp_build.HOST, f) for f in os.listdir(cpp_build.HOST) if f.endswith(".hpp")] + cpp_build.SHARED_HEADERS + [
        os.path.join(cpp_build.CPP, "golden_data.hpp")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        pkg = os.path.join(ROOT, "eth-lc-plonky2_amd")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", BIN] + srcs + ["-L", pkg, "-llcp2", "-Wl,-rpath," + pkg], check=True)
    return BIN


def test_the_binary_builds_and_refuses_other_modes():
    r = subprocess.run([build_binary(), "cpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_proofs_with_and_without_the_opt_in_are_equal():
    r = subprocess.run([build_binary(), "gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "test_fill_copies gpu ... ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    cells = dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in re.finditer(r"cells: (\S+) off (\d+) on (\d+)", r.stdout))
    assert set(cells) == {"ContractState", "two_to_one_sha256"}
    for off, on in cells.values():
        assert 0 < on <= off
