"""CircuitData::diagnose of the C++ host layer (tests/cpp/test_diagnose.cpp, built here): one broken ArithmeticGate row of the
smallest circuit the builder makes is named by the builder's gate name and its row, as orc_check_witness finds it.  CPU mode: the
text of the report, and the documented refusal of the device calls without attach_gpu.  GPU mode: lcp2_check_witness on the device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_diagnose")


def build_binary():
    import cpp_build
    cpp_build.build()   # liblcp2.so, liboracle.so
    srcs = [os.path.join(cpp_build.CPP, "test_diagnose.cpp")] + [os.path.join(cpp_build.HOST, f) for f in cpp_build.HOST_SOURCES]
    deps = srcs + [os.path.join(cpp_build.HOST, f) for f in os.listdir(cpp_build.HOST) if f.endswith(".hpp")] + cpp_build.SHARED_HEADERS + [
        os.path.join(ROOT, "oracle", "plonk.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        pkg, orc = os.path.join(ROOT, "eth-lc-plonky2_amd"), os.path.join(ROOT, "oracle")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", BIN] + srcs + ["-L", pkg, "-llcp2", "-L", orc, "-loracle",
                        "-Wl,-rpath," + pkg, "-Wl,-rpath," + orc, "-fopenmp"], check=True)
    return BIN


def run(mode):
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "16")
    r = subprocess.run([build_binary(), mode], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "test_diagnose %s ... ok" % mode in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    return [ln[len("diagnose: "):] for ln in r.stdout.splitlines() if ln.startswith("diagnose: ")]


def test_report_text_names_the_gate_and_the_row():
    texts = run("cpu")
    assert re.fullmatch(r"row \d+, gate ArithmeticGate, constraint \d+ \(\d+ gate constraints violated\)", texts[0])
    assert re.fullmatch(r"row (\d+), gate ArithmeticGate, constraint \d+ \(\d+ gate constraints violated\); copy constraint \(\1, 3\) != \(\d+, 0\) \(2 cells\)", texts[1])


@pytest.mark.gpu
def test_diagnose_on_the_device_names_the_broken_arithmetic_row():
    texts = run("gpu")
    assert re.match(r"row \d+, gate ArithmeticGate, constraint \d+ \(\d+ gate constraints violated\); copy constraint \(\d+, 3\) != \(\d+, \d+\) \(\d+ cells\)$", texts[0])
    assert texts[1] == "the witness satisfies every gate and copy constraint"
