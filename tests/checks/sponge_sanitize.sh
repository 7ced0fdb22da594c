#!/bin/bash
# The sponge of the leaf and Merkle kernels (csrc/poseidon.hpp, tests/emu/emu_sponge.cpp) under AddressSanitizer +
# UndefinedBehaviorSanitizer as a stand-alone program, built and run the way emu_sanitize.sh builds and runs its four
# (tests/emu/sanitize_sponge_main.cpp; tests/test_sponge_tails.py runs the same program in the suite).  CPU only.
set -e
cd "$(dirname "$0")/../.."
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o /tmp/emu_sanitize_sponge tests/emu/sanitize_sponge_main.cpp
ASAN_OPTIONS=abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 /tmp/emu_sanitize_sponge
