#!/bin/bash
# The row texts the device shares with the CPU (csrc/pos_rows.hpp, csrc/u32_rows.hpp) under AddressSanitizer +
# UndefinedBehaviorSanitizer as a stand-alone program: tests/emu/sanitize_main.cpp with emu_pos.cpp and emu_u32.cpp.  CPU only.
set -e
cd "$(dirname "$0")/../.."
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o /tmp/emu_sanitize \
    tests/emu/sanitize_main.cpp tests/emu/emu_pos.cpp tests/emu/emu_u32.cpp
ASAN_OPTIONS=abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 /tmp/emu_sanitize
