#!/bin/bash
# The portable texts the device shares with the CPU under AddressSanitizer + UndefinedBehaviorSanitizer, as four stand-alone
# programs run one after another (tests/emu/sanitize_common.hpp): csrc/pos_rows.hpp, csrc/u32_rows.hpp and csrc/light_gates.hpp
# (sanitize_main.cpp with emu_pos.cpp, emu_u32.cpp and emu_gates.cpp), csrc/pos_plan.hpp with csrc/rec_rows.hpp (sanitize_plan_main.cpp), csrc/sha_rows.hpp
# (sanitize_sha_main.cpp) and csrc/verify_query.hpp (sanitize_verify_main.cpp).  CPU only; the first failure ends the script.
set -e
cd "$(dirname "$0")/../.."
run() {  # run <program> <sources...>
  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -o "/tmp/emu_$1" "${@:2}"
  ASAN_OPTIONS=abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "/tmp/emu_$1"
}
run sanitize_rows tests/emu/sanitize_main.cpp tests/emu/emu_pos.cpp tests/emu/emu_u32.cpp tests/emu/emu_gates.cpp
run sanitize_plan tests/emu/sanitize_plan_main.cpp
run sanitize_sha tests/emu/sanitize_sha_main.cpp
run sanitize_verify tests/emu/sanitize_verify_main.cpp
