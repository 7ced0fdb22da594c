// TEST HARNESS (not product code): what the stand-alone sanitizer programs sanitize_*_main.cpp share.  tests/checks/emu_sanitize.sh
// builds each of them with g++ under ASan + UBSan and runs it on the CPU; a program exits non-zero on a wrong value, and the
// sanitizers abort on a bad access or undefined arithmetic.
#pragma once
#include <cstdint>
#include <cstdio>

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// xorshift64 (13, 7, 17) from a fixed seed: every program draws the same words on every run
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
[[maybe_unused]] static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
