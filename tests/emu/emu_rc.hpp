// TEST HARNESS (not product code): the round-constant table of the emulation programs, derived once: the 360 round constants, then
// the constants of the grouped walk (csrc/poseidon.hpp POS_RC_WORDS), as lcp2_ctx_create uploads it.
#pragma once
#include "../../eth-lc-plonky2_amd/csrc/poseidon.hpp"

inline const lcp2::u64 *emu_round_constants() {
  static const struct Table {
    lcp2::u64 rc[lcp2::POS_RC_WORDS];
    Table() { lcp2::pos_derive_round_constants(rc); lcp2::pos_extend_round_constants(rc); }
  } table;
  return table.rc;
}
