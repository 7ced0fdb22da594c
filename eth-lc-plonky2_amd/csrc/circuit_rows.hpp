// lcp2_circuit_rows_expand as portable text: what the kernels of circuit_rows.hip run per cell and per list entry, and what
// tests/emu/emu_rows.cpp runs on the CPU.  The opposite direction of witness_fill.hpp: from one gate index per row, a few gate
// constants per row and the list of bound routed cells with their copy class to the preprocessed columns that plonky2's build()
// hands over expanded (selector columns, gate-constant columns, sigma columns).
//
// The passes, in the order the entry point launches them (every lane writes words of its own: the result does not depend on the
// order the lanes ran in; atomics only count digits, set bits of a bitmap and keep the smallest refused index):
//   (a) constants   one lane per (constant column, row): rows_constant_value - the selector value of the row's gate, 0xFFFFFFFF in the
//                   other selector columns, the transposition of row_constants behind them.  A gate index out of range is refused.
//   (b) identity    one lane per routed cell: its own id k_is[col] w^row (rows_cell_id, the inverse of wc_decode_cell).
//   (c) keys        one lane per list entry: range checks, the cell's bit in a bitmap over the routed cells (a bit that was already
//                   set marks the cell in a second bitmap: bound twice), and the sort key cls << 32 | list index.
//   (d) grouping    a stable LSD radix sort of the keys by cls, 4 bits per pass over ceil(log2 num_classes) bits.  A tile is
//                   threads x run consecutive entries; lane l ranks the run [l run, (l + 1) run) of its tile in list order
//                   (rows_count_run, rows_scatter_run), so a tile is stable, and the per-(digit, tile) counts - digit-major - are
//                   scanned once per pass, so the tiles are stable among each other.  The list index in the low half of a key is
//                   never sorted on: it only travels, and ends up ascending inside each class because every pass is stable.
//   (e) cycles      one lane per sorted entry: the bound cells of a class form ONE cycle in list order - each maps to the next
//                   entry of its class, the last one to the first (rows_successor; the tail finds its head by a binary search for
//                   the first key of its class).  A class with one bound cell writes its own id again.
#pragma once
#include "../../include/lcp2.h"
#include "gl64.hpp"
#include "ntt.hpp"
#include "row_flag.hpp"

namespace lcp2 {

constexpr u32 ROWS_DIGIT_BITS = 4, ROWS_DIGITS = 1u << ROWS_DIGIT_BITS;
constexpr u32 ROWS_UNUSED_SELECTOR = 0xFFFFFFFFu;  // plonky2 gates/selectors.rs UNUSED_SELECTOR
constexpr u64 ROWS_MAX_CELLS = 1ull << 32;         // cell indices and list indices are 32-bit
// why an entry is refused (the problem byte of a refusal word)
enum : u32 { ROWS_BIND_ROW = 1, ROWS_BIND_COLUMN = 2, ROWS_BIND_CLASS = 3, ROWS_BIND_TWICE = 4, ROWS_GATE = 5 };
inline const char *rows_problem_str(u32 problem) {
  switch (problem) {
    case ROWS_BIND_ROW: return "row out of range";
    case ROWS_BIND_COLUMN: return "column is no routed wire";
    case ROWS_BIND_CLASS: return "class out of range";
    case ROWS_BIND_TWICE: return "cell bound twice";
    default: return "gate index out of range";
  }
}

struct BindingDev { u32 row, col, cls; };  // = lcp2_copy_binding
struct GateSelDev { u32 selector_index, selector_value; };  // the two selector words of an lcp2_gate

// folds: the kernels' atomics, plain words on the CPU
LCP2_HD u32 rows_fold_or(u32 *word, u32 v) {  // -> the word before
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicOr(word, v);
#else
  const u32 old = *word;
  *word |= v;
  return old;
#endif
}
LCP2_HD void rows_fold_min(u64 *word, u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin((unsigned long long *)word, (unsigned long long)v);
#else
  if (v < *word) *word = v;
#endif
}

// the key bits of the sort and its passes
LCP2_HD u32 rows_key_bits(u32 num_classes) {
  u32 bits = 0;
  while (bits < 32 && (1ull << bits) < num_classes) bits++;
  return bits;
}
LCP2_HD u32 rows_passes(u32 num_classes) { return (rows_key_bits(num_classes) + ROWS_DIGIT_BITS - 1) / ROWS_DIGIT_BITS; }

// ---- (a) constant column `col` (selectors first) at `row`; gate: the row's gate index, already known to be < num_gates
LCP2_HD u64 rows_selector_value(const GateSelDev &g, u32 col) { return g.selector_index == col ? g.selector_value : ROWS_UNUSED_SELECTOR; }
// row_constants: row-major [num_rows][num_gate_constants], null = zeros
LCP2_HD u64 rows_constant_value(const GateSelDev *gates, u32 gate, u32 num_selectors, u32 num_gate_constants, const u64 *row_constants,
                                u64 num_rows, u32 col, u64 row) {
  if (col < num_selectors) return rows_selector_value(gates[gate], col);
  if (!row_constants || row >= num_rows) return 0;
  return row_constants[row * num_gate_constants + (col - num_selectors)];
}

// ---- (b) the id of a routed cell: the value wc_decode_cell takes apart.  k_is canonical, roots: w_n^e (NttHost::root_table)
LCP2_HD u64 rows_cell_id(const u64 *k_is, const TwoLevelTable &roots, u32 col, u64 row) { return gl_mul(k_is[col], two_level(roots, row)); }
// one lane of the identity pass: the ids of `row` in the routed columns [col0, col0 + count), w^row looked up once
LCP2_HD void rows_identity_lane(const u64 *k_is, const TwoLevelTable &roots, u64 n, u32 num_routed, u32 col0, u32 count, u64 row, u64 *sigmas) {
  const u64 w = two_level(roots, row);
  for (u32 t = 0; t < count && col0 + t < num_routed; t++) sigmas[(u64)(col0 + t) * n + row] = gl_mul(k_is[col0 + t], w);
}

// ---- (c) entry i: 0, or why it is refused for its range
LCP2_HD u32 rows_binding_problem(const BindingDev &b, u64 n, u32 num_routed, u32 num_classes) {
  if (b.row >= n) return ROWS_BIND_ROW;
  if (b.col >= num_routed) return ROWS_BIND_COLUMN;
  if (b.cls >= num_classes) return ROWS_BIND_CLASS;
  return 0;
}
// lane i of the key pass: keys[i], the bit of its cell in `bound`, and in `twice` when it was set before.  Returns 0 or the range
// problem of an entry that takes part in nothing (its key sorts as class 0; the call is refused before the cycles are written)
LCP2_HD u32 rows_key_lane(const BindingDev *bindings, u64 i, u64 n, u32 num_routed, u32 num_classes, u64 *keys, u32 *bound, u32 *twice, u32 *any_twice) {
  const BindingDev b = bindings[i];
  const u32 problem = rows_binding_problem(b, n, num_routed, num_classes);
  keys[i] = (problem ? 0ull : (u64)b.cls << 32) | i;
  if (problem) return problem;
  const u64 cell = (u64)b.col * n + b.row;
  const u32 bit = 1u << (cell & 31);
  if (rows_fold_or(&bound[cell >> 5], bit) & bit) {
    rows_fold_or(&twice[cell >> 5], bit);
    *any_twice = 1;  // every such lane stores the same 1
  }
  return 0;
}
// after the whole key pass, only when a cell was bound twice: the smallest list index whose cell is bound more than once ...
LCP2_HD void rows_twice_first(const BindingDev *bindings, u64 i, u64 n, u32 num_routed, u32 num_classes, const u32 *twice, u64 *first) {
  const BindingDev b = bindings[i];
  if (rows_binding_problem(b, n, num_routed, num_classes)) return;
  const u64 cell = (u64)b.col * n + b.row;
  if (twice[cell >> 5] >> (cell & 31) & 1) rows_fold_min(first, i);
}
// ... and the next entry that binds the same cell
LCP2_HD void rows_twice_second(const BindingDev *bindings, u64 i, u64 first, u64 *second) {
  const BindingDev a = bindings[first], b = bindings[i];
  if (i != first && a.row == b.row && a.col == b.col) rows_fold_min(second, i);
}

// ---- (d) one run of a tile: the entries [begin, end) of `keys`, in list order
#if defined(__HIP_DEVICE_COMPILE__)
#define LCP2_ROWS_UNROLL _Pragma("unroll")
#else
#define LCP2_ROWS_UNROLL
#endif
LCP2_HD u32 rows_digit(u64 key, u32 pass) { return (u32)(key >> (32 + pass * ROWS_DIGIT_BITS)) & (ROWS_DIGITS - 1); }
LCP2_HD void rows_count_run(const u64 *keys, u64 begin, u64 end, u32 pass, u32 count[ROWS_DIGITS]) {
  LCP2_ROWS_UNROLL
  for (u32 d = 0; d < ROWS_DIGITS; d++) count[d] = 0;
  for (u64 i = begin; i < end; i++) {
    const u32 mine = rows_digit(keys[i], pass);
    LCP2_ROWS_UNROLL
    for (u32 d = 0; d < ROWS_DIGITS; d++) count[d] += mine == d ? 1u : 0u;  // (no array indexed by a value: the counts stay in registers)
  }
}
// at[d]: where the run's first entry of digit d goes (the entries of the digit in front of this run, in all tiles)
LCP2_HD void rows_scatter_run(const u64 *keys, u64 begin, u64 end, u32 pass, u32 at[ROWS_DIGITS], u64 *out) {
  for (u64 i = begin; i < end; i++) {
    const u64 key = keys[i];
    const u32 mine = rows_digit(key, pass);
    u32 to = 0;
    LCP2_ROWS_UNROLL
    for (u32 d = 0; d < ROWS_DIGITS; d++) { if (mine == d) { to = at[d]; at[d] = to + 1; } }
    out[to] = key;
  }
}

// ---- (e) the sorted position of the entry that follows the one at position p in its class's cycle
LCP2_HD u64 rows_successor(const u64 *sorted, u64 count, u64 p) {
  const u64 cls = sorted[p] >> 32;
  if (p + 1 < count && sorted[p + 1] >> 32 == cls) return p + 1;
  u64 lo = 0, hi = p;  // the tail: the first position whose key is not below cls << 32 is the head (it is <= p)
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (sorted[mid] >> 32 < cls) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// lane p of the cycle pass: sigma of the entry's cell = the id of its successor's cell
LCP2_HD void rows_cycle_lane(const BindingDev *bindings, const u64 *sorted, u64 count, u64 p, const u64 *k_is, const TwoLevelTable &roots, u64 n, u64 *sigmas) {
  const BindingDev cur = bindings[(u32)sorted[p]], nxt = bindings[(u32)sorted[rows_successor(sorted, count, p)]];
  sigmas[(u64)cur.col * n + cur.row] = rows_cell_id(k_is, roots, nxt.col, nxt.row);
}

// ---- what the entry points refuse before anything is uploaded: nullptr, or the reason with *unsupported telling LCP2_E_UNSUPPORTED from
// LCP2_E_INVALID.  desc and rows non-null; desc->params already checked
inline const char *rows_args_problem(const lcp2_circuit_desc *d, const lcp2_circuit_rows *r, bool *unsupported) {
  *unsupported = false;
  const lcp2_params &p = d->params;
  const u64 n = 1ull << p.degree_bits;
  if (!d->k_is || !d->gates || d->num_gates == 0) return "null description field";
  if (d->num_selectors > p.num_constants) return "more selector columns than constant columns";
  if ((unsigned)r->bindings_mem > 1) return "bad lcp2_mem";
  if (r->num_rows && !r->gate_of_row) return "gate_of_row is null but num_rows is not zero";
  if (r->num_bindings && !r->bindings) return "the binding list is null but its count is not zero";
  if (r->num_rows > n) return "num_rows > n";
  if (r->pad_gate >= d->num_gates) return "pad_gate out of range";
  for (u32 g = 0; g < d->num_gates; g++)
    if (d->gates[g].selector_index >= d->num_selectors) return "a gate's selector_index is no selector column";
  *unsupported = true;
  if ((u64)p.num_routed_wires * n >= ROWS_MAX_CELLS) return "2^32 routed cells or more (cell indices are 32-bit)";
  if ((u64)r->num_bindings >= ROWS_MAX_CELLS) return "2^32 bindings or more (list indices are 32-bit)";
  *unsupported = false;
  return nullptr;
}

}  // namespace lcp2
