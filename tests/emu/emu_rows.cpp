// TEST HARNESS (not product code): csrc/circuit_rows.hpp compiled for the CPU - the constant columns, the identity sigmas, the key pass
// with its two bitmaps, the radix sort with the kernels' tiling (threads x run entries per tile, each lane ranking its own contiguous
// run; both are parameters, so that tiny lists cross tile borders) and the cycle pass - lane by lane in the order the entry point
// launches them; `reverse` runs the lanes of every pass from the last to the first, which must change nothing.
// tests/test_circuit_rows_emu.py holds the results to circuit.expand_rows_model.  Built by tests/rows_lib.py build_emu with g++ (and by
// hand with sanitizers: sanitize_rows_main.cpp); never loaded by the package.
#include <cstring>
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/circuit_rows.hpp"
#include "../../eth-lc-plonky2_amd/csrc/ntt_host.hpp"

using namespace lcp2;

namespace {
struct Roots {
  std::vector<u64> lo, hi;
  TwoLevelTable t;
  explicit Roots(u32 lg) {
    t.h = (lg + 1) / 2;
    const u64 w = gl_root_of_unity(lg);
    lo = make_pow_table(w, 1, (size_t)1 << t.h);
    hi = make_pow_table(w, 1ull << t.h, (size_t)1 << (lg - t.h));
    t.lo = lo.data(); t.hi = hi.data();
  }
};
template <class F>
void lanes(u64 count, int reverse, F f) {
  for (u64 k = 0; k < count; k++) f(reverse ? count - 1 - k : k);
}
}  // namespace

extern "C" {
// what the entry points refuse before anything runs: 0, or LCP2_E_INVALID / LCP2_E_UNSUPPORTED with the reason in *why
int emu_rows_args(const lcp2_circuit_desc *d, const lcp2_circuit_rows *r, const char **why) {
  bool unsupported = false;
  *why = rows_args_problem(d, r, &unsupported);
  return !*why ? LCP2_OK : unsupported ? LCP2_E_UNSUPPORTED : LCP2_E_INVALID;
}
const char *emu_rows_problem_str(unsigned problem) { return rows_problem_str(problem); }
unsigned emu_rows_passes(unsigned num_classes) { return rows_passes(num_classes); }

// out [num_constants + num_routed_wires][n].  info[0]: the refusal word of the list, info[1]: of gate_of_row (ROW_NO_PROBLEM: none),
// info[2], info[3]: the two list indices of a double binding (~0: none), info[4]: sort passes run, info[5]: tiles.
// Returns 0, or LCP2_E_INVALID when one of the four says so (the sort and the cycles have then not run)
int emu_rows_expand(const lcp2_circuit_desc *d, const lcp2_circuit_rows *r, unsigned threads, unsigned run, int reverse, u64 *out, u64 *info) {
  const lcp2_params &p = d->params;
  const u64 n = 1ull << p.degree_bits, cells = (u64)p.num_routed_wires * n, M = r->num_bindings;
  const u32 NC = p.num_constants, NR = p.num_routed_wires, S = d->num_selectors, K = NC - S, NG = d->num_gates;
  std::vector<GateSelDev> gates(NG);
  for (u32 g = 0; g < NG; g++) gates[g] = {d->gates[g].selector_index, d->gates[g].selector_value};
  std::vector<u64> k_is(NR);
  for (u32 j = 0; j < NR; j++) k_is[j] = gl_canon(d->k_is[j]);
  Roots R(p.degree_bits);
  const BindingDev *list = (const BindingDev *)r->bindings;
  info[0] = info[1] = ROW_NO_PROBLEM; info[2] = info[3] = ~0ull; info[4] = info[5] = 0;
  // (a)
  lanes((u64)NC * n, reverse, [&](u64 at) {
    const u32 col = (u32)(at / n);
    const u64 row = at % n;
    const u32 gate = row < r->num_rows ? r->gate_of_row[row] : r->pad_gate;
    if (gate >= NG) { if (col == 0) rows_fold_min(&info[1], row_refusal(row, ROWS_GATE)); return; }
    out[at] = rows_constant_value(gates.data(), gate, S, K, (const u64 *)r->row_constants, r->num_rows, col, row);
  });
  // (b) in groups of 8 columns, as the kernel
  u64 *sigmas = out + (u64)NC * n;
  const u32 groups = (NR + 7) / 8;
  lanes((u64)groups * n, reverse, [&](u64 at) { rows_identity_lane(k_is.data(), R.t, n, NR, (u32)(at / n) * 8, 8, at % n, sigmas); });
  // (c)
  std::vector<u64> keys[2] = {std::vector<u64>(M), std::vector<u64>(M)};
  std::vector<u32> bound((cells + 31) / 32, 0), twice((cells + 31) / 32, 0);
  u32 any_twice = 0;
  lanes(M, reverse, [&](u64 i) {
    if (const u32 problem = rows_key_lane(list, i, n, NR, r->num_classes, keys[0].data(), bound.data(), twice.data(), &any_twice))
      rows_fold_min(&info[0], row_refusal(i, problem));
  });
  if (info[1] != ROW_NO_PROBLEM || info[0] != ROW_NO_PROBLEM) return LCP2_E_INVALID;
  if (any_twice) {
    lanes(M, reverse, [&](u64 i) { rows_twice_first(list, i, n, NR, r->num_classes, twice.data(), &info[2]); });
    lanes(M, reverse, [&](u64 i) { rows_twice_second(list, i, info[2], &info[3]); });
    return LCP2_E_INVALID;
  }
  // (d)
  const u64 tile = (u64)threads * run, tiles = (M + tile - 1) / tile;
  const u32 passes = M ? rows_passes(r->num_classes) : 0;
  u32 side = 0;
  for (u32 pass = 0; pass < passes; pass++, side ^= 1) {
    const u64 *src = keys[side].data();
    auto my_run = [&](u64 t, u64 lane, u64 *begin, u64 *end) {
      const u64 base = t * tile + lane * run;
      *begin = base < M ? base : M;
      *end = base + run < M ? base + run : M;
    };
    std::vector<u32> table(ROWS_DIGITS * tiles, 0);
    lanes(tiles * threads, reverse, [&](u64 at) {  // k_rows_hist
      u64 begin, end;
      my_run(at / threads, at % threads, &begin, &end);
      u32 c[ROWS_DIGITS];
      rows_count_run(src, begin, end, pass, c);
      for (u32 dg = 0; dg < ROWS_DIGITS; dg++) table[dg * tiles + at / threads] += c[dg];
    });
    u32 running = 0;  // k_rows_scan
    for (u32 &v : table) { const u32 mine = v; v = running; running += mine; }
    std::vector<u32> below((size_t)threads * ROWS_DIGITS);
    for (u64 t = 0; t < tiles; t++) {  // k_rows_scatter: the prefix over the lanes of a block, then every lane its run
      u32 sum[ROWS_DIGITS] = {0};
      for (u64 lane = 0; lane < threads; lane++) {
        u64 begin, end;
        my_run(t, lane, &begin, &end);
        u32 c[ROWS_DIGITS];
        rows_count_run(src, begin, end, pass, c);
        for (u32 dg = 0; dg < ROWS_DIGITS; dg++) { below[lane * ROWS_DIGITS + dg] = sum[dg]; sum[dg] += c[dg]; }
      }
      lanes(threads, reverse, [&](u64 lane) {
        u64 begin, end;
        my_run(t, lane, &begin, &end);
        u32 at[ROWS_DIGITS];
        for (u32 dg = 0; dg < ROWS_DIGITS; dg++) at[dg] = table[dg * tiles + t] + below[lane * ROWS_DIGITS + dg];
        rows_scatter_run(src, begin, end, pass, at, keys[side ^ 1].data());
      });
    }
  }
  info[4] = passes; info[5] = tiles;
  // (e)
  lanes(M, reverse, [&](u64 q) { rows_cycle_lane(list, keys[side].data(), M, q, k_is.data(), R.t, n, sigmas); });
  return LCP2_OK;
}
}
