// lcp2_circuit_rows_expand and lcp2_circuit_create_from_rows: the preprocessed columns of a circuit (selector, gate-constant and sigma
// columns) built on the device from one gate index per row, the gate constants per row and the list of bound routed cells with
// their copy class, instead of the expanded matrix written on the host (plonky2: the tail of circuit_builder.rs::build).  The per-cell
// and per-entry texts are circuit_rows.hpp (portable: tests/emu/emu_rows.cpp runs them on the CPU); here are the kernels and the two
// entry points.  The column passes are bandwidth bound (one lane per cell, rows in the fast dimension: contiguous stores); the
// passes over the list are small beside them - 8 bytes of key per binding and pass against 8 bytes per routed CELL of the identity.
#include "circuit_state.hpp"
#include "row_stage.hpp"
#include "circuit_rows.hpp"

using namespace lcp2;

namespace lcp2 {
constexpr u32 ROWS_THREADS = 256;
constexpr u32 ROWS_RUN = 8;                        // list entries a lane ranks: 64 contiguous bytes of keys
constexpr u32 ROWS_TILE = ROWS_THREADS * ROWS_RUN;  // entries per block of a sort pass
constexpr u32 ROWS_ID_WIRES = 8;                   // routed columns per lane of the identity pass (one w^row for all of them)
constexpr u32 ROWS_WAVES = ROWS_THREADS / 64;

struct RowsShape {
  u64 n, num_rows;
  u32 num_selectors, num_gate_constants, num_gates, pad_gate, num_routed, num_classes;
};

// (a) blockIdx.y = constant column
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_constants(const GateSelDev *__restrict__ gates, const u32 *__restrict__ gate_of_row,
                                                                 const u64 *__restrict__ row_constants, RowsShape sh, u64 *__restrict__ out, u64 *flag) {
  const u32 col = blockIdx.y;
  const u64 row = (u64)blockIdx.x * ROWS_THREADS + threadIdx.x;
  if (row >= sh.n) return;
  const u32 gate = row < sh.num_rows ? gate_of_row[row] : sh.pad_gate;
  if (gate >= sh.num_gates) {
    if (col == 0) atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(row, ROWS_GATE));
    return;
  }
  out[(u64)col * sh.n + row] = rows_constant_value(gates, gate, sh.num_selectors, sh.num_gate_constants, row_constants, sh.num_rows, col, row);
}
// (b) blockIdx.y = group of ROWS_ID_WIRES routed columns
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_identity(const u64 *__restrict__ k_is, TwoLevelTable roots, u64 n, u32 num_routed, u64 *__restrict__ sigmas) {
  const u64 row = (u64)blockIdx.x * ROWS_THREADS + threadIdx.x;
  if (row < n) rows_identity_lane(k_is, roots, n, num_routed, blockIdx.y * ROWS_ID_WIRES, ROWS_ID_WIRES, row, sigmas);
}
// (c) one lane per list entry
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_keys(const BindingDev *__restrict__ bindings, u64 count, RowsShape sh, u64 *__restrict__ keys, u32 *bound,
                                                            u32 *twice, u32 *any_twice, u64 *flag) {
  const u64 i = (u64)blockIdx.x * ROWS_THREADS + threadIdx.x;
  if (i >= count) return;
  if (const u32 problem = rows_key_lane(bindings, i, sh.n, sh.num_routed, sh.num_classes, keys, bound, twice, any_twice))
    atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(i, problem));
}
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_twice_first(const BindingDev *__restrict__ bindings, u64 count, RowsShape sh, const u32 *__restrict__ twice, u64 *res) {
  const u64 i = (u64)blockIdx.x * ROWS_THREADS + threadIdx.x;
  if (i < count) rows_twice_first(bindings, i, sh.n, sh.num_routed, sh.num_classes, twice, &res[0]);
}
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_twice_second(const BindingDev *__restrict__ bindings, u64 count, u64 *res) {
  const u64 i = (u64)blockIdx.x * ROWS_THREADS + threadIdx.x;
  if (i < count && res[0] < count) rows_twice_second(bindings, i, res[0], &res[1]);
}

// (d) the run of this lane in this block's tile
static __device__ __forceinline__ void rows_my_run(u64 count, u64 *begin, u64 *end) {
  const u64 base = (u64)blockIdx.x * ROWS_TILE + (u64)threadIdx.x * ROWS_RUN;
  *begin = base < count ? base : count;
  *end = base + ROWS_RUN < count ? base + ROWS_RUN : count;
}
// table[digit][tile] = the entries of the tile with that digit
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_hist(const u64 *__restrict__ keys, u64 count, u32 pass, u32 tiles, u32 *__restrict__ table) {
  __shared__ u32 wave_total[ROWS_DIGITS][ROWS_WAVES];
  u64 begin, end;
  rows_my_run(count, &begin, &end);
  u32 c[ROWS_DIGITS];
  rows_count_run(keys, begin, end, pass, c);
#pragma unroll
  for (u32 d = 0; d < ROWS_DIGITS; d++) {
    u32 v = c[d];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wave_total[d][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < ROWS_DIGITS) {
    u32 all = 0;
#pragma unroll
    for (u32 k = 0; k < ROWS_WAVES; k++) all += wave_total[threadIdx.x][k];
    table[(u64)threadIdx.x * tiles + blockIdx.x] = all;
  }
}
// one block: table[0 .. count) -> the sums in front of each entry, in place (the scan of witness_fill.hip's tile sums)
__global__ __launch_bounds__(1024) void k_rows_scan(u32 *table, u32 count) {
  __shared__ u32 part[1024];
  const u32 t = threadIdx.x, piece = (count + 1023) / 1024;
  const u32 a = (u64)t * piece < count ? t * piece : count, b = (u64)a + piece < count ? a + piece : count;
  u32 mine = 0;
  for (u32 i = a; i < b; i++) mine += table[i];
  part[t] = mine;
  __syncthreads();
  for (u32 off = 1; off < 1024; off <<= 1) {
    const u32 v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  u32 running = part[t] - mine;
  for (u32 i = a; i < b; i++) { const u32 v = table[i]; table[i] = running; running += v; }
}
// table scanned: every entry of the tile to its place, runs in lane order, a run in list order
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_scatter(const u64 *__restrict__ keys, u64 count, u32 pass, u32 tiles, const u32 *__restrict__ table,
                                                               u64 *__restrict__ out) {
  __shared__ u32 wave_total[ROWS_DIGITS][ROWS_WAVES];
  u64 begin, end;
  rows_my_run(count, &begin, &end);
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 at[ROWS_DIGITS];
  rows_count_run(keys, begin, end, pass, at);
#pragma unroll
  for (u32 d = 0; d < ROWS_DIGITS; d++) {
    const u32 mine = at[d];
    u32 v = mine;  // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const u32 o = __shfl_up(v, off); if ((int)lane >= off) v += o; }
    if (lane == 63) wave_total[d][wave] = v;
    at[d] = v - mine;
  }
  __syncthreads();
#pragma unroll
  for (u32 d = 0; d < ROWS_DIGITS; d++) {
    u32 below = table[(u64)d * tiles + blockIdx.x];
#pragma unroll
    for (u32 k = 0; k < ROWS_WAVES; k++) below += k < wave ? wave_total[d][k] : 0;
    at[d] += below;
  }
  rows_scatter_run(keys, begin, end, pass, at, out);
}
// (e) one lane per sorted entry
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_cycles(const BindingDev *__restrict__ bindings, const u64 *__restrict__ sorted, u64 count,
                                                              const u64 *__restrict__ k_is, TwoLevelTable roots, u64 n, u64 *sigmas) {
  const u64 p = (u64)blockIdx.x * ROWS_THREADS + threadIdx.x;
  if (p < count) rows_cycle_lane(bindings, sorted, count, p, k_is, roots, n, sigmas);
}

namespace {
size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// null pointers aside, what both entry points refuse before anything is allocated or uploaded
int rows_guard(lcp2_ctx *ctx, const lcp2_circuit_desc *d, const lcp2_circuit_rows *r) {
  LCP2_TRY(check_params(ctx, d->params));
  bool unsupported;
  if (const char *why = rows_args_problem(d, r, &unsupported)) return ctx->fail(unsupported ? LCP2_E_UNSUPPORTED : LCP2_E_INVALID, std::string("circuit rows: ") + why);
  return LCP2_OK;
}

// The expansion, arguments checked; out: device, [num_constants + num_routed_wires][n].  The work area is scratch slot 2:
//   gate table and coset shifts | gate_of_row | row_constants | bound bitmap | twice bitmap | any_twice, the two indices of a double
//   binding | keys | keys (the other side of the sort) | digit counts [16][tiles]
int rows_expand(lcp2_ctx *ctx, const lcp2_circuit_desc *d, const lcp2_circuit_rows *r, u64 *out) {
  static_assert(sizeof(lcp2_copy_binding) == sizeof(BindingDev) && sizeof(GateSelDev) == 8, "ABI structs must match the kernels'");
  const lcp2_params &p = d->params;
  const u64 n = 1ull << p.degree_bits, cells = (u64)p.num_routed_wires * n, M = r->num_bindings;
  const u32 NC = p.num_constants, NR = p.num_routed_wires, S = d->num_selectors, K = NC - S, NG = d->num_gates;
  const u64 num_rows = r->num_rows;
  const bool with_constants = r->row_constants && num_rows && K;
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const u32 tiles = (u32)((M + ROWS_TILE - 1) / ROWS_TILE), passes = M ? rows_passes(r->num_classes) : 0;
  const size_t small_bytes = up256((size_t)(NG + NR) * 8), gor_bytes = up256((size_t)num_rows * 4), rc_bytes = with_constants ? up256((size_t)num_rows * K * 8) : 0;
  const size_t map_bytes = up256((size_t)((cells + 31) / 32) * 4), res_bytes = 256, key_bytes = up256((size_t)M * 8);
  const size_t table_bytes = up256((size_t)ROWS_DIGITS * tiles * 4);
  char *base;
  LCP2_TRY(scratch_ensure(ctx, 2, small_bytes + gor_bytes + rc_bytes + 2 * map_bytes + res_bytes + 2 * key_bytes + table_bytes, (void **)&base));
  char *at = base;
  auto take = [&](size_t bytes) { char *q = at; at += bytes; return q; };
  GateSelDev *d_gates = (GateSelDev *)take(small_bytes);
  const u64 *d_kis = (const u64 *)d_gates + NG;
  u32 *d_gor = (u32 *)take(gor_bytes);
  u64 *d_rc = with_constants ? (u64 *)take(rc_bytes) : nullptr;
  u32 *d_bound = (u32 *)take(map_bytes), *d_twice = (u32 *)take(map_bytes);
  u64 *d_res = (u64 *)take(res_bytes);  // [0], [1]: the two list indices of a double binding; [2]: any_twice
  u64 *d_keys[2];
  d_keys[0] = (u64 *)take(key_bytes); d_keys[1] = (u64 *)take(key_bytes);
  u32 *d_table = (u32 *)take(table_bytes);
  {  // host lists, each through the whole pinned buffer (the caller's arrays are his again when the call returns)
    std::vector<u64> small((size_t)NG + NR);
    for (u32 g = 0; g < NG; g++) small[g] = (u64)d->gates[g].selector_index | (u64)d->gates[g].selector_value << 32;
    for (u32 j = 0; j < NR; j++) small[NG + j] = gl_canon(d->k_is[j]);
    Stage st{ctx};
    LCP2_TRY(st.whole(d_gates, small.data(), small.size() * 8));
    if (num_rows) LCP2_TRY(st.whole(d_gor, r->gate_of_row, (size_t)num_rows * 4));
    if (with_constants) LCP2_TRY(st.whole(d_rc, r->row_constants, (size_t)num_rows * K * 8));
  }
  const BindingDev *list = (const BindingDev *)r->bindings;
  if (M && r->bindings_mem == LCP2_MEM_HOST) {
    void *up;
    LCP2_TRY(scratch_ensure(ctx, 3, (size_t)M * sizeof(BindingDev), &up));
    LCP2_TRY(Stage{ctx}.whole(up, r->bindings, (size_t)M * sizeof(BindingDev)));
    list = (const BindingDev *)up;
  }
  DeviceNttBackend be{ctx};
  NttHost<DeviceNttBackend> ntt(be);
  const TwoLevelTable roots = ntt.root_table(p.degree_bits, false);  // w^row from the transforms' two power tables: no exponentiation per lane
  if (be.status) return be.status;
  RefusalFlag flag{ctx};
  flag.nwords = 2;  // [0]: the list, [1]: gate_of_row
  LCP2_TRY(flag.begin());
  RowsShape sh{n, num_rows, S, K, NG, r->pad_gate, NR, r->num_classes};
  const unsigned row_blocks = (unsigned)((n + ROWS_THREADS - 1) / ROWS_THREADS), list_blocks = (unsigned)((M + ROWS_THREADS - 1) / ROWS_THREADS);
  u64 *sigmas = out + (u64)NC * n;
  {  // (a)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)NC * n * 8.0 + (double)num_rows * (4.0 + (with_constants ? K * 8.0 : 0.0)));
    hipLaunchKernelGGL(k_rows_constants, dim3(row_blocks, NC), dim3(ROWS_THREADS), 0, s, d_gates, d_gor, d_rc, sh, out, flag.d + 1);
  }
  {  // (b)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)cells * 8.0);
    hipLaunchKernelGGL(k_rows_identity, dim3(row_blocks, (NR + ROWS_ID_WIRES - 1) / ROWS_ID_WIRES), dim3(ROWS_THREADS), 0, s, d_kis, roots, n, NR, sigmas);
  }
  u64 twice_words[3] = {0, 0, 0};
  Download dl(ctx);
  if (M) {  // (c)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)M * 20.0 + (double)map_bytes * 2.0);
    LCP2_HIP(ctx, hipMemsetAsync(d_bound, 0, 2 * map_bytes, s));
    {
      SmallWords w{};
      w.v[0] = ~0ull; w.v[1] = ~0ull;
      launch_set_words(s, d_res, w, 3);
    }
    hipLaunchKernelGGL(k_rows_keys, dim3(list_blocks), dim3(ROWS_THREADS), 0, s, list, M, sh, d_keys[0], d_bound, d_twice, (u32 *)(d_res + 2), flag.d);
    LCP2_TRY(dl.add(twice_words, d_res, sizeof twice_words));
  }
  LCP2_TRY(flag.read());  // before an entry is followed to its cell: every index must be in range, every cell bound once
  LCP2_TRY(dl.wait());
  if (flag.words[1] != ROW_NO_PROBLEM)
    return ctx->fail(LCP2_E_INVALID, "circuit rows: row " + std::to_string(flag.words[1] >> 8) + ": " + rows_problem_str((u32)(flag.words[1] & 0xFF)));
  if (flag.words[0] != ROW_NO_PROBLEM)
    return ctx->fail(LCP2_E_INVALID, "circuit rows: binding " + std::to_string(flag.words[0] >> 8) + ": " + rows_problem_str((u32)(flag.words[0] & 0xFF)));
  if (twice_words[2]) {
    hipLaunchKernelGGL(k_rows_twice_first, dim3(list_blocks), dim3(ROWS_THREADS), 0, s, list, M, sh, d_twice, d_res);
    hipLaunchKernelGGL(k_rows_twice_second, dim3(list_blocks), dim3(ROWS_THREADS), 0, s, list, M, d_res);
    LCP2_HIP(ctx, hipGetLastError());
    LCP2_TRY(download(ctx, twice_words, d_res, 16));
    BindingDev b{};
    if (twice_words[0] < M) LCP2_TRY(download(ctx, &b, list + twice_words[0], sizeof b));
    return ctx->fail(LCP2_E_INVALID, "circuit rows: binding " + std::to_string(twice_words[1]) + ": " + rows_problem_str(ROWS_BIND_TWICE) + " (row " + std::to_string(b.row) +
                                         ", wire " + std::to_string(b.col) + "), also bound by binding " + std::to_string(twice_words[0]));
  }
  u32 side = 0;
  for (u32 pass = 0; pass < passes; pass++, side ^= 1) {  // (d)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)M * 32.0);
    hipLaunchKernelGGL(k_rows_hist, dim3(tiles), dim3(ROWS_THREADS), 0, s, d_keys[side], M, pass, tiles, d_table);
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(1024), 0, s, d_table, ROWS_DIGITS * tiles);
    hipLaunchKernelGGL(k_rows_scatter, dim3(tiles), dim3(ROWS_THREADS), 0, s, d_keys[side], M, pass, tiles, d_table, d_keys[side ^ 1]);
  }
  if (M) {  // (e)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)M * 48.0);
    hipLaunchKernelGGL(k_rows_cycles, dim3(list_blocks), dim3(ROWS_THREADS), 0, s, list, d_keys[side], M, d_kis, roots, n, sigmas);
  }
  LCP2_HIP(ctx, hipGetLastError());
  LCP2_HIP(ctx, hipStreamSynchronize(s));
  return LCP2_OK;
}
}  // namespace
}  // namespace lcp2

extern "C" int lcp2_circuit_rows_expand(lcp2_ctx *ctx, const lcp2_circuit_desc *desc, const lcp2_circuit_rows *rows, uint64_t *out) {
  if (!ctx || !desc || !rows || !out) return LCP2_E_INVALID;
  LCP2_TRY(rows_guard(ctx, desc, rows));
  const int rc = rows_expand(ctx, desc, rows, (u64 *)out);
  if (rc != LCP2_OK) (void)hipStreamSynchronize(ctx->stream);  // a failed call may have left an upload in flight
  return rc;
}

extern "C" int lcp2_circuit_create_from_rows(lcp2_ctx *ctx, const lcp2_circuit_desc *desc, const lcp2_circuit_rows *rows, lcp2_circuit **out) {
  if (!ctx || !desc || !rows || !out) return LCP2_E_INVALID;
  *out = nullptr;
  LCP2_TRY(rows_guard(ctx, desc, rows));
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  const lcp2_params &p = desc->params;
  void *matrix;
  LCP2_TRY(scratch_ensure(ctx, 0, ((size_t)(p.num_constants + p.num_routed_wires) << p.degree_bits) * 8, &matrix));
  const int rc = rows_expand(ctx, desc, rows, (u64 *)matrix);
  if (rc != LCP2_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  lcp2_circuit_desc expanded = *desc;
  expanded.constants_sigmas = (const uint64_t *)matrix;
  expanded.constants_sigmas_mem = LCP2_MEM_DEVICE;
  return lcp2_circuit_create(ctx, &expanded, out);
}
