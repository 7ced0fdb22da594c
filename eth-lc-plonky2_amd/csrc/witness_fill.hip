// lcp2_witness_fill_copies and lcp2_circuit_copy_classes: one value per copy class goes up, the device hands it to every routed cell
// of the class (plonky2: PartitionWitness::get_full_witness).  The per-cell texts are witness_fill.hpp (portable: tests/emu/emu_fill.cpp
// runs them on the CPU); here are the kernels, the one-time construction of the class table and the entry points - also
// lcp2_witness_settle_copies, the same call with the values read from the matrix (witness_settle.hpp, the k_settle_* kernels).  Nothing of the
// proving state of the handle is read or written: the table is a buffer of its own in the handle, everything else is scratch of
// the context.  All kernels are bandwidth bound: one lane per cell, rows in the fast dimension, so the loads of class_of / label and
// the stores into the matrix are contiguous; the gathers (label[ptr], rank[label], owner[class], the owner's list entry) are the
// data-dependent part and hit few distinct lines per wave in a circuit whose classes are short.
#include "circuit_state.hpp"
#include "row_stage.hpp"
#include "witness_fill.hpp"
#include "witness_settle.hpp"

using namespace lcp2;

namespace lcp2 {
constexpr u32 FILL_THREADS = 256;
constexpr u32 FILL_TILE = 2048;  // cells per block of the two root passes (8 steps of 256 lanes)
// the result block of a call (scratch slot 2, in front of owner[])
enum : u32 { FILL_R_CLASSES_SET = 0, FILL_R_FILLED, FILL_R_CONFLICTS, FILL_R_CONFLICT_INDEX, FILL_R_OWNER_INDEX, FILL_R_CONFLICT_CELL, FILL_R_OWNER_CELL, FILL_R_WORDS = 8 };

static __device__ __forceinline__ u32 fill_wave_sum(u32 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
static __device__ __forceinline__ u64 fill_wave_min(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}

// ---- the class table
// (a) one lane per routed cell, blockIdx.y = wire: the decode of its sigma value
__global__ __launch_bounds__(FILL_THREADS) void k_fill_next(const u64 *__restrict__ sigmas, const u64 *__restrict__ k_is, WcDecode t, u64 n,
                                                            u32 *__restrict__ next, u32 *inv, u64 *flag) {
  const u32 wire = blockIdx.y;
  const u64 row = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (row >= n) return;
  if (!fill_next_lane(t, sigmas, n, wire, row, gl_mul(k_is[wire], two_level(t.roots, row)), next, inv))
    atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal((u64)wire * n + row, FILL_SIGMA_NO_ID));
}
__global__ __launch_bounds__(FILL_THREADS) void k_fill_shared(const u32 *__restrict__ next, const u32 *__restrict__ inv, u64 cells, u64 *flag) {
  const u64 cell = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (cell < cells && fill_image_shared(next, inv, (u32)cell))
    atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(cell, FILL_SIGMA_SHARED));
}
// (b) one lane per cell, one launch per round; *changed is set when a label went down (a plain store from every such lane: they
// all store the same 1, and the host reads the word only after the launch)
__global__ __launch_bounds__(FILL_THREADS) void k_fill_jump_first(const u32 *__restrict__ next, u32 *__restrict__ label_out, u32 *__restrict__ ptr_out,
                                                                  u64 cells, u32 *changed) {
  const u64 cell = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (cell < cells && fill_jump_first(next, label_out, ptr_out, (u32)cell)) *changed = 1;
}
__global__ __launch_bounds__(FILL_THREADS) void k_fill_jump(const u32 *__restrict__ label_in, const u32 *__restrict__ ptr_in, u32 *__restrict__ label_out,
                                                            u32 *__restrict__ ptr_out, u64 cells, u32 *changed) {
  const u64 cell = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (cell < cells && fill_jump_cell(label_in, ptr_in, label_out, ptr_out, (u32)cell)) *changed = 1;
}
// (c) the roots below each root, in three launches: the roots of every tile, the tile sums scanned by one block, the ranks.
// flags of the block's 256 lanes in lane order -> how many are set below this lane, and in the whole block
static __device__ __forceinline__ u32 fill_block_prefix(bool flag, u32 *wave_total /* LDS, 4 words */, u32 *total) {
  const u64 mask = __ballot(flag);
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 before = (u32)__popcll(mask & ((1ull << lane) - 1));
  __syncthreads();  // the step before has read wave_total
  if (lane == 0) wave_total[wave] = (u32)__popcll(mask);
  __syncthreads();
  u32 below = 0, all = 0;
#pragma unroll
  for (u32 k = 0; k < FILL_THREADS / 64; k++) { const u32 v = wave_total[k]; all += v; if (k < wave) below += v; }
  *total = all;
  return below + before;
}
// rank == nullptr: sums[block] = the roots of the block's tile; else sums holds the roots below each tile and rank[root] is written
__global__ __launch_bounds__(FILL_THREADS) void k_fill_roots(const u32 *__restrict__ label, const u32 *__restrict__ next, u64 cells, u32 *sums, u32 *rank) {
  __shared__ u32 wave_total[FILL_THREADS / 64];
  const u64 base = (u64)blockIdx.x * FILL_TILE;
  u32 running = rank ? sums[blockIdx.x] : 0;
  for (u32 k = 0; k < FILL_TILE / FILL_THREADS; k++) {  // every lane takes every step: the barriers are uniform
    const u64 cell = base + (u64)k * FILL_THREADS + threadIdx.x;
    const bool root = cell < cells && fill_is_root(label, next, (u32)cell);
    u32 total;
    const u32 before = fill_block_prefix(root, wave_total, &total);
    if (rank && root) rank[cell] = running + before;
    running += total;
  }
  if (!rank && threadIdx.x == 0) sums[blockIdx.x] = running;
}
// one block: sums[0 .. count) -> the sums in front of each, in place; *total = all of them
__global__ __launch_bounds__(1024) void k_fill_scan_sums(u32 *sums, u32 count, u64 *total) {
  __shared__ u32 part[1024];
  const u32 t = threadIdx.x, piece = (count + 1023) / 1024;
  const u32 a = t * piece < count ? t * piece : count, b = a + piece < count ? a + piece : count;
  u32 mine = 0;
  for (u32 i = a; i < b; i++) mine += sums[i];
  part[t] = mine;
  __syncthreads();
  for (u32 off = 1; off < 1024; off <<= 1) {
    const u32 v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  u32 running = part[t] - mine;
  for (u32 i = a; i < b; i++) { const u32 v = sums[i]; sums[i] = running; running += v; }
  if (t == 1023) *total = part[1023];
}
// class_of written over next, each lane its own word
__global__ __launch_bounds__(FILL_THREADS) void k_fill_number(const u32 *__restrict__ label, const u32 *__restrict__ rank, u32 *class_of, u64 cells) {
  const u64 cell = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (cell < cells) fill_number_cell(label, rank, class_of, class_of, (u32)cell);
}

// ---- a call
// one lane per listed entry: validation, the plain store, the minimum on the class's owner word, the mark
__global__ __launch_bounds__(FILL_THREADS) void k_fill_owner(const CellDev *__restrict__ cells, u64 ncells, u32 *class_of, u32 *owner, u64 *wires, u64 n,
                                                             u32 num_wires, u32 num_routed, u64 *flag) {
  const u64 i = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (const u32 problem = fill_owner_lane(cells, ncells, i, class_of, owner, wires, n, num_wires, num_routed))
    atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(i, problem));
}
// one lane per routed cell (cell = wire * n + row is also its word in the matrix: the routed wires are the first columns)
__global__ __launch_bounds__(FILL_THREADS) void k_fill_broadcast(const CellDev *__restrict__ cells, u32 *class_of, const u32 *__restrict__ owner, u64 *wires,
                                                                 u64 ncells_routed, u64 *res) {
  const u64 cell = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  const u32 filled = cell < ncells_routed ? fill_broadcast_cell(cells, class_of, owner, wires, (u32)cell) : 0;
  const u32 sum = fill_wave_sum(filled);
  if (sum && (threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&res[FILL_R_FILLED], (unsigned long long)sum);
}
// one lane per listed entry, after the owners are known: the owned classes and the conflicts
__global__ __launch_bounds__(FILL_THREADS) void k_fill_conflicts(const CellDev *__restrict__ cells, u64 ncells, const u32 *__restrict__ class_of,
                                                                 const u32 *__restrict__ owner, u64 n, u32 num_wires, u32 num_routed, u64 *res) {
  const u64 i = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  const u32 what = fill_conflict_lane(cells, ncells, i, class_of, owner, n, num_wires, num_routed);
  const u32 owners = fill_wave_sum(what == FILL_IS_OWNER ? 1u : 0u), conflicts = fill_wave_sum(what == FILL_CONFLICT ? 1u : 0u);
  const bool lead = (threadIdx.x & 63) == 0;
  if (owners && lead) atomicAdd((unsigned long long *)&res[FILL_R_CLASSES_SET], (unsigned long long)owners);
  if (conflicts) {  // wave-uniform
    const u64 first = fill_wave_min(what == FILL_CONFLICT ? i : ~0ull);
    if (lead) {
      atomicAdd((unsigned long long *)&res[FILL_R_CONFLICTS], (unsigned long long)conflicts);
      atomicMin((unsigned long long *)&res[FILL_R_CONFLICT_INDEX], (unsigned long long)first);
    }
  }
}
// the first conflict for the message: its owner's list index and both cells (row | col << 32), with the counts in the one download
__global__ void k_fill_first_conflict(const CellDev *__restrict__ cells, const u32 *__restrict__ class_of, const u32 *__restrict__ owner, u64 n,
                                      u32 num_routed, u64 *res) {
  const u64 i = res[FILL_R_CONFLICT_INDEX];
  if (i == ~0ull) return;
  const CellDev c = cells[i];
  const u32 o = owner[fill_class_of_listed(c, class_of, n, num_routed)];
  const CellDev oc = cells[o];
  res[FILL_R_OWNER_INDEX] = o;
  res[FILL_R_CONFLICT_CELL] = (u64)c.row | (u64)c.col << 32;
  res[FILL_R_OWNER_CELL] = (u64)oc.row | (u64)oc.col << 32;
}

// ---- lcp2_witness_settle_copies: the same call with the values read from the matrix (witness_settle.hpp, where the order of the
// passes is argued: owner, then conflicts, then the broadcast, which alone stores to the matrix and reads only owner cells, which it
// never stores to).  One launch each, on one stream, so each pass sees the one before complete.
// one lane per source: validation, the minimum on the class's owner word, the mark.  No access to the matrix
__global__ __launch_bounds__(FILL_THREADS) void k_settle_owner(const CellRefDev *__restrict__ refs, u64 nsources, u32 *class_of, u32 *owner, u64 n, u32 num_wires,
                                                               u32 num_routed, u64 *flag) {
  const u64 i = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  if (const u32 problem = settle_owner_lane(refs, nsources, i, class_of, owner, n, num_wires, num_routed))
    atomicMin((unsigned long long *)flag, (unsigned long long)row_refusal(i, problem));
}
// one lane per source, after the owners are known and before any word of the matrix changes: the owned classes and the conflicts
__global__ __launch_bounds__(FILL_THREADS) void k_settle_conflicts(const CellRefDev *__restrict__ refs, u64 nsources, const u32 *__restrict__ class_of,
                                                                   const u32 *__restrict__ owner, const u64 *__restrict__ wires, u64 n, u32 num_wires,
                                                                   u32 num_routed, u64 *res) {
  const u64 i = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  const u32 what = settle_conflict_lane(refs, nsources, i, class_of, owner, wires, n, num_wires, num_routed);
  const u32 owners = fill_wave_sum(what == FILL_IS_OWNER ? 1u : 0u), conflicts = fill_wave_sum(what == FILL_CONFLICT ? 1u : 0u);
  const bool lead = (threadIdx.x & 63) == 0;
  if (owners && lead) atomicAdd((unsigned long long *)&res[FILL_R_CLASSES_SET], (unsigned long long)owners);
  if (conflicts) {  // wave-uniform
    const u64 first = fill_wave_min(what == FILL_CONFLICT ? i : ~0ull);
    if (lead) {
      atomicAdd((unsigned long long *)&res[FILL_R_CONFLICTS], (unsigned long long)conflicts);
      atomicMin((unsigned long long *)&res[FILL_R_CONFLICT_INDEX], (unsigned long long)first);
    }
  }
}
// one lane per routed cell: class_of streams along rows, owner[class] -> the source -> the word at its cell are dependent gathers,
// the store is along rows.  wires is read and written here, so it carries no __restrict__ (the lanes' reads and writes are disjoint
// words all the same, witness_settle.hpp)
__global__ __launch_bounds__(FILL_THREADS) void k_settle_broadcast(const CellRefDev *__restrict__ refs, u32 *class_of, const u32 *__restrict__ owner, u64 *wires,
                                                                   u64 n, u64 ncells_routed, u64 *res) {
  const u64 cell = (u64)blockIdx.x * FILL_THREADS + threadIdx.x;
  const u32 filled = cell < ncells_routed ? settle_broadcast_cell(refs, class_of, owner, wires, n, (u32)cell) : 0;
  const u32 sum = fill_wave_sum(filled);
  if (sum && (threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&res[FILL_R_FILLED], (unsigned long long)sum);
}
// k_fill_first_conflict for a list of sources
__global__ void k_settle_first_conflict(const CellRefDev *__restrict__ refs, const u32 *__restrict__ class_of, const u32 *__restrict__ owner, u64 n,
                                        u32 num_routed, u64 *res) {
  const u64 i = res[FILL_R_CONFLICT_INDEX];
  if (i == ~0ull) return;
  const CellRefDev c = refs[i];
  const u32 o = owner[settle_class_of_source(c, class_of, n, num_routed)];
  const CellRefDev oc = refs[o];
  res[FILL_R_OWNER_INDEX] = o;
  res[FILL_R_CONFLICT_CELL] = (u64)c.row | (u64)c.col << 32;
  res[FILL_R_OWNER_CELL] = (u64)oc.row | (u64)oc.col << 32;
}

namespace {
std::string cell_name(u64 cell, u64 n) { return "(row " + std::to_string(cell % n) + ", wire " + std::to_string(cell / n) + ")"; }

// what both entry points refuse after the handle itself: LCP2_OK or the status, the reason in lcp2_last_error
int fill_guard(lcp2_circuit *c, const char *who) {
  lcp2_ctx *ctx = c->ctx;
  if (c->sharded()) return ctx->fail(LCP2_E_UNSUPPORTED, std::string(who) + ": a sharded circuit holds only its own blocks");
  if ((u64)c->p.num_routed_wires << c->p.degree_bits >= FILL_MAX_CELLS)
    return ctx->fail(LCP2_E_UNSUPPORTED, std::string(who) + ": 2^32 routed cells or more (cell indices are 32-bit)");
  return LCP2_OK;
}

// The class table of the handle, built at the first call.  The table is NOT constant afterwards: a call keeps the marks of its
// listed cells in it between its owner pass and its broadcast (witness_fill.hpp), which spares a bitmap of a bit per routed cell
// that would have to be cleared per call.  The price: one call at a time per handle (a handle belongs to one context and its one
// stream anyway), and a call that fails between the two passes leaves marks behind, so it drops the table and the next call
// builds it again (copy_classes_ready).  Scratch slot 0 (kept by the context like all scratch) holds the two (label, ptr) pairs of the jumping rounds - inv
// lives in the second label array until the first round has run, rank in the ptr array beside the final labels - then the tile
// sums, their total and one `changed` word per round; slot 1 the refusal flag of the sigma columns.
int copy_classes_ensure(lcp2_circuit *c, StageEnv &e) {
  if (c->copy_classes_ready) return LCP2_OK;
  lcp2_ctx *ctx = c->ctx;
  hipStream_t s = e.s;
  const u64 n = e.n, cells = (u64)e.NR * n;
  const u32 tiles = (u32)((cells + FILL_TILE - 1) / FILL_TILE), blocks = (u32)((cells + FILL_THREADS - 1) / FILL_THREADS);
  const size_t plane = ((size_t)cells * 4 + 255) & ~(size_t)255, sums_bytes = ((size_t)tiles * 4 + 255) & ~(size_t)255;
  char *base;
  LCP2_TRY(scratch_ensure(ctx, 0, 4 * plane + sums_bytes + 8 + FILL_MAX_ROUNDS * 4, (void **)&base));
  u32 *label[2] = {(u32 *)base, (u32 *)(base + 2 * plane)}, *ptr[2] = {(u32 *)(base + plane), (u32 *)(base + 3 * plane)};
  u32 *sums = (u32 *)(base + 4 * plane);
  u64 *total = (u64 *)(base + 4 * plane + sums_bytes);
  u32 *changed = (u32 *)(total + 1);
  LCP2_HIP(ctx, c->copy_class_of.ensure((size_t)cells * 4));
  u32 *next = (u32 *)c->copy_class_of.p, *inv = label[1];
  WcDecode t{};
  LCP2_TRY(wc_device_decode(c, e, &t));
  RefusalFlag flag{ctx};
  LCP2_TRY(flag.begin());
  {  // (a)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)cells * 20.0);
    LCP2_HIP(ctx, hipMemsetAsync(inv, 0xFF, (size_t)cells * 4, s));
    LCP2_HIP(ctx, hipMemsetAsync(changed, 0, FILL_MAX_ROUNDS * 4, s));
    hipLaunchKernelGGL(k_fill_next, dim3((unsigned)((n + FILL_THREADS - 1) / FILL_THREADS), e.NR), dim3(FILL_THREADS), 0, s,
                       c->cs_values.u() + (u64)e.NC * n, c->d_kis.u(), t, n, next, inv, flag.d);
    hipLaunchKernelGGL(k_fill_shared, dim3(blocks), dim3(FILL_THREADS), 0, s, next, inv, cells, flag.d);
  }
  LCP2_TRY(flag.read());  // before a round follows a pointer: next must be a permutation
  if (flag.words[0] != ROW_NO_PROBLEM) {
    const u64 cell = flag.words[0] >> 8;
    std::string why = "fill copies: the sigma columns are no permutation of the routed cells: ";
    if ((flag.words[0] & 0xFF) == FILL_SIGMA_NO_ID) {
      why += "the value at " + cell_name(cell, n) + " is the id of no cell";
    } else {
      u32 image = 0, other = 0;
      LCP2_TRY(download(ctx, &image, next + cell, 4));
      LCP2_TRY(download(ctx, &other, inv + image, 4));
      why += cell_name(other, n) + " and " + cell_name(cell, n) + " have the same image " + cell_name(image, n);
    }
    c->copy_class_of.release();
    return ctx->fail(LCP2_E_INVALID, why);
  }
  // (b) the last round's output holds the labels, whether it lowered one or not
  u32 rounds = 0, last = 0;
  for (u32 r = 0; r < FILL_MAX_ROUNDS; r++) {
    last = r & 1;
    {
      ProfScope ps(ctx, LCP2_K_OTHER, (double)cells * (r ? 24.0 : 16.0));
      if (r == 0) hipLaunchKernelGGL(k_fill_jump_first, dim3(blocks), dim3(FILL_THREADS), 0, s, next, label[0], ptr[0], cells, changed);
      else hipLaunchKernelGGL(k_fill_jump, dim3(blocks), dim3(FILL_THREADS), 0, s, label[last ^ 1], ptr[last ^ 1], label[last], ptr[last], cells, changed + r);
    }
    LCP2_HIP(ctx, hipGetLastError());
    u32 went_down = 0;
    LCP2_TRY(download(ctx, &went_down, changed + r, 4));
    if (!went_down) break;
    rounds++;
  }
  {  // (c)
    ProfScope ps(ctx, LCP2_K_OTHER, (double)cells * 20.0);
    u32 *rank = ptr[last];
    hipLaunchKernelGGL(k_fill_roots, dim3(tiles), dim3(FILL_THREADS), 0, s, label[last], next, cells, sums, (u32 *)nullptr);
    hipLaunchKernelGGL(k_fill_scan_sums, dim3(1), dim3(1024), 0, s, sums, tiles, total);
    hipLaunchKernelGGL(k_fill_roots, dim3(tiles), dim3(FILL_THREADS), 0, s, label[last], next, cells, sums, rank);
    hipLaunchKernelGGL(k_fill_number, dim3(blocks), dim3(FILL_THREADS), 0, s, label[last], rank, next, cells);
  }
  LCP2_HIP(ctx, hipGetLastError());
  u64 num_classes = 0;
  LCP2_TRY(download(ctx, &num_classes, total, 8));
  c->copy_num_classes = num_classes;
  c->copy_rounds = rounds;
  c->copy_classes_ready = true;
  return LCP2_OK;
}
}  // namespace
}  // namespace lcp2

extern "C" int lcp2_circuit_copy_classes(lcp2_circuit *c, uint32_t *class_of, uint64_t *num_classes) {
  LCP2_TRY(entry_guard(c));
  LCP2_TRY(fill_guard(c, "copy classes"));
  StageEnv e(c);
  LCP2_TRY(e.status);
  LCP2_TRY(copy_classes_ensure(c, e));
  if (num_classes) *num_classes = c->copy_num_classes;
  if (class_of) LCP2_TRY(download(c->ctx, class_of, c->copy_class_of.p, (size_t)e.NR * e.n * 4));
  else LCP2_HIP(c->ctx, hipStreamSynchronize(e.s));
  return LCP2_OK;
}

namespace {
// What lcp2_witness_fill_copies (Entry = CellDev: the values are in the list) and lcp2_witness_settle_copies (Entry = CellRefDev: the
// values are in the matrix) share: the argument checks, the host validation and the staging of a host list, the table, the cleared
// result block and owner words, the marks' bracket around the passes, the one download and the messages.  `passes` launches the
// call's kernels in ITS order; list_bytes is what the profile books per entry, device_note what a refused device entry left done.
template <class Entry, class Passes>
int copies_call(lcp2_circuit *c, const std::string &who, const Entry *list, size_t count, lcp2_mem mem, uint64_t *wires, lcp2_fill_report *report, double list_bytes,
                const char *device_note, Passes passes) {
  LCP2_TRY(entry_guard(c, {wires}));
  lcp2_ctx *ctx = c->ctx;
  if ((unsigned)mem > 1) return ctx->fail(LCP2_E_INVALID, who + ": bad lcp2_mem");
  if (count && !list) return ctx->fail(LCP2_E_INVALID, who + ": the list is null but its count is not zero");
  LCP2_TRY(fill_guard(c, who.c_str()));
  if ((u64)count >= FILL_MAX_CELLS) return ctx->fail(LCP2_E_UNSUPPORTED, who + ": 2^32 listed cells or more (list indices are 32-bit)");
  lcp2_fill_report out{};
  out.conflict_index = ~0ull; out.owner_index = ~0ull;
  if (!count) {
    if (report) *report = out;
    return LCP2_OK;
  }
  const u64 n = 1ull << c->p.degree_bits;
  const u32 W = c->p.num_wires, NR = c->p.num_routed_wires;
  if (mem == LCP2_MEM_HOST) {
    u32 problem = 0;
    if (const size_t at = fill_cells_problem(list, count, n, W, &problem); at != count)
      return ctx->fail(LCP2_E_INVALID, who + ": cell " + std::to_string(at) + ": " + fill_cell_problem_str(problem));
  }
  StageEnv e(c);
  LCP2_TRY(e.status);
  hipStream_t s = e.s;
  LCP2_TRY(copy_classes_ensure(c, e));
  const u64 routed = (u64)NR * n, num_classes = c->copy_num_classes;
  if (mem == LCP2_MEM_HOST) {
    void *up;
    LCP2_TRY(scratch_ensure(ctx, 3, count * sizeof(Entry), &up));
    LCP2_TRY(Stage{ctx}.behind(up, list, count * sizeof(Entry)));
    list = (const Entry *)up;
  }
  u64 *res;
  LCP2_TRY(scratch_ensure(ctx, 2, FILL_R_WORDS * 8 + (size_t)num_classes * 4, (void **)&res));
  u32 *owner = (u32 *)(res + FILL_R_WORDS), *class_of = (u32 *)c->copy_class_of.p;
  RefusalFlag flag{ctx};
  LCP2_TRY(flag.begin());
  {
    SmallWords w{};
    w.v[FILL_R_CONFLICT_INDEX] = ~0ull; w.v[FILL_R_OWNER_INDEX] = ~0ull;
    launch_set_words(s, res, w, FILL_R_WORDS);
    if (num_classes) LCP2_HIP(ctx, hipMemsetAsync(owner, 0xFF, (size_t)num_classes * 4, s));  // FILL_NONE
  }
  c->copy_classes_ready = false;  // the marks of the listed cells are in the table until the broadcast has taken them off
  {
    ProfScope ps(ctx, LCP2_K_OTHER, (double)count * list_bytes + (double)routed * 4.0);
    passes(s, list, (u64)count, dim3((unsigned)((count + FILL_THREADS - 1) / FILL_THREADS)), dim3((unsigned)((routed + FILL_THREADS - 1) / FILL_THREADS)), class_of,
           owner, n, W, NR, routed, flag.d, res);
  }
  u64 r[FILL_R_WORDS];
  Download dl(ctx);
  LCP2_TRY(dl.add(r, res, sizeof r));
  LCP2_TRY(flag.read());  // the stream is waited for: the caller's list may go, every cell is written
  LCP2_TRY(dl.wait());
  c->copy_classes_ready = true;
  out.num_classes = num_classes;
  out.classes_set = r[FILL_R_CLASSES_SET];
  out.cells_filled = r[FILL_R_FILLED];
  out.conflicts = r[FILL_R_CONFLICTS];
  out.conflict_index = r[FILL_R_CONFLICT_INDEX];
  out.owner_index = r[FILL_R_OWNER_INDEX];
  if (report) *report = out;
  if (flag.words[0] != ROW_NO_PROBLEM)
    return ctx->fail(LCP2_E_INVALID, who + ": cell " + std::to_string(flag.words[0] >> 8) + ": " + fill_cell_problem_str((u32)(flag.words[0] & 0xFF)) + device_note);
  if (out.conflicts) {
    auto cell = [](u64 packed) { return "(row " + std::to_string(packed & 0xFFFFFFFFull) + ", wire " + std::to_string(packed >> 32) + ")"; };
    return ctx->fail(LCP2_E_UNSAT, who + ": cell " + std::to_string(out.conflict_index) + " " + cell(r[FILL_R_CONFLICT_CELL]) +
                                       " differs from cell " + std::to_string(out.owner_index) + " " + cell(r[FILL_R_OWNER_CELL]) +
                                       ", which gave their copy class its value (" + std::to_string(out.conflicts) + " such cells; the class holds the owner's value)");
  }
  return LCP2_OK;
}
}  // namespace

extern "C" int lcp2_witness_fill_copies(lcp2_circuit *c, const lcp2_cell *cells, size_t ncells, lcp2_mem cells_mem, uint64_t *wires,
                                        lcp2_fill_report *report) {
  static_assert(sizeof(lcp2_cell) == sizeof(CellDev), "ABI structs must match the kernels'");
  u64 *w = (u64 *)wires;
  return copies_call(c, "fill copies", (const CellDev *)cells, ncells, cells_mem, wires, report, 40.0,
                     " (found on the device: the valid cells are written and their classes filled)",
                     [w](hipStream_t s, const CellDev *list, u64 count, dim3 list_blocks, dim3 cell_blocks, u32 *class_of, u32 *owner, u64 n, u32 W, u32 NR, u64 routed,
                         u64 *flag, u64 *res) {
                       hipLaunchKernelGGL(k_fill_owner, list_blocks, dim3(FILL_THREADS), 0, s, list, count, class_of, owner, w, n, W, NR, flag);
                       hipLaunchKernelGGL(k_fill_broadcast, cell_blocks, dim3(FILL_THREADS), 0, s, list, class_of, owner, w, routed, res);
                       hipLaunchKernelGGL(k_fill_conflicts, list_blocks, dim3(FILL_THREADS), 0, s, list, count, class_of, owner, n, W, NR, res);
                       hipLaunchKernelGGL(k_fill_first_conflict, dim3(1), dim3(1), 0, s, list, class_of, owner, n, NR, res);
                     });
}

// the order is the point: the matrix is compared before it is written, and written from words that are not (witness_settle.hpp)
extern "C" int lcp2_witness_settle_copies(lcp2_circuit *c, const lcp2_cell_ref *sources, size_t nsources, lcp2_mem sources_mem, uint64_t *wires,
                                          lcp2_fill_report *report) {
  static_assert(sizeof(lcp2_cell_ref) == sizeof(CellRefDev), "ABI structs must match the kernels'");
  u64 *w = (u64 *)wires;
  return copies_call(c, "settle copies", (const CellRefDev *)sources, nsources, sources_mem, wires, report, 48.0,
                     " (found on the device: the classes of the valid cells are filled)",
                     [w](hipStream_t s, const CellRefDev *list, u64 count, dim3 list_blocks, dim3 cell_blocks, u32 *class_of, u32 *owner, u64 n, u32 W, u32 NR,
                         u64 routed, u64 *flag, u64 *res) {
                       hipLaunchKernelGGL(k_settle_owner, list_blocks, dim3(FILL_THREADS), 0, s, list, count, class_of, owner, n, W, NR, flag);
                       hipLaunchKernelGGL(k_settle_conflicts, list_blocks, dim3(FILL_THREADS), 0, s, list, count, class_of, owner, (const u64 *)w, n, W, NR, res);
                       hipLaunchKernelGGL(k_settle_first_conflict, dim3(1), dim3(1), 0, s, list, class_of, owner, n, NR, res);
                       hipLaunchKernelGGL(k_settle_broadcast, cell_blocks, dim3(FILL_THREADS), 0, s, list, class_of, owner, w, n, routed, res);
                     });
}
