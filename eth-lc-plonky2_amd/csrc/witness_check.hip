// lcp2_check_witness: WHERE a witness violates the circuit - every unfiltered constraint of every row's own gate, and every routed
// cell against the cell its sigma value names - counted exactly, with the first violation of either kind named.  The per-row and
// per-cell texts are witness_check.hpp (portable: tests/emu/emu_check.cpp runs them on the CPU); here are the two kernels, their
// memory for the gate-program walk, and the entry point.  Nothing of the proving state of the handle is read or written: the
// results live in scratch of the context, a host witness is uploaded into scratch, a device witness is read in place.
#include "circuit_state.hpp"
#include "host_protocol.hpp"
#include "quotient_common.hpp"
#include "witness_check.hpp"

using namespace lcp2;

namespace lcp2 {
// the result block (scratch slot 1): these words, then one counter per gate
enum : u32 { WC_R_GATE_COUNT = 0, WC_R_GATE_KEY, WC_R_COPY_COUNT, WC_R_COPY_KEY, WC_R_NONCANON, WC_R_PI /* 4 words */, WC_R_COPY_SIGMA = 9, WC_R_WORDS = 16 };

static __device__ __forceinline__ u32 wc_wave_sum(u32 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
static __device__ __forceinline__ u64 wc_wave_min(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}

#if defined(__HIP_DEVICE_COMPILE__)
// the memory of wc_walk on the device: registers and staging slots in LDS (reg r of thread t at lds[r * T + t], as in q_interpret),
// columns from the witness / constants VALUES on H at this lane's row, canonicalised where they are read
struct WcDevMem {
  const QuotientArgs &a;
  u64 *lds;
  u32 T, tid;
  u64 i;
  __device__ __forceinline__ u64 insn(u32 pc) const { return konst((const u64 *)a.code)[pc]; }
  __device__ __forceinline__ void stage(u32 cnt, u32 off) {  // all loads issued before the first is used (q_stage)
    const_as<u32> lst = konst(a.stage_list) + off;
    u64 v[QUOTIENT_STAGE];
#pragma unroll
    for (u32 j = 0; j < QUOTIENT_STAGE; j++) {
      const u32 e = lst[j < cnt ? j : 0];
      const u64 *col = e < a.num_wires ? a.wires + (u64)e * a.stride : a.consts + (u64)(e - a.num_wires) * a.stride;
      v[j] = col[i];
    }
#pragma unroll
    for (u32 j = 0; j < QUOTIENT_STAGE; j++)
      if (j < cnt) lds[(a.num_regs + j) * T + tid] = gl_canon(v[j]);
  }
  __device__ __forceinline__ u64 operand(u32 kind, u32 idx) const {
    switch (kind) {
      case 0: return lds[idx * T + tid];
      case 1: return gl_canon(a.wires[(u64)idx * a.stride + i]);
      case 2: return gl_canon(a.consts[(u64)(a.num_selectors + idx) * a.stride + i]);
      case 3: return konst(a.imm)[idx];
      case 4: return a.pis[idx];  // written by the launch before this one: not through the constant address space
      default: return lds[(a.num_regs + idx) * T + tid];  // QKIND_STAGE
    }
  }
  __device__ __forceinline__ u64 reg(u32 r) const { return lds[r * T + tid]; }
  __device__ __forceinline__ void set_reg(u32 r, u64 v) { lds[r * T + tid] = v; }
  __device__ __forceinline__ void pmds(u32 dst, u32 src, u32 imm_offset) { q_pmds(lds, T, tid, dst, src, konst(a.imm) + imm_offset); }
  __device__ __forceinline__ u64 sbox(u64 x) const { return q_sbox(x); }
};
#endif

// One lane per row of H.  A wave skips a gate none of its rows holds; the lanes past the last row repeat it, so that every lane
// votes, and are not counted.  res: the result block; per_gate: nullable.
__global__ __launch_bounds__(128) void k_witness_gates(QuotientArgs a, u64 *res, u64 *per_gate) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ u64 lds[];
  const u32 T = blockDim.x, tid = threadIdx.x, lane = tid & 63;
  const u64 i0 = (u64)blockIdx.x * T + tid;
  const bool live = i0 < a.count;
  const u64 i = live ? i0 : a.count - 1;
  WcDevMem m{a, lds, T, tid, i};
  u32 count = 0;
  u64 key = WC_NONE;
  for (u32 g = 0; g < a.num_gates; g++) {
    const GateDev G = q_load_gate(a, g);
    if (G.num_constraints == 0) continue;
    const bool mine = gl_canon(a.consts[(u64)G.selector_index * a.stride + i]) == G.selector_value;
    if (!__any(mine)) continue;  // wave-uniform
    WcCount sink;
    sink.begin(G.num_constraints, G.flags);
    wc_walk(m, G.code_offset, G.code_len, sink);
    const u32 bad = mine && live ? sink.count : 0;
    if (bad) {
      count += bad;
      const u64 k = wc_gate_key(i, g, sink.first);
      key = k < key ? k : key;
    }
    if (per_gate) {
      const u32 sum = wc_wave_sum(bad);
      if (lane == 0 && sum) atomicAdd((unsigned long long *)&per_gate[g], (unsigned long long)sum);
    }
  }
  const u32 total = wc_wave_sum(count);
  const u64 first = wc_wave_min(key);
  if (lane == 0 && total) {
    atomicAdd((unsigned long long *)&res[WC_R_GATE_COUNT], (unsigned long long)total);
    atomicMin((unsigned long long *)&res[WC_R_GATE_KEY], (unsigned long long)first);
  }
#endif
}

// One lane per cell of the witness, rows in the fast dimension (blockIdx.y = wire): the words >= p of every column, and for a
// routed column the copy constraint of the cell.
__global__ __launch_bounds__(256) void k_witness_copies(const u64 *__restrict__ wires, const u64 *__restrict__ sigmas, const u64 *__restrict__ k_is,
                                                        WcDecode t, u64 n, u64 *res) {
  const u32 lane = threadIdx.x & 63, wire = blockIdx.y;
  const u64 row = (u64)blockIdx.x * 256 + threadIdx.x;
  bool bad = false, noncanonical = false;
  if (row < n) {
    noncanonical = wires[(u64)wire * n + row] >= GL_P;
    if (wire < t.num_routed) bad = wc_copy_violated(t, wires, sigmas, n, wire, row, gl_mul(k_is[wire], two_level(t.roots, row)), nullptr);
  }
  const u32 nbad = wc_wave_sum(bad ? 1u : 0u), nnc = wc_wave_sum(noncanonical ? 1u : 0u);
  if (nnc && lane == 0) atomicAdd((unsigned long long *)&res[WC_R_NONCANON], (unsigned long long)nnc);
  if (nbad) {  // wave-uniform
    const u64 first = wc_wave_min(bad ? wc_copy_key(row, wire) : WC_NONE);
    if (lane == 0) {
      atomicAdd((unsigned long long *)&res[WC_R_COPY_COUNT], (unsigned long long)nbad);
      atomicMin((unsigned long long *)&res[WC_R_COPY_KEY], (unsigned long long)first);
    }
  }
}
// the sigma value of the first violated cell, for the host to decode: it travels with the counts, in the one download
__global__ void k_witness_first_sigma(const u64 *__restrict__ sigmas, u64 n, u64 *res) {
  const u64 key = res[WC_R_COPY_KEY];
  res[WC_R_COPY_SIGMA] = key == WC_NONE ? 0 : sigmas[(key & 0xFFFFFFFFull) * n + (key >> 32)];
}

// host copy of NttHost::root_table(lg, false)
struct HostRoots {
  std::vector<u64> lo, hi;
  TwoLevelTable t;
  explicit HostRoots(u32 lg) {
    t.h = (lg + 1) / 2;
    const u64 w = gl_root_of_unity(lg);
    lo = make_pow_table(w, 1, (size_t)1 << t.h);
    hi = make_pow_table(w, 1ull << t.h, (size_t)1 << (lg - t.h));
    t.lo = lo.data(); t.hi = hi.data();
  }
};
}  // namespace lcp2

namespace lcp2 {
// the call itself, arguments checked (below)
int check_witness_run(lcp2_circuit *c, const u64 *wires, lcp2_mem wires_mem, const uint64_t *public_inputs, size_t num_public_inputs,
                      lcp2_witness_report *report, uint64_t *per_gate);
}  // namespace lcp2

extern "C" int lcp2_check_witness(lcp2_circuit *c, const uint64_t *wires, lcp2_mem wires_mem, const uint64_t *public_inputs, size_t num_public_inputs,
                                  lcp2_witness_report *report, uint64_t *per_gate, uint32_t num_gates) {
  LCP2_TRY(entry_guard(c, {wires, report}));
  lcp2_ctx *ctx = c->ctx;
  if (c->sharded()) return ctx->fail(LCP2_E_UNSUPPORTED, "lcp2_check_witness: a sharded circuit holds only its own blocks");
  if (num_public_inputs != c->npi || (num_public_inputs && !public_inputs)) return ctx->fail(LCP2_E_INVALID, "lcp2_check_witness: wrong number of public inputs");
  if ((unsigned)wires_mem > 1) return ctx->fail(LCP2_E_INVALID, "lcp2_check_witness: bad lcp2_mem");
  const u32 NG = (u32)c->gates.size();
  if (per_gate && num_gates != NG) return ctx->fail(LCP2_E_INVALID, "lcp2_check_witness: per_gate needs num_gates = the circuit's gate count");
  if (NG >= WC_MAX_GATES) return ctx->fail(LCP2_E_UNSUPPORTED, "lcp2_check_witness: 2^16 gates or more");
  for (const lcp2_gate &G : c->gates)
    if (G.num_constraints >= WC_MAX_CONSTRAINTS) return ctx->fail(LCP2_E_UNSUPPORTED, "lcp2_check_witness: a gate with 2^16 constraints or more");
  const int rc = check_witness_run(c, (const u64 *)wires, wires_mem, public_inputs, num_public_inputs, report, per_gate);
  // a failed call may have left the upload of a host witness in flight: the caller's buffer is his again only after the stream
  if (rc != LCP2_OK && wires_mem == LCP2_MEM_HOST) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

namespace lcp2 {
// the decode tables of this circuit on the device (cached in the context under the k_is): also what lcp2_witness_fill_copies decodes with
int wc_device_decode(lcp2_circuit *c, StageEnv &e, WcDecode *out) {
  const u32 NR = e.NR, d = e.p.degree_bits;
  std::string kis_key = "wckis:" + std::to_string(d);
  for (u64 k : c->k_is) kis_key += ":" + std::to_string(k);
  const u64 *d_tables = e.be.table(kis_key, [&] {
    std::vector<u64> t(2 * (size_t)NR);
    wc_decode_tables(c->k_is.data(), NR, d, t.data());
    return t;
  });
  WcDecode t{};
  t.roots = e.ntt.root_table(d, false);
  if (e.be.status) return e.be.status;
  t.kn = d_tables; t.kinv = d_tables + NR; t.num_routed = NR; t.degree_bits = d;
  *out = t;
  return LCP2_OK;
}

int check_witness_run(lcp2_circuit *c, const u64 *wires, lcp2_mem wires_mem, const uint64_t *public_inputs, size_t num_public_inputs,
                      lcp2_witness_report *report, uint64_t *per_gate) {
  lcp2_ctx *ctx = c->ctx;
  const u32 NG = (u32)c->gates.size();
  StageEnv e(c);
  LCP2_TRY(e.status);
  hipStream_t s = e.s;
  const u64 n = e.n;
  const u32 W = e.W, NR = e.NR, NC = e.NC, d = e.p.degree_bits;

  const u64 *d_wires = wires;
  if (wires_mem == LCP2_MEM_HOST) {
    void *up;
    LCP2_TRY(scratch_ensure(ctx, 0, (size_t)W * n * 8, &up));
    LCP2_HIP(ctx, hipMemcpyAsync(up, wires, (size_t)W * n * 8, hipMemcpyHostToDevice, s));  // the stream is waited for before the call returns
    d_wires = (const u64 *)up;
  }
  u64 *res;
  LCP2_TRY(scratch_ensure(ctx, 1, (size_t)(WC_R_WORDS + NG) * 8, (void **)&res));
  {  // counters, the two keys, the public-input hash: by value in the arguments of one small launch
    SmallWords w{};
    w.v[WC_R_GATE_KEY] = WC_NONE; w.v[WC_R_COPY_KEY] = WC_NONE;
    uint64_t h[4];
    LCP2_TRY(lcp2_hash_no_pad(public_inputs, num_public_inputs, h));
    for (u32 k = 0; k < 4; k++) w.v[WC_R_PI + k] = h[k];
    launch_set_words(s, res, w, WC_R_WORDS);
    LCP2_HIP(ctx, hipMemsetAsync(res + WC_R_WORDS, 0, (size_t)NG * 8, s));
  }
  // ---- gate constraints
  {
    QuotientArgs a{};
    a.wires = d_wires; a.consts = c->cs_values.u(); a.stride = n; a.count = n;
    a.imm = c->d_imm.u(); a.pis = res + WC_R_PI;
    a.code = (const u32 *)c->d_code.p; a.gates = (const GateDev *)c->d_gates.p; a.stage_list = (const u32 *)c->d_stage.p;
    a.num_wires = W; a.num_selectors = c->num_selectors; a.num_gates = NG;
    a.num_regs = c->num_regs;  // every program is WALKED here, also those K6 runs natively: the registers of all of them
    // (registers + staging slots) x threads words of LDS: 128 threads where that stays inside 64 KiB, else one wave
    const u32 T = (size_t)(a.num_regs + QUOTIENT_STAGE) * 128 * 8 <= 65536 ? 128 : 64;
    ProfScope ps(ctx, LCP2_K_QUOTIENT, (double)n * 8.0 * (W + NC));
    hipLaunchKernelGGL(k_witness_gates, dim3((unsigned)((n + T - 1) / T)), dim3(T), (size_t)(a.num_regs + QUOTIENT_STAGE) * T * 8, s, a, res,
                       per_gate ? res + WC_R_WORDS : nullptr);
  }
  // ---- copy constraints, and the words >= p
  const u64 *d_sigmas = c->cs_values.u() + (u64)NC * n;
  WcDecode t{};
  LCP2_TRY(wc_device_decode(c, e, &t));
  {
    ProfScope ps(ctx, LCP2_K_PERM_Z, (double)n * 8.0 * (W + NR));
    hipLaunchKernelGGL(k_witness_copies, dim3((unsigned)((n + 255) / 256), W), dim3(256), 0, s, d_wires, d_sigmas, c->d_kis.u(), t, n, res);
  }
  hipLaunchKernelGGL(k_witness_first_sigma, dim3(1), dim3(1), 0, s, d_sigmas, n, res);
  LCP2_HIP(ctx, hipGetLastError());
  // ---- everything comes back in one download, behind one synchronisation
  u64 r[WC_R_WORDS];
  {
    Download dl(ctx);
    LCP2_TRY(dl.add(r, res, sizeof r));
    if (per_gate) LCP2_TRY(dl.add(per_gate, res + WC_R_WORDS, (size_t)NG * 8));
    LCP2_TRY(dl.wait());
  }
  lcp2_witness_report out{};
  out.gate_violations = r[WC_R_GATE_COUNT];
  out.gate_row = ~0ull; out.copy_row = ~0ull; out.copy_to_row = ~0ull; out.copy_to_wire = WC_NO_WIRE;
  if (r[WC_R_GATE_KEY] != WC_NONE) {
    out.gate_row = r[WC_R_GATE_KEY] >> 32;
    out.gate_index = (u32)(r[WC_R_GATE_KEY] >> 16) & 0xFFFF;
    out.gate_constraint = (u32)r[WC_R_GATE_KEY] & 0xFFFF;
  }
  out.copy_violations = r[WC_R_COPY_COUNT];
  if (r[WC_R_COPY_KEY] != WC_NONE) {  // the partner of the first cell: the same text, on the host
    out.copy_row = r[WC_R_COPY_KEY] >> 32;
    out.copy_wire = (u32)r[WC_R_COPY_KEY];
    HostRoots roots(d);
    std::vector<u64> tab(2 * (size_t)NR);
    wc_decode_tables(c->k_is.data(), NR, d, tab.data());
    WcDecode h{tab.data(), tab.data() + NR, roots.t, NR, d};
    const WcCell to = wc_decode_cell(h, r[WC_R_COPY_SIGMA]);
    out.copy_to_wire = to.wire;
    out.copy_to_row = to.wire == WC_NO_WIRE ? ~0ull : to.row;
  }
  out.noncanonical_cells = r[WC_R_NONCANON];
  *report = out;
  return LCP2_OK;
}
}  // namespace lcp2
