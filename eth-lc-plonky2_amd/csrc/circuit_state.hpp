// The circuit handle and what the prover's host units (prover.hip, prover_build.hip, prover_stages.hip, prover_open.hip) share.
// fri_commit.hpp, the FRI back end of prover_open.hip and fri_openings.hip, builds on the copy helpers here and declares its own
// functions.  No kernel unit includes this.
#pragma once
#include <array>
#include <cstring>
#include <initializer_list>
#include <memory>
#include "host_protocol.hpp"
#include "internal.hpp"
#include "ntt_host.hpp"
#include "prover_kernels.hpp"

// a batched opening in flight: lcp2_fri_open runs its three phases back to back, a coset-sharded proof exchanges the
// openings after the first and the cap of FRI layer 0 after the second
struct FriOpenState {
  lcp2::gl2 zeta{}, alpha{};
  lcp2::HostChallenger ch;
  lcp2::gl2 fri_betas[LCP2_MAX_FRI_LAYERS] = {};
  lcp2::u64 pow_witness = 0;
  std::vector<lcp2::u64> idx, idx_up;  // the queried leaves [1 + layers][queries]; with this handle's local leaves behind them, as uploaded
  int phase = 0;  // 0: none, 1: openings evaluated, 2: final polynomial composed and FRI layer 0 committed
};

struct lcp2_circuit {
  using u64 = lcp2::u64;
  using DevBuf = lcp2::DevBuf;
  lcp2_ctx *ctx = nullptr;
  lcp2_params p{};
  uint32_t npi = 0, num_selectors = 0, num_regs = 1, dev_regs = 1;
  std::vector<lcp2::GateDev> dev_gates;  // the gate table as uploaded: offsets into the staged code
  std::vector<lcp2_gate> gates;
  std::vector<uint32_t> gate_degree;     // per gate: the degree bound of its constraints, derived from its program (prover_build.hip)
  lcp2::QuotientTiers tiers;             // K6: the bundles of low-degree gates evaluated on half of the quotient coset (none: all on the full tier)
  DevBuf d_half_mask, tier_planes;       // [num_gates] bundle masks; [bundles][CH][2^q n] plane values, first half computed, second half extended
  std::vector<uint32_t> code;
  std::vector<u64> imm, k_is;
  u64 digest[4] = {0, 0, 0, 0};
  std::vector<u64> cs_cap;
  u64 last_challenges[97] = {0};
  // device: description
  DevBuf d_gates, d_code, d_stage, d_imm, d_kis, d_l0, d_zh_inv, cs_values;
  lcp2_oracle cs;  // constants_sigmas commitment
  // device: per-proof workspace (allocated once)
  lcp2_oracle wires, zs, quot;
  std::array<lcp2_oracle *, 4> oracles() { return {&cs, &wires, &zs, &quot}; }  // in the order of the proof's opening sets
  DevBuf wires_vals, zs_vals, chunk_q, row_tot, scan_tmp, qvals, planes, small, partial, tables, alpha_limbs, open_out;
  DevBuf fri_c[2];                       // ping-pong coefficient planes [2][m]
  std::vector<DevBuf> fri_vals, fri_dig; // per layer: value planes [2][8 m_l], digests
  std::vector<std::vector<u64>> fri_level_off;
  std::vector<DevBuf> fri_d_level_off;
  DevBuf q_idx, q_buf;
  // staged proving (lcp2_commit_wires -> lcp2_perm_zs -> lcp2_quotient -> lcp2_fri_open)
  const u64 *d_wires_cur = nullptr;
  enum Stage { ST_NONE = 0, ST_WIRES, ST_ZS, ST_QVALS, ST_QUOT };  // what the handle holds of the proof in flight
  Stage stage = ST_NONE;
  FriOpenState fo;
  // coset-sharded circuit: this handle holds the leaf blocks [bf, bf + bc) of every LDE and Merkle tree;
  // bc = 0: all of them.  cap_final: the full constants_sigmas cap (hence the digest) is known.
  uint32_t bf = 0, bc = 0;
  bool cap_final = true;
  bool sharded() const { return bc != 0; }
  uint32_t nblocks() const { return bc ? bc : (1u << p.rate_bits); }
  // row exchange form of a sharded proof (lcp2_commit_wires_rows): the handle holds the witness VALUES of the rows
  // [row0(), row0() + rows()) only - rank r of `world` holds the r-th block of n / world rows - and runs the permutation
  // argument and the gate check on them
  bool rows_mode = false, cs_rows_ready = false;
  int perm_phase = 0;  // row exchange form: 1 after lcp2_perm_zs_rows_begin, 2 after _finish (the order is enforced: _commit reads what they wrote)
  DevBuf cs_rows;   // the constants on this rank's rows, [num_constants][rows()]
  DevBuf zs_rows;   // exchange buffer of Z / partial products, [world][num_challenges * (1 + npp)][rows()]
  // a sharded circuit with at most 8 blocks interpolates the quotient coset by coset (each rank its own blocks, before the
  // exchange of the planes) and combines the interpolants into the chunks afterwards: no rank transforms 2^rate_bits n points
  DevBuf q_combine;  // the combining matrix [R][R] (k_quotient_combine)
  bool local_quotient() const { return sharded() && p.rate_bits <= 3; }
  u64 perm_wrap[2 * lcp2::QUOTIENT_MAX_CH] = {0};  // per challenge: Z before the block's last row, the last row's quotient (host)
  u64 noncanon_host = 0;   // stage_wires: a witness value was >= p (arrives with the wires cap)
  DevBuf leaf_state;       // chunked commitment of the wires (lcp2_commit_wires_chunk): the sponge state of every local leaf, [12][leaves]
  int chunk_next = -1;     // the column the next chunk must start at; -1: no chunked commitment in progress
  DevBuf wit_slot[2];      // staged host witnesses (lcp2_witness_stage), [num_wires][n] each
  hipEvent_t wit_ready[2] = {nullptr, nullptr};  // the slot's upload has finished (recorded on the context's copy stream)
  bool wit_staged[2] = {false, false};
  ~lcp2_circuit() { for (hipEvent_t e : wit_ready) if (e) (void)hipEventDestroy(e); }
  // lcp2_witness_fill_copies (witness_fill.hip): the copy classes read back from the sigma columns, built at the first call
  DevBuf copy_class_of;              // [num_routed_wires][n] u32: the class of a routed cell, 0xFFFFFFFF for a cell that is its own image
  u64 copy_num_classes = 0;
  uint32_t copy_rounds = 0;          // pointer-jumping rounds that lowered a label while the table was built
  bool copy_classes_ready = false;
  bool check_pending = false;  // the gate-check verdict of stage_quotient_values has not been read yet (it arrives with the quotient cap)
  uint32_t world() const { return bc ? (1u << p.rate_bits) / bc : 1; }
  // q = ceil(log2 Q): K6 evaluates the quotient on the 2^q n-point coset 7 H_{2^q n}, the first 2^q n leaves of every LDE
  uint32_t qbits() const { uint32_t q = 0; while ((1u << q) < p.quotient_degree_factor) q++; return q; }
  uint32_t rank() const { return bc ? bf / bc : 0; }
  u64 rows() const { return rows_mode ? (1ull << p.degree_bits) / world() : (1ull << p.degree_bits); }
  u64 row0() const { return rows_mode ? rows() * rank() : 0; }
  // the words of a full-size cap that this handle's leaf blocks produce: 2^(cap_height - rate_bits) entries per block
  struct Range { size_t first, count; };
  Range cap_share() const {
    if (!sharded()) return {0, (size_t)4 << p.cap_height};
    const size_t per_block = (size_t)4 << (p.cap_height - p.rate_bits);
    return {bf * per_block, bc * per_block};
  }
  // first column and count of this rank's share of `nc` columns (the whole range for an unsharded circuit)
  void column_share(uint32_t nc, uint32_t &first, uint32_t &count) const {
    first = 0; count = nc;
    if (!sharded()) return;
    const uint32_t base = nc / world(), extra = nc % world();
    first = rank() * base + std::min(rank(), extra);
    count = base + (rank() < extra ? 1 : 0);
  }
};

namespace lcp2 {
#define LCP2_TRY(expr) do { int rc_ = (expr); if (rc_ != LCP2_OK) return rc_; } while (0)

inline u32 npp_of(const lcp2_params &p) { return (p.num_routed_wires + p.quotient_degree_factor - 1) / p.quotient_degree_factor - 1; }

inline int check_params(lcp2_ctx *ctx, const lcp2_params &p) {
  bool unsupported;
  if (const char *why = params_problem(p, &unsupported)) return ctx->fail(unsupported ? LCP2_E_UNSUPPORTED : LCP2_E_INVALID, why);
  return LCP2_OK;
}

// opens every entry point that works on the device: handle and required pointers non-null, else LCP2_E_INVALID; then a device, else LCP2_E_NODEVICE
inline int entry_guard(const lcp2_circuit *c, std::initializer_list<const void *> required = {}) {
  if (!c) return LCP2_E_INVALID;
  for (const void *q : required) if (!q) return LCP2_E_INVALID;
  return c->ctx ? LCP2_OK : LCP2_E_NODEVICE;
}

inline int upload(lcp2_ctx *ctx, DevBuf &b, const void *src, size_t bytes) {
  LCP2_HIP(ctx, b.ensure(bytes));
  if (bytes) LCP2_HIP(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return LCP2_OK;
}
// Device-to-host copies of a proof go through the context's pinned staging buffer: the pieces of one transcript step (a cap and a
// flag, all the openings, ...) are queued back to back and arrive with ONE synchronisation of the stream.
struct Download {
  lcp2_ctx *ctx;
  struct Piece { void *dst; size_t off, bytes; };
  std::vector<Piece> pieces;
  size_t used = 0;
  explicit Download(lcp2_ctx *c) : ctx(c) {}
  int add(void *dst, const void *src, size_t bytes) {
    if (!bytes) return LCP2_OK;
    if (!ctx->pin || used + bytes > lcp2_ctx::PIN_BYTES) {  // does not fit the staging buffer (or there is none): straight to its destination
      LCP2_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
      return LCP2_OK;
    }
    LCP2_HIP(ctx, hipMemcpyAsync((char *)ctx->pin + used, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    pieces.push_back({dst, used, bytes});
    used += (bytes + 7) & ~(size_t)7;
    return LCP2_OK;
  }
  int wait() {  // the one synchronisation; the staged pieces land in their destinations
    LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (const Piece &q : pieces) memcpy(q.dst, (const char *)ctx->pin + q.off, q.bytes);
    pieces.clear();
    used = 0;
    return LCP2_OK;
  }
};
inline int download(lcp2_ctx *ctx, void *dst, const void *src, size_t bytes) {
  Download d(ctx);
  LCP2_TRY(d.add(dst, src, bytes));
  return d.wait();
}
// a cap of this handle (device, its own entries only) into a full-size cap buffer: a sharded circuit writes its entries at their
// global position and zeros elsewhere (its share: the caps of all ranks OR-ed together are the cap)
inline int queue_cap(Download &d, const lcp2_circuit *c, const u64 *d_cap, u64 *dst) {
  const lcp2_circuit::Range mine = c->cap_share();
  if (c->sharded()) memset(dst, 0, ((size_t)4 << c->p.cap_height) * 8);
  return d.add(dst + mine.first, d_cap, mine.count * 8);
}

inline int select_device(lcp2_ctx *ctx) {
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  return LCP2_OK;
}
// What a stage works with: the context with its device selected (status: LCP2_OK or why not, the first thing a stage looks at),
// the circuit's shape under the names the formulas use, the proof layout, the stream and the transforms
struct StageEnv {
  lcp2_ctx *const ctx;
  const int status;
  const lcp2_params &p;
  const u64 n, N;
  const u32 lgN, W, NR, NC, CH, Q, npp, nchunks, ncs;
  const ProofLayout L;
  const hipStream_t s;
  DeviceNttBackend be;
  NttHost<DeviceNttBackend> ntt;
  explicit StageEnv(lcp2_circuit *c)
      : ctx(c->ctx), status(select_device(ctx)), p(c->p), n(1ull << p.degree_bits), N(n << p.rate_bits), lgN(p.degree_bits + p.rate_bits),
        W(p.num_wires), NR(p.num_routed_wires), NC(p.num_constants), CH(p.num_challenges), Q(p.quotient_degree_factor), npp(npp_of(p)),
        nchunks(npp + 1), ncs(NC + NR), L(p), s(ctx->stream), be{ctx}, ntt(be) {}
};

// ---- witness_check.hip: the cell-id decode tables of this circuit on the device (witness_check.hpp WcDecode), cached in the context
struct WcDecode;
int wc_device_decode(lcp2_circuit *c, StageEnv &e, WcDecode *out);
// ---- prover_stages.hip: each is a function of its inputs and of the commitments made by the stages before it
int stage_wires(lcp2_circuit *c, const u64 *wires_in, lcp2_mem wires_mem, const u64 *d_coeffs, u64 *cap_out, bool rows_only = false);
int perm_begin(lcp2_circuit *c, const u64 *betas, const u64 *gammas);
int queue_perm_wrap(Download &d, lcp2_circuit *c);
int perm_finish(lcp2_circuit *c, const u64 *prefix);
int perm_commit(lcp2_circuit *c, u64 *cap_out, bool with_wrap = false);
int stage_perm_zs(lcp2_circuit *c, const u64 *betas, const u64 *gammas, u64 *cap_out);
int tier_extend(lcp2_circuit *c, NttHost<DeviceNttBackend> &ntt);
int stage_quotient_values(lcp2_circuit *c, const u64 *alphas, const u64 *pi_hash, bool defer_check = false);
int stage_quotient_commit(lcp2_circuit *c, u64 *cap_out);
int stage_quotient(lcp2_circuit *c, const u64 *alphas, const u64 *pi_hash, u64 *cap_out);
// ---- prover_open.hip: the three phases of the batched opening, state in c->fo
int fri_open_openings(lcp2_circuit *c, u64 *proof);
int fri_open_commit(lcp2_circuit *c, u64 *proof);
int fri_open_finish(lcp2_circuit *c, u64 *proof);
}  // namespace lcp2
