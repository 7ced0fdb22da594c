// build(): lcp2_circuit_create and the verifier-only constructor, with the checks both make of a circuit description, and the
// accessors of what build() leaves in the handle (digest, cap, proof size, the verifier's view).
#include <algorithm>
#include <cstdlib>
#include "circuit_state.hpp"
#include "gate_program.hpp"

using namespace lcp2;
namespace gp = gate_program;

namespace lcp2 {
// shape checks shared by build() and the verifier-only constructor: everything the prover's workspaces and the verifier's
// fixed-size arrays rely on.  Returns nullptr or the reason; *unsupported says which status it is.
const char *params_problem(const lcp2_params &p, bool *unsupported) {
  *unsupported = false;
  if (p.degree_bits < 1 || p.rate_bits < 1 || p.rate_bits > 8 || p.degree_bits + p.rate_bits > 30) return "degree_bits / rate_bits out of range";
  if (p.num_wires == 0 || p.num_wires > 65535 || p.num_constants > 65535) return "bad column counts";
  if (p.num_routed_wires > p.num_wires || p.num_routed_wires == 0) return "bad routed wire count";
  if (p.cap_height > p.degree_bits + p.rate_bits) return "cap_height exceeds the LDE tree";
  *unsupported = true;
  if (p.quotient_degree_factor < 2 || p.quotient_degree_factor > (1u << p.rate_bits)) return "quotient_degree_factor must lie in [2, 2^rate_bits]";
  if (p.num_challenges < 1 || p.num_challenges > QUOTIENT_MAX_CH) return "num_challenges must be 1 or 2";
  if ((p.num_routed_wires + p.quotient_degree_factor - 1) / p.quotient_degree_factor > PERM_MAX_CHUNKS) return "too many routed wires";
  if (p.num_query_rounds > 64 || p.num_fri_layers > LCP2_MAX_FRI_LAYERS) return "too many queries / layers";
  if (p.proof_of_work_bits < 1 || p.proof_of_work_bits > 40) return "proof_of_work_bits out of range";
  *unsupported = false;
  u32 lg = p.degree_bits + p.rate_bits, d = p.degree_bits;
  for (u32 l = 0; l < p.num_fri_layers; l++) {
    u32 ab = p.fri_arity_bits[l];
    if (ab < 1 || ab > 5 || ab > d || lg - ab < p.cap_height) return "bad FRI arity schedule";
    lg -= ab; d -= ab;
  }
  return nullptr;
}
}  // namespace lcp2

namespace {
// light_gates.hpp weights constraint j with entry j of the alpha-limb table, as the generated evaluators do
static_assert(QUOTIENT_TERM_POWS == 128, "the limit LIGHT_GATE_LIMIT names");
const char *const LIGHT_GATE_LIMIT = "LCP2_GATE_NATIVE_ARITHMETIC / LCP2_GATE_NATIVE_BASE_SUM2: at most 128 constraints (the alpha power table holds 128 weights)";
// validate the programs once so that neither the kernels nor the host verifier ever index out of range
const char *validate_programs(const lcp2_circuit_desc *d) {
  const lcp2_params &p = d->params;
  if (d->num_regs > 64 || d->num_selectors > p.num_constants) return "bad gate set";
  const gp::Limits limits{std::max(d->num_regs, 1u), p.num_wires, p.num_constants - d->num_selectors, d->num_imm, 4};
  for (u32 g = 0; g < d->num_gates; g++) {
    const lcp2_gate &G = d->gates[g];
    if (G.selector_index >= d->num_selectors || ((size_t)G.code_offset + (size_t)G.code_len) * 2 > d->code_words || G.group_end < G.group_start ||
        (G.flags & ~(LCP2_GATE_EMIT_FORWARD | LCP2_GATE_NATIVE_MASK)))
      return "gate descriptor out of range";
    switch (G.flags & LCP2_GATE_NATIVE_MASK) {
      case 0: break;
      case LCP2_GATE_NATIVE_POSEIDON:
        if (!(G.flags & LCP2_GATE_EMIT_FORWARD) || G.num_constraints != 123 || p.num_wires < 135) return "LCP2_GATE_NATIVE_POSEIDON needs 135 wires, 123 forward-emitted constraints";
        break;
      case LCP2_GATE_NATIVE_ARITHMETIC:
        if ((G.flags & LCP2_GATE_EMIT_FORWARD) || G.num_constraints == 0 || 4 * (size_t)G.num_constraints > p.num_wires || p.num_constants - d->num_selectors < 2)
          return "LCP2_GATE_NATIVE_ARITHMETIC needs 4 wires per operation and 2 gate constants";
        if (G.num_constraints > QUOTIENT_TERM_POWS) return LIGHT_GATE_LIMIT;
        break;
      case LCP2_GATE_NATIVE_BASE_SUM2:
        if ((G.flags & LCP2_GATE_EMIT_FORWARD) || G.num_constraints < 2 || G.num_constraints > p.num_wires) return "LCP2_GATE_NATIVE_BASE_SUM2 needs num_limbs + 1 wires";
        if (G.num_constraints > QUOTIENT_TERM_POWS) return LIGHT_GATE_LIMIT;
        break;
      default:
        // a generated evaluator weights constraint j with alpha^j whichever way the program lists them (the claim check decides)
        if (!(G.flags & 0x8000u) || ((G.flags >> 8) & 0x7Fu) >= QUOTIENT_GENERATED_GATES || G.num_constraints > QUOTIENT_TERM_POWS) return "unknown native gate id";
        break;
    }
    size_t emits_seen = 0;
    for (size_t pc = G.code_offset; pc < (size_t)G.code_offset + G.code_len; pc++) {
      const gp::Insn in(d->code[2 * pc], d->code[2 * pc + 1]);
      if (const char *why = gp::insn_problem(in, limits)) return why;
      emits_seen += in.emits();
    }
    if (emits_seen != G.num_constraints) return "num_constraints does not match the program";
  }
  return nullptr;
}

using gp::program_degree;  // the degree bound of a program's constraints (gate_program.hpp)

// The half tier of K6 (prover_kernels.hpp QuotientTiers), from the derived degrees alone.  Per selector group the gates of degree
// <= 2^(q-1) are taken by falling degree and put first-fit into bundles with max degree + size - 1 <= 2^(q-1).
void form_bundles(lcp2_circuit *c) {
  QuotientTiers &t = c->tiers;
  t.bundles.clear();
  t.bundle_of.assign(c->gates.size(), -1);
  const u32 qb = c->qbits();
  if (qb == 0) return;
  const u32 half = 1u << (qb - 1);
  std::vector<u32> order;
  for (u32 g = 0; g < c->gates.size(); g++) {
    const lcp2_gate &G = c->gates[g];
    if (G.num_constraints == 0 || c->gate_degree[g] > half) continue;
    if (G.selector_value < G.group_start || G.selector_value >= G.group_end || G.group_end - G.group_start > 64) continue;  // the masks hold 64 values
    order.push_back(g);
  }
  std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) { return c->gate_degree[x] > c->gate_degree[y]; });
  std::vector<u32> maxdeg;
  for (u32 g : order) {
    const lcp2_gate &G = c->gates[g];
    size_t b = 0;
    for (; b < t.bundles.size(); b++) {
      const QuotientBundle &B = t.bundles[b];
      if (B.selector_index == G.selector_index && B.group_start == G.group_start && B.group_end == G.group_end &&
          maxdeg[b] + B.gates.size() <= half && !((B.mask >> (G.selector_value - G.group_start)) & 1))
        break;
    }
    if (b == t.bundles.size()) {
      t.bundles.push_back(QuotientBundle{G.selector_index, G.group_start, G.group_end, 0, {}});
      maxdeg.push_back(c->gate_degree[g]);  // falling degrees: the first gate of a bundle has the largest
    }
    t.bundles[b].gates.push_back(g);
    t.bundles[b].mask |= 1ull << (G.selector_value - G.group_start);
    t.bundle_of[g] = (int)b;
  }
}

// circuit_builder.rs::build: circuit_digest = hash_no_pad(constants_sigmas_cap || domain_separator_digest || degree_bits) with
// domain_separator_digest = hash_pad(domain separator), the separator empty unless the builder sets one: pad10*1 = [1, 0 x 6, 1]
void circuit_digest(const std::vector<u64> &cs_cap, u32 degree_bits, u64 digest[4]) {
  std::vector<u64> buf(cs_cap);
  const u64 empty_padded[8] = {1, 0, 0, 0, 0, 0, 0, 1};
  u64 ds[4];
  HostPoseidon::get().hash_no_pad(empty_padded, 8, ds);
  buf.insert(buf.end(), ds, ds + 4);
  buf.push_back(degree_bits);
  HostPoseidon::get().hash_no_pad(buf.data(), buf.size(), digest);
}

// The LCP2_GATE_NATIVE_* claims of the description, checked on the device: program and native evaluator on 256 random points
// (a polynomial identity in 135 + NC variables of degree <= 9: a wrong claim survives with probability ~2^-60).
int check_native_gates(lcp2_circuit *c) {
  lcp2_ctx *ctx = c->ctx;
  bool any = false;
  for (const lcp2_gate &G : c->gates) any = any || (G.flags & LCP2_GATE_NATIVE_MASK);
  if (!any) return LCP2_OK;
  const lcp2_params &p = c->p;
  const u64 cnt = 256;
  u64 seed = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { seed += 0x9E3779B97F4A7C15ull; u64 z = seed; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return gl_canon(z ^ (z >> 31)); };
  std::vector<u64> hw((size_t)p.num_wires * cnt), hc((size_t)p.num_constants * cnt);
  for (auto &v : hw) v = rnd();
  for (auto &v : hc) v = rnd();
  DevBuf dw, dc;
  LCP2_TRY(upload(ctx, dw, hw.data(), hw.size() * 8));
  LCP2_TRY(upload(ctx, dc, hc.data(), hc.size() * 8));
  LCP2_HIP(ctx, c->alpha_limbs.ensure((size_t)QUOTIENT_MAX_CH * QUOTIENT_TERM_POWS * 16));
  u64 *d_small = c->small.u();
  QuotientSetupArgs qs{};
  for (u32 i = 0; i < 4; i++) qs.pi_hash[i] = rnd();
  qs.num_challenges = p.num_challenges; qs.num_gates = (u32)c->gates.size(); qs.gates = (const GateDev *)c->d_gates.p; qs.small = d_small;
  qs.limbs = (u32 *)c->alpha_limbs.p;
  QuotientArgs a{};
  a.wires = dw.u(); a.consts = dc.u(); a.stride = cnt; a.count = cnt;
  a.alphas = d_small + SMALL_ALPHAS; a.alpha_inv = d_small + SMALL_ALPHA_INV; a.pis = d_small + SMALL_PI_HASH; a.gate_scale = d_small + SMALL_GATE_SCALE;
  a.alpha_limbs = (const u32 *)c->alpha_limbs.p;
  a.imm = c->d_imm.u(); a.code = (const u32 *)c->d_code.p; a.gates = (const GateDev *)c->d_gates.p; a.stage_list = (const u32 *)c->d_stage.p;
  a.num_wires = p.num_wires; a.num_gates = (u32)c->gates.size(); a.num_selectors = c->num_selectors; a.num_constants = p.num_constants;
  a.num_challenges = p.num_challenges; a.num_regs = c->num_regs; a.rc = ctx->d_rc;
  u64 bad = ~0ull;
  // two settings of the challenges: random ones, and alpha = 0 (there the combination is the FIRST constraint alone, the corner in
  // which a forward and a last-to-first evaluator differ if one of them folds in the wrong direction).  Everything derived from
  // them, and the reset flag, comes from the setup kernel of a proof (k_quotient_setup).
  for (int zero_alpha = 0; zero_alpha < 2 && bad == ~0ull; zero_alpha++) {
    for (u32 k = 0; k < p.num_challenges; k++) qs.alphas[k] = zero_alpha ? 0 : gl_canon(rnd() | 1);
    launch_quotient_setup(ctx->stream, qs);
    launch_native_check(ctx->stream, a, c->dev_gates, (unsigned long long *)(d_small + SMALL_CHECK));
    LCP2_HIP(ctx, hipGetLastError());
    LCP2_TRY(download(ctx, &bad, d_small + SMALL_CHECK, 8));
  }
  if (bad != ~0ull) return ctx->fail(LCP2_E_INVALID, "a gate flagged LCP2_GATE_NATIVE_* does not compute what its program computes");
  return LCP2_OK;
}

// the description as the handle keeps it (prover and verifier alike): immediates and coset shifts canonical
void copy_description(lcp2_circuit *c, const lcp2_circuit_desc *d) {
  const lcp2_params &p = d->params;
  c->p = p; c->npi = d->num_public_inputs; c->num_selectors = d->num_selectors; c->num_regs = std::max(d->num_regs, 1u);
  c->gates.assign(d->gates, d->gates + d->num_gates);
  c->code.assign(d->code, d->code + d->code_words);
  c->imm.resize(std::max<size_t>(d->num_imm, 1), 0);
  for (size_t i = 0; i < d->num_imm; i++) c->imm[i] = gl_canon(d->imm[i]);
  c->k_is.resize(p.num_routed_wires);
  for (u32 i = 0; i < p.num_routed_wires; i++) c->k_is[i] = gl_canon(d->k_is[i]);
  c->gate_degree.resize(c->gates.size());
  for (size_t g = 0; g < c->gates.size(); g++) c->gate_degree[g] = program_degree(c->code.data(), c->gates[g].code_offset, c->gates[g].code_len, c->num_regs);
  c->tiers.bundle_of.assign(c->gates.size(), -1);
}

int circuit_create(lcp2_ctx *ctx, const lcp2_circuit_desc *d, uint32_t bf, uint32_t bc, lcp2_circuit **out) {
  if (!ctx || !d || !out) return LCP2_E_INVALID;
  *out = nullptr;
  if (!d->constants_sigmas || !d->k_is || !d->gates || !d->code || (d->num_imm && !d->imm)) return ctx->fail(LCP2_E_INVALID, "null description field");
  LCP2_TRY(check_params(ctx, d->params));
  const lcp2_params &p = d->params;
  if (d->num_selectors > p.num_constants || d->num_regs > 64 || d->num_gates == 0) return ctx->fail(LCP2_E_INVALID, "bad gate set");
  if (d->num_public_inputs > (1u << 20)) return ctx->fail(LCP2_E_UNSUPPORTED, "too many public inputs");
  if (const char *why = validate_programs(d)) return ctx->fail(LCP2_E_INVALID, why);
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<lcp2_circuit> c(new lcp2_circuit());
  c->ctx = ctx;
  if (bc) {
    if (p.quotient_degree_factor != (1u << p.rate_bits)) return ctx->fail(LCP2_E_UNSUPPORTED, "sharded circuit: needs quotient_degree_factor = 2^rate_bits");
    if (p.cap_height < p.rate_bits) return ctx->fail(LCP2_E_INVALID, "sharded circuit: needs cap_height >= rate_bits");
    if ((bc & (bc - 1)) || bf % bc || bf + bc > (1u << p.rate_bits)) return ctx->fail(LCP2_E_INVALID, "sharded circuit: block range must be an aligned power of two");
    c->bf = bf; c->bc = bc; c->cap_final = false;
    for (lcp2_oracle *o : c->oracles()) { o->block_first = bf; o->block_count = bc; }
  }
  copy_description(c.get(), d);
  const u64 n = 1ull << p.degree_bits, N = n << p.rate_bits;
  const u32 ncs = p.num_constants + p.num_routed_wires, CH = p.num_challenges, npp = npp_of(p), nchunks = npp + 1;
  {  // the device runs the staged form of the programs (prover_kernels.hpp); the verifier keeps the caller's form
    static_assert(sizeof(GateDev) == sizeof(lcp2_gate), "GateDev mirrors lcp2_gate");
    std::vector<GateDev> &dev_gates = c->dev_gates;
    dev_gates.resize(c->gates.size());
    memcpy(dev_gates.data(), c->gates.data(), c->gates.size() * sizeof(lcp2_gate));
    std::vector<uint32_t> staged, lists;
    stage_gate_programs(c->code, dev_gates, p.num_wires, c->num_selectors, staged, lists);
    // LDS registers the DEVICE needs: programs that run natively never touch them (their count is only a verifier matter)
    c->dev_regs = 1;
    for (const lcp2_gate &G : c->gates) {
      if (G.flags & LCP2_GATE_NATIVE_MASK) continue;
      for (size_t pc = G.code_offset; pc < (size_t)G.code_offset + G.code_len; pc++)
        c->dev_regs = std::max(c->dev_regs, gp::Insn(c->code[2 * pc], c->code[2 * pc + 1]).top_reg());
    }
    staged.resize(staged.size() + 4, 0);  // padded by two instructions: K6 fetches one instruction ahead of the one it executes
    LCP2_TRY(upload(ctx, c->d_gates, dev_gates.data(), dev_gates.size() * sizeof(GateDev)));
    LCP2_TRY(upload(ctx, c->d_code, staged.data(), staged.size() * 4));
    LCP2_TRY(upload(ctx, c->d_stage, lists.data(), lists.size() * 4));
    LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging vectors go out of scope
  }
  LCP2_TRY(upload(ctx, c->d_imm, c->imm.data(), c->imm.size() * 8));
  LCP2_TRY(upload(ctx, c->d_kis, c->k_is.data(), c->k_is.size() * 8));
  // constants_sigmas values stay resident (K5 reads the sigma columns on H)
  LCP2_HIP(ctx, c->cs_values.alloc((size_t)ncs * n * 8));
  LCP2_HIP(ctx, hipMemcpyAsync(c->cs_values.p, d->constants_sigmas, (size_t)ncs * n * 8,
                               d->constants_sigmas_mem == LCP2_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  LCP2_TRY(commit_values_dev(ctx, c->cs_values.u(), ncs, p.degree_bits, p.rate_bits, p.cap_height, &c->cs));
  const size_t capw = (size_t)4 << p.cap_height;
  c->cs_cap.resize(capw);
  {
    Download dl(ctx);
    LCP2_TRY(queue_cap(dl, c.get(), c->cs.cap_dev(), c->cs_cap.data()));
    LCP2_TRY(dl.wait());
  }
  if (!c->sharded()) circuit_digest(c->cs_cap, p.degree_bits, c->digest);  // sharded: lcp2_circuit_set_constants_cap
  // L_0 on the LDE points (leaf order): LDE of the polynomial with all coefficients 1/n
  {
    DevBuf ones;
    LCP2_HIP(ctx, ones.alloc(n * 8));
    launch_fill(ctx->stream, ones.u(), n, gl_inv(n % GL_P));
    LCP2_HIP(ctx, c->d_l0.alloc(N * 8));
    DeviceNttBackend be{ctx};
    NttHost<DeviceNttBackend> ntt(be);
    ntt.forward(ones.u(), n, c->d_l0.u(), N, p.degree_bits, 1, GL_GENERATOR, p.rate_bits);
    if (be.status) return be.status;
    LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  const u32 qb = c->qbits();
  const u64 NQ = n << qb;  // the quotient's domain (= N when Q = 2^rate_bits)
  {  // 1 / Z_H(7 w_NQ^j) depends on j mod 2^q = bitrev of the top q bits of the leaf index
    std::vector<u64> t(1u << qb);
    u64 shift_n = gl_pow(GL_GENERATOR, n), wr = gl_root_of_unity(qb);
    for (u32 top = 0; top < (1u << qb); top++) {
      u32 r = bitrev32(top, qb);
      t[top] = gl_inv(gl_sub(gl_mul(shift_n, gl_pow(wr, r)), 1));
    }
    LCP2_TRY(upload(ctx, c->d_zh_inv, t.data(), t.size() * 8));
  }
  // per-proof workspace
  LCP2_HIP(ctx, c->zs_vals.alloc((size_t)CH * (1 + npp) * n * 8));
  LCP2_HIP(ctx, c->chunk_q.alloc((size_t)CH * nchunks * n * 8));
  LCP2_HIP(ctx, c->row_tot.alloc((size_t)CH * n * 8));
  LCP2_HIP(ctx, c->scan_tmp.alloc(std::max(scan_scratch_words(n, 4), (u64)16) * 8));
  LCP2_HIP(ctx, c->qvals.alloc((size_t)CH * NQ * 8));
  {  // K6's half tier; LCP2_QUOTIENT_TIERS=0 in the environment keeps every gate on the full tier.  A sharded circuit evaluates
     // its own leaf blocks only and has no coset prefix to halve.
    const char *sw = getenv("LCP2_QUOTIENT_TIERS");
    if (!c->sharded() && !(sw && sw[0] == '0' && !sw[1])) form_bundles(c.get());
    if (c->tiers.on()) {
      std::vector<u64> masks(c->gates.size(), 0);
      for (const QuotientBundle &B : c->tiers.bundles)
        for (u32 g : B.gates) masks[g] = B.mask;
      LCP2_TRY(upload(ctx, c->d_half_mask, masks.data(), masks.size() * 8));
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `masks` goes out of scope
      LCP2_HIP(ctx, c->tier_planes.alloc(c->tiers.bundles.size() * (size_t)CH * NQ * 8));
      // one extension of zeroed planes: the transforms' twiddle and shift tables and the coefficient buffer exist before the first proof
      LCP2_HIP(ctx, hipMemsetAsync(c->tier_planes.p, 0, c->tiers.bundles.size() * (size_t)CH * NQ * 8, ctx->stream));
      DeviceNttBackend be{ctx};
      NttHost<DeviceNttBackend> ntt(be);
      LCP2_TRY(tier_extend(c.get(), ntt));
      if (be.status) return be.status;
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  LCP2_HIP(ctx, c->planes.alloc((size_t)4 * n * 8));
  LCP2_HIP(ctx, c->small.alloc((SMALL_GATE_SCALE + (size_t)QUOTIENT_MAX_CH * d->num_gates + 8) * 8));
  {
    u32 maxcols = std::max(std::max(ncs, p.num_wires), std::max(CH * (1 + npp), CH * p.quotient_degree_factor));
    u64 nchk = (n + EVAL_CHUNK - 1) / EVAL_CHUNK;
    LCP2_HIP(ctx, c->partial.alloc((size_t)maxcols * nchk * 16 + (size_t)maxcols * 16));
  }
  LCP2_HIP(ctx, c->tables.alloc(((size_t)8 * ((1ull << ((p.degree_bits + 1) / 2)) + (n >> ((p.degree_bits + 1) / 2)) + 2) + 4 * 1024 + 2 * (ncs + p.num_wires + 64) + 64) * 16));
  LCP2_HIP(ctx, c->fri_c[0].alloc((size_t)2 * n * 8));
  LCP2_HIP(ctx, c->fri_c[1].alloc((size_t)2 * n * 8));
  {
    u64 m = n;
    c->fri_vals.resize(p.num_fri_layers); c->fri_dig.resize(p.num_fri_layers);
    c->fri_level_off.resize(p.num_fri_layers); c->fri_d_level_off.resize(p.num_fri_layers);
    for (u32 l = 0; l < p.num_fri_layers; l++) {
      u64 nvals = m << p.rate_bits, nleaves = nvals >> p.fri_arity_bits[l];
      u32 h = 0;
      while ((1ull << h) < nleaves) h++;
      u32 nlev = h - p.cap_height + 1;
      if (l == 0 && c->sharded()) {  // its own leaf blocks only, down to its own cap entries: the same number of levels
        nvals = (u64)c->bc * m;
        nleaves = nvals >> p.fri_arity_bits[0];
      }
      LCP2_HIP(ctx, c->fri_vals[l].alloc((size_t)2 * nvals * 8));
      c->fri_level_off[l].resize(nlev);
      u64 tot = 0;
      for (u32 k = 0; k < nlev; k++) { c->fri_level_off[l][k] = tot; tot += nleaves >> k; }
      LCP2_HIP(ctx, c->fri_dig[l].alloc(tot * 32));
      LCP2_TRY(upload(ctx, c->fri_d_level_off[l], c->fri_level_off[l].data(), nlev * 8));
      m >>= p.fri_arity_bits[l];
    }
  }
  LCP2_HIP(ctx, c->q_idx.alloc(64 * 8 * (3 + LCP2_MAX_FRI_LAYERS)));
  LCP2_HIP(ctx, c->q_buf.alloc((size_t)64 * (ncs + p.num_wires + CH * (1 + npp) + CH * p.quotient_degree_factor + 4 * 4 * 32 + LCP2_MAX_FRI_LAYERS * (64 + 4 * 32)) * 8));
  LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LCP2_TRY(check_native_gates(c.get()));
  *out = c.release();
  return LCP2_OK;
}
}  // namespace

extern "C" int lcp2_circuit_create(lcp2_ctx *ctx, const lcp2_circuit_desc *d, lcp2_circuit **out) { return circuit_create(ctx, d, 0, 0, out); }
extern "C" int lcp2_circuit_create_sharded(lcp2_ctx *ctx, const lcp2_circuit_desc *d, uint32_t block_first, uint32_t block_count,
                                           lcp2_circuit **out) {
  if (block_count == 0) return LCP2_E_INVALID;
  return circuit_create(ctx, d, block_first, block_count, out);
}
extern "C" int lcp2_circuit_set_constants_cap(lcp2_circuit *c, const uint64_t *cap) {
  if (!c || !cap) return LCP2_E_INVALID;
  if (!c->sharded()) return LCP2_E_INVALID;
  const lcp2_circuit::Range mine = c->cap_share();  // the entries this handle computed itself must be in the cap it is given
  if (memcmp(cap + mine.first, c->cs_cap.data() + mine.first, mine.count * 8) != 0)
    return c->ctx->fail(LCP2_E_INVALID, "constants cap does not contain this shard's entries");
  c->cs_cap.assign((const u64 *)cap, (const u64 *)cap + c->cs_cap.size());
  circuit_digest(c->cs_cap, c->p.degree_bits, c->digest);
  c->cap_final = true;
  return LCP2_OK;
}

extern "C" int lcp2_verifier_create(const lcp2_circuit_desc *d, const uint64_t digest[4], const uint64_t *cap, lcp2_circuit **out) {
  if (!d || !digest || !cap || !out || !d->k_is || !d->gates || !d->code) return LCP2_E_INVALID;
  *out = nullptr;
  const lcp2_params &p = d->params;
  bool unsupported;
  if (params_problem(p, &unsupported)) return unsupported ? LCP2_E_UNSUPPORTED : LCP2_E_INVALID;  // the verifier indexes fixed-size arrays by these
  if (d->num_selectors > p.num_constants || d->num_gates == 0 || (d->num_imm && !d->imm)) return LCP2_E_INVALID;
  if (validate_programs(d)) return LCP2_E_INVALID;
  lcp2_circuit *c = new lcp2_circuit();
  copy_description(c, d);
  memcpy(c->digest, digest, 32);
  c->cs_cap.assign((const u64 *)cap, (const u64 *)cap + ((size_t)4 << p.cap_height));
  *out = c;
  return LCP2_OK;
}

extern "C" void lcp2_circuit_destroy(lcp2_circuit *c) {
  if (!c) return;
  if (c->ctx) { (void)hipSetDevice(c->ctx->device); (void)hipStreamSynchronize(c->ctx->stream); }
  delete c;
}
extern "C" int lcp2_circuit_digest(const lcp2_circuit *c, uint64_t digest[4], uint64_t *cap) {
  if (!c || !digest) return LCP2_E_INVALID;
  memcpy(digest, c->digest, 32);
  if (cap) memcpy(cap, c->cs_cap.data(), c->cs_cap.size() * 8);
  return LCP2_OK;
}
extern "C" size_t lcp2_proof_words(const lcp2_params *p) {
  bool unsupported;
  if (!p || params_problem(*p, &unsupported)) return 0;  // the layout arithmetic relies on a sane FRI schedule
  return ProofLayout(*p).total;
}
extern "C" int lcp2_gate_program_degree(const uint32_t *code, size_t num_instructions, uint32_t num_regs, uint32_t *degree) {
  if (!code || !degree || num_regs > 64) return LCP2_E_INVALID;
  const gp::Limits registers_only{std::max(num_regs, 1u)};  // the walk below indexes nothing else
  for (size_t pc = 0; pc < num_instructions; pc++)
    if (gp::insn_problem(gp::Insn(code[2 * pc], code[2 * pc + 1]), registers_only)) return LCP2_E_INVALID;
  *degree = program_degree(code, 0, num_instructions, registers_only.regs);
  return LCP2_OK;
}
extern "C" int lcp2_circuit_gate_tiers(const lcp2_circuit *c, uint32_t num_gates, uint32_t *degrees, int32_t *bundles) {
  if (!c || num_gates != c->gates.size()) return LCP2_E_INVALID;
  for (uint32_t g = 0; g < num_gates; g++) {
    if (degrees) degrees[g] = c->gate_degree[g];
    if (bundles) bundles[g] = c->tiers.bundle_of[g];
  }
  return LCP2_OK;
}
extern "C" int lcp2_last_challenges(const lcp2_circuit *c, uint64_t out[97]) {
  if (!c || !out) return LCP2_E_INVALID;
  memcpy(out, c->last_challenges, sizeof c->last_challenges);
  return LCP2_OK;
}

// host-side accessors for the verifier (verifier.hip)
namespace lcp2 {
VerifierView verifier_view(const lcp2_circuit *c) {
  VerifierView v;
  v.p = &c->p; v.npi = c->npi; v.num_selectors = c->num_selectors;
  v.gates = c->gates.data(); v.num_gates = (u32)c->gates.size(); v.code = c->code.data(); v.imm = c->imm.data();
  v.k_is = c->k_is.data(); v.digest = c->digest; v.cs_cap = c->cs_cap.data();
  v.code_words = c->code.size(); v.num_imm = c->imm.size(); v.num_regs = c->num_regs;
  return v;
}
}  // namespace lcp2
