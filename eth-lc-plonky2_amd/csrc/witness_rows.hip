// Witness-row entry points of liblcp2.so (K10): lcp2_sha256_witness, lcp2_scatter_cells, lcp2_poseidon_gate_rows,
// lcp2_u32_gate_rows, lcp2_rec_gate_rows, lcp2_witness_plan_rows, lcp2_witness_plan_rows_u32 and lcp2_witness_plan_rows_sha, with
// the device scratch, the host-to-device staging and the refusal flag they share (row_stage.hpp, which lcp2_witness_fill_copies
// uses too).  The last four check their arguments and run one level runner (run_plan_rows): a rec-gate call is a plan without SHA
// jobs, u32 jobs and PoseidonGate chains.  The kernels are in kernels_witness.hip; the per-row texts in sha_rows.hpp, pos_rows.hpp, u32_rows.hpp, rec_rows.hpp,
// pos_plan.hpp, u32_plan.hpp and sha_plan.hpp.
#include <cstring>
#include "internal.hpp"
#include "row_stage.hpp"
#include "sha_layout.hpp"
#include "sha_rows.hpp"
#include "pos_rows.hpp"
#include "prover_kernels.hpp"
#include "u32_rows.hpp"
#include "rec_rows.hpp"
#include "pos_plan.hpp"
#include "u32_plan.hpp"
#include "sha_plan.hpp"

using namespace lcp2;

namespace lcp2 {
// scratch slot `slot` of the context with at least `bytes` bytes (contents undefined); the stream orders its reuse
int scratch_ensure(lcp2_ctx *ctx, int slot, size_t bytes, void **out) {
  if (ctx->scratch_bytes[slot] < bytes) {
    if (ctx->scratch[slot]) { LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream)); LCP2_HIP(ctx, hipFree(ctx->scratch[slot])); ctx->scratch[slot] = nullptr; ctx->scratch_bytes[slot] = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    LCP2_HIP(ctx, hipMalloc(&ctx->scratch[slot], want));
    ctx->scratch_bytes[slot] = want;
  }
  *out = ctx->scratch[slot];
  return LCP2_OK;
}
}  // namespace lcp2

namespace {
// A table of ascending ends over `total` records, as level_ends, rec_level_ends, pos_level_ends and a host chain_ends must be:
// ENDS_OK, or the first entry below the one before it or above `total`, or `count` where the table does not end at `total`
constexpr size_t ENDS_OK = ~(size_t)0;
size_t ends_problem(const uint32_t *ends, size_t count, size_t total) {
  if (!total) return ENDS_OK;
  for (size_t l = 0; l < count; l++)
    if (ends[l] < (l ? ends[l - 1] : 0) || ends[l] > total) return l;
  return count && ends[count - 1] == total ? ENDS_OK : count;
}
}  // namespace

// ------------------------------------------------------------------ K10: witness generation, device buffers
static_assert(sizeof(lcp2_sha_job) == sizeof(ShaJobDev) && sizeof(lcp2_cell) == sizeof(CellDev), "ABI structs must match the kernels'");

extern "C" int lcp2_sha256_witness(lcp2_ctx *ctx, const lcp2_sha_job *jobs, size_t njobs, const uint32_t *level_start, uint32_t nlevels,
                                   const uint32_t *words_in, size_t nwords, uint64_t *wires, uint64_t n, uint32_t *digests) {
  if (!ctx || !wires || (njobs && (!jobs || !level_start || nlevels == 0)) || (nwords && !words_in)) return LCP2_E_INVALID;
  if (njobs == 0) return LCP2_OK;
  // validate once so that the kernels cannot read or write out of range (sha_rows.hpp)
  if (const ShaProblem refused = sha_jobs_problem((const ShaJobDev *)jobs, njobs, level_start, nlevels, nwords, n); refused.problem)
    return ctx->fail(LCP2_E_INVALID, sha_problem_str(refused.problem));
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  void *d_jobs, *d_words, *d_rec;
  LCP2_TRY(scratch_ensure(ctx, 0, njobs * sizeof(lcp2_sha_job), &d_jobs));
  LCP2_TRY(scratch_ensure(ctx, 1, std::max<size_t>(nwords, 1) * 4, &d_words));
  LCP2_TRY(scratch_ensure(ctx, 2, njobs * (size_t)SHA_REC_WORDS * 4, &d_rec));
  Stage stage{ctx};
  LCP2_TRY(stage.behind(d_jobs, jobs, njobs * sizeof(lcp2_sha_job)));
  if (nwords) LCP2_TRY(stage.behind(d_words, words_in, nwords * 4));
  {
    ProfScope ps(ctx, LCP2_K_SHA256, 96.0 * njobs + 8.0 * 108 * SHA_ROWS * njobs);
    for (uint32_t l = 0; l < nlevels; l++)
      launch_sha_jobs_level(ctx->stream, (const ShaJobDev *)d_jobs, level_start[l], level_start[l + 1] - level_start[l],
                            (const uint32_t *)d_words, (uint32_t *)d_rec);
    launch_sha_fill_rows(ctx->stream, (const ShaJobDev *)d_jobs, (u32)njobs, (const uint32_t *)d_rec, (u64 *)wires, n);
  }
  LCP2_HIP(ctx, hipGetLastError());
  // the 8 digest words of every job's record, as one strided copy (not the whole record buffer), through the pinned staging buffer
  // when they fit behind the uploads
  char *back = digests ? stage.room(njobs * 32) : nullptr;
  if (digests)
    LCP2_HIP(ctx, hipMemcpy2DAsync(back ? (void *)back : (void *)digests, 32, (const uint32_t *)d_rec + SHA_REC_DIGEST,
                                   (size_t)SHA_REC_WORDS * 4, 32, njobs, hipMemcpyDeviceToHost, ctx->stream));
  LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's job list and words may go; the digests have landed
  if (back) memcpy(digests, back, njobs * 32);
  return LCP2_OK;
}

extern "C" int lcp2_scatter_cells(lcp2_ctx *ctx, const lcp2_cell *cells, size_t ncells, uint64_t *wires, uint64_t n) {
  if (!ctx || !wires || (ncells && !cells)) return LCP2_E_INVALID;
  if (!ncells) return LCP2_OK;
  if (scatter_cells_problem((const CellDev *)cells, ncells, n) != ncells) return ctx->fail(LCP2_E_INVALID, "scatter: row out of range");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  void *d;
  LCP2_TRY(scratch_ensure(ctx, 3, ncells * sizeof(lcp2_cell), &d));
  LCP2_TRY(Stage{ctx}.behind(d, cells, ncells * sizeof(lcp2_cell)));  // (a list pinned by the caller - lcp2_host_register - goes up as a DMA too)
  launch_scatter_cells(ctx->stream, (const CellDev *)d, ncells, (u64 *)wires, n);
  LCP2_HIP(ctx, hipGetLastError());
  LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's list may go
  return LCP2_OK;
}

extern "C" int lcp2_poseidon_gate_rows(lcp2_ctx *ctx, const lcp2_poseidon_row *rows, size_t nrows, uint64_t *wires, uint64_t n) {
  static_assert(sizeof(lcp2_poseidon_row) == sizeof(PoseidonRowDev), "row job layouts must agree");
  if (!ctx || !wires || (nrows && !rows)) return LCP2_E_INVALID;
  if (!nrows) return LCP2_OK;
  for (size_t i = 0; i < nrows; i++)
    if (pos_row_problem(((const PoseidonRowDev *)rows)[i], n)) return ctx->fail(LCP2_E_INVALID, "poseidon rows: row out of range or swap flag not boolean");
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  void *d;
  LCP2_TRY(scratch_ensure(ctx, 0, nrows * sizeof(lcp2_poseidon_row), &d));
  LCP2_TRY(Stage{ctx}.behind(d, rows, nrows * sizeof(lcp2_poseidon_row)));
  launch_poseidon_gate_rows(ctx->stream, (const PoseidonRowDev *)d, nrows, (u64 *)wires, n, ctx->d_rc);
  LCP2_HIP(ctx, hipGetLastError());
  LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's list may go
  return LCP2_OK;
}

// plonky2_u32 / comparison rows: one job per operation of a row.  A host list is validated here, before anything is queued, and
// goes up in pieces through scratch slot 0 (a 2^22-row circuit of the reference's mix has 13 M jobs, 315 MB: the piece bounds the
// scratch, and the stream orders the kernel of one piece before the upload of the next).  A device list is validated by the
// kernel, which is why the flag word is read back either way.
extern "C" int lcp2_u32_gate_rows(lcp2_ctx *ctx, const lcp2_u32_job *jobs, size_t njobs, lcp2_mem jobs_mem, uint64_t *wires, uint64_t n) {
  static_assert(sizeof(lcp2_u32_job) == 24 && sizeof(lcp2_u32_job) == sizeof(U32JobDev), "job layouts must agree");
  static_assert(LCP2_U32_ARITHMETIC == U32_KIND_ARITHMETIC && LCP2_U32_ADD_MANY == U32_KIND_ADD_MANY && LCP2_U32_SUBTRACTION == U32_KIND_SUBTRACTION &&
                LCP2_U32_RANGE_CHECK == U32_KIND_RANGE_CHECK && LCP2_U32_COMPARISON == U32_KIND_COMPARISON, "kind numbering must agree");
  if (!ctx || !wires || (njobs && !jobs)) return LCP2_E_INVALID;
  if (jobs_mem != LCP2_MEM_HOST && jobs_mem != LCP2_MEM_DEVICE) return ctx->fail(LCP2_E_INVALID, "u32 rows: bad lcp2_mem");
  if (!njobs) return LCP2_OK;
  const U32JobDev *list = (const U32JobDev *)jobs;
  if (jobs_mem == LCP2_MEM_HOST)
    for (size_t i = 0; i < njobs; i++)
      if (u32 problem = u32_job_problem(list[i], n))
        return ctx->fail(LCP2_E_INVALID, "u32 rows: job " + std::to_string(i) + ": " + u32_problem_str(problem));
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  RefusalFlag flag{ctx};
  LCP2_TRY(flag.begin());
  if (jobs_mem == LCP2_MEM_DEVICE) {
    launch_u32_gate_rows(ctx->stream, list, njobs, (u64 *)wires, n, flag.d);
  } else {
    constexpr size_t PIECE = (size_t)1 << 20;  // jobs: 24 MiB
    void *d;
    LCP2_TRY(scratch_ensure(ctx, 0, std::min(njobs, PIECE) * sizeof(lcp2_u32_job), &d));
    for (size_t at = 0; at < njobs; at += PIECE) {
      const size_t count = std::min(PIECE, njobs - at);
      LCP2_TRY(Stage{ctx}.behind(d, list + at, count * sizeof(lcp2_u32_job), njobs <= PIECE));
      launch_u32_gate_rows(ctx->stream, (const U32JobDev *)d, count, (u64 *)wires, n, flag.d);
    }
  }
  return flag.end("u32 rows", u32_problem_str, "the valid jobs are written");
}

namespace {
// What a refusal says: "<label>: <rec_job or "poseidon job ">N: <reason>", and for one found on the device what is written
struct PlanTexts {
  const char *label, *rec_job, *written;
};

// A recorded plan of ALL FOUR families, level by level, behind lcp2_rec_gate_rows (a plan of rec jobs only), lcp2_witness_plan_rows
// (no u32 jobs), lcp2_witness_plan_rows_u32 (no SHA jobs) and lcp2_witness_plan_rows_sha, which have checked the arguments: the rec
// jobs of a level through k_rec_gate_rows (its job indices shifted per level, row_flag.hpp), then its SHA jobs through
// k_sha_plan_jobs and its u32 jobs through k_u32_plan_rows (both shifted alike), then its PoseidonGate chains through
// k_pos_plan_chains, all on the context's stream with no host wait in between.  Host lists are validated completely first (rec jobs,
// then SHA jobs, then u32 jobs, then PoseidonGate jobs: structure, and the values that are IMM) and go up whole through the pinned
// staging buffer, in pieces of its size: operands into scratch slot 2, rec jobs into slot 0, and into slot 3 the PoseidonGate jobs,
// chain_ends, the u32 plan jobs and the SHA plan jobs, each at an offset rounded to 16 bytes.  Device lists are validated by the
// kernels.  Either way the value conditions of CELL operands can only be seen on the device: the flag words (two; three with u32
// jobs; four with SHA jobs) are in slot 1 and come back once, after the last level, because a level that begins after a refused job
// writes nothing (rec_rows_lane, sha_plan_job_lane, u32_plan_lane, pos_plan_chain_lane).
int run_plan_rows(lcp2_ctx *ctx, const lcp2_witness_plan_sha &r, lcp2_mem lists_mem, uint64_t *wires, uint32_t ncols, uint64_t n, const PlanTexts &text) {
  const lcp2_witness_plan_u32 &q = r.base;
  const lcp2_witness_plan &p = q.base;
  const bool host = lists_mem == LCP2_MEM_HOST;
  const RecJobDev *rec = (const RecJobDev *)p.rec_jobs;
  const U32PlanJobDev *u32_jobs = (const U32PlanJobDev *)q.u32_jobs;
  const ShaPlanJobDev *sha = (const ShaPlanJobDev *)r.sha_jobs;
  const PosJobDev *pos = (const PosJobDev *)p.pos_jobs;
  const RecOperandDev *ops = (const RecOperandDev *)p.operands;
  const u32 *chain_ends = p.chain_ends;
  auto refused = [&](u32 family, u64 job, u32 problem, bool on_device) {
    return ctx->fail(LCP2_E_INVALID, std::string(text.label) + ": " + (family == 3 ? "sha job " : family == 2 ? "u32 job " : family ? "poseidon job " : text.rec_job) + std::to_string(job) + ": " +
                                         (family == 3 ? sha_plan_problem_str(problem) : family == 2 ? u32_plan_problem_str(problem)
                                          : family   ? pos_plan_problem_str(problem) : rec_problem_str(problem)) +
                                         (on_device ? std::string(" (found on the device: ") + text.written + ")" : std::string()));
  };
  if (host)
    if (const PlanProblem bad = plan_sha_lists_problem(rec, p.nrec, sha, r.nsha, u32_jobs, q.nu32, pos, chain_ends, p.nchains, ops, p.noperands, ncols, n);
        bad.problem)
      return refused(bad.family, bad.job, bad.problem, false);
  LCP2_HIP(ctx, hipSetDevice(ctx->device));
  RefusalFlag flag{ctx, r.nsha ? (size_t)4 : q.nu32 ? (size_t)3 : (size_t)2};
  LCP2_TRY(flag.begin());
  if (host) {
    void *d_rec, *d_ops, *d_lists = nullptr;
    const size_t pos_bytes = (p.npos * sizeof(lcp2_pos_job) + 15) & ~(size_t)15;
    const size_t chain_bytes = q.nu32 || r.nsha ? (p.nchains * sizeof(uint32_t) + 15) & ~(size_t)15 : std::max<size_t>(p.nchains, 1) * sizeof(uint32_t);
    LCP2_TRY(scratch_ensure(ctx, 0, std::max<size_t>(p.nrec, 1) * sizeof(lcp2_rec_job), &d_rec));
    LCP2_TRY(scratch_ensure(ctx, 2, std::max<size_t>(p.noperands, 1) * sizeof(lcp2_rec_operand), &d_ops));
    const size_t sha_at = pos_bytes + chain_bytes + q.nu32 * sizeof(lcp2_u32_plan_job);  // a multiple of 16
    if (p.npos || p.nchains || q.nu32 || r.nsha) LCP2_TRY(scratch_ensure(ctx, 3, sha_at + r.nsha * sizeof(lcp2_sha_plan_job), &d_lists));
    Stage stage{ctx};
    if (p.noperands) LCP2_TRY(stage.whole(d_ops, ops, p.noperands * sizeof(lcp2_rec_operand)));
    if (p.nrec) LCP2_TRY(stage.whole(d_rec, rec, p.nrec * sizeof(lcp2_rec_job)));
    if (p.npos) LCP2_TRY(stage.whole(d_lists, pos, p.npos * sizeof(lcp2_pos_job)));
    if (p.nchains) LCP2_TRY(stage.whole((char *)d_lists + pos_bytes, chain_ends, p.nchains * sizeof(uint32_t)));
    if (q.nu32) LCP2_TRY(stage.whole((char *)d_lists + pos_bytes + chain_bytes, u32_jobs, q.nu32 * sizeof(lcp2_u32_plan_job)));
    if (r.nsha) LCP2_TRY(stage.whole((char *)d_lists + sha_at, sha, r.nsha * sizeof(lcp2_sha_plan_job)));
    sha = (const ShaPlanJobDev *)((char *)d_lists + sha_at);
    rec = (const RecJobDev *)d_rec;
    ops = (const RecOperandDev *)d_ops;
    pos = (const PosJobDev *)d_lists;
    chain_ends = (const u32 *)((char *)d_lists + pos_bytes);
    u32_jobs = (const U32PlanJobDev *)((char *)d_lists + pos_bytes + chain_bytes);
  }
  for (size_t l = 0; l < p.nlevels; l++) {
    const u64 rec_begin = p.nrec && l ? p.rec_level_ends[l - 1] : 0, rec_end = p.nrec ? p.rec_level_ends[l] : 0, shift = plan_shift(l);
    launch_rec_gate_rows(ctx->stream, rec, shift, rec_begin + shift, rec_end + shift, ops, p.noperands, (u64 *)wires, ncols, n, flag.d, !host);
    if (r.nsha)
      launch_sha_plan_jobs(ctx->stream, sha, shift, (l ? r.sha_level_ends[l - 1] : 0) + shift, r.sha_level_ends[l] + shift, ops, p.noperands,
                           (u64 *)wires, ncols, n, flag.d, plan_gate(rec_begin, l), rec_end + shift);
    if (q.nu32)
      launch_u32_plan_rows(ctx->stream, u32_jobs, shift, (l ? q.u32_level_ends[l - 1] : 0) + shift, q.u32_level_ends[l] + shift, ops, p.noperands,
                           (u64 *)wires, ncols, n, flag.d, plan_gate(rec_begin, l), rec_end + shift);
    if (p.nchains)
      launch_pos_plan_chains(ctx->stream, pos, p.npos, chain_ends, l ? p.pos_level_ends[l - 1] : 0, p.pos_level_ends[l], ops, p.noperands,
                             (u64 *)wires, ncols, n, ctx->d_rc, flag.d, plan_gate(rec_begin, l), rec_end + shift);
  }
  LCP2_TRY(flag.read());
  const PlanRefusal found = r.nsha   ? plan_refusal_sha(flag.words, p.rec_level_ends, q.u32_level_ends, r.sha_level_ends, p.nlevels)
                            : q.nu32 ? plan_refusal_u32(flag.words, p.rec_level_ends, q.u32_level_ends, p.nlevels)
                                     : plan_refusal(flag.words, p.rec_level_ends, p.nlevels);
  return found.problem ? refused(found.family, found.job, found.problem, true) : LCP2_OK;
}
}  // namespace

// Recursion-gate rows, level by level: the plan that holds these rec jobs and no PoseidonGate job.
extern "C" int lcp2_rec_gate_rows(lcp2_ctx *ctx, const lcp2_rec_job *jobs, size_t njobs, const lcp2_rec_operand *operands, size_t noperands,
                                  const uint32_t *level_ends, size_t nlevels, lcp2_mem lists_mem, uint64_t *wires, uint32_t ncols, uint64_t n) {
  static_assert(sizeof(lcp2_rec_job) == 16 && sizeof(lcp2_rec_job) == sizeof(RecJobDev) && sizeof(lcp2_rec_operand) == 16 &&
                sizeof(lcp2_rec_operand) == sizeof(RecOperandDev), "record layouts must agree");
  static_assert(LCP2_REC_ARITHMETIC == REC_ARITHMETIC && LCP2_REC_BASE_SUM == REC_BASE_SUM && LCP2_REC_ARITHMETIC_EXT == REC_ARITHMETIC_EXT &&
                LCP2_REC_MUL_EXT == REC_MUL_EXT && LCP2_REC_REDUCING == REC_REDUCING && LCP2_REC_REDUCING_EXT == REC_REDUCING_EXT &&
                LCP2_REC_POSEIDON_MDS == REC_POSEIDON_MDS && LCP2_REC_RANDOM_ACCESS == REC_RANDOM_ACCESS &&
                LCP2_REC_EXPONENTIATION == REC_EXPONENTIATION && LCP2_REC_COSET_INTERPOLATION == REC_COSET_INTERPOLATION &&
                LCP2_REC_KINDS == REC_KINDS && LCP2_REC_IMM == REC_IMM && LCP2_REC_CELL == REC_CELL, "numbering must agree");
  if (!ctx || !wires || (njobs && (!jobs || !level_ends || !nlevels)) || (noperands && !operands)) return LCP2_E_INVALID;
  if (lists_mem != LCP2_MEM_HOST && lists_mem != LCP2_MEM_DEVICE) return ctx->fail(LCP2_E_INVALID, "rec rows: bad lcp2_mem");
  if (!njobs) return LCP2_OK;
  if (ncols < REC_ROW_COLUMNS) return ctx->fail(LCP2_E_INVALID, "rec rows: the matrix needs at least 135 columns");
  if (const size_t at = ends_problem(level_ends, nlevels, njobs); at != ENDS_OK)
    return ctx->fail(LCP2_E_INVALID, at < nlevels ? "rec rows: level_ends is not ascending at level " + std::to_string(at)
                                                  : std::string("rec rows: level_ends does not end at njobs"));
  const lcp2_witness_plan_sha plan = {{{jobs, njobs, level_ends, nullptr, 0, nullptr, 0, nullptr, operands, noperands, nlevels}, nullptr, 0, nullptr}, nullptr, 0, nullptr};
  return run_plan_rows(ctx, plan, lists_mem, wires, ncols, n,
                       {"rec rows", "job ", "the valid jobs of its level and of the levels before are written, later levels are not"});
}

namespace {
// lcp2_witness_plan_rows, lcp2_witness_plan_rows_u32 and lcp2_witness_plan_rows_sha behind their null checks: the arguments, then the
// level runner
int checked_plan_rows(lcp2_ctx *ctx, const lcp2_witness_plan_sha &r, lcp2_mem lists_mem, uint64_t *wires, uint32_t ncols, uint64_t n) {
  const lcp2_witness_plan_u32 &q = r.base;
  const lcp2_witness_plan &p = q.base;
  if (lists_mem != LCP2_MEM_HOST && lists_mem != LCP2_MEM_DEVICE) return ctx->fail(LCP2_E_INVALID, "plan rows: bad lcp2_mem");
  if ((p.nrec && (!p.rec_jobs || !p.rec_level_ends)) || (p.npos && !p.pos_jobs) || (p.nchains && (!p.chain_ends || !p.pos_level_ends)) ||
      (q.nu32 && (!q.u32_jobs || !q.u32_level_ends)) || (r.nsha && (!r.sha_jobs || !r.sha_level_ends)) || (p.noperands && !p.operands) ||
      ((p.nrec || p.nchains || q.nu32 || r.nsha) && !p.nlevels))
    return ctx->fail(LCP2_E_INVALID, "plan rows: a list is null but its count is not zero");
  if (!p.nrec && !p.npos && !q.nu32 && !r.nsha) return LCP2_OK;
  if (ncols < POS_GATE_WIRES) return ctx->fail(LCP2_E_INVALID, "plan rows: the matrix needs at least 135 columns");
  if (p.nrec > 0xFFFFFFFFull || p.npos > 0xFFFFFFFFull || p.nchains > 0xFFFFFFFFull || q.nu32 > 0xFFFFFFFFull || r.nsha > 0xFFFFFFFFull)
    return ctx->fail(LCP2_E_INVALID, "plan rows: more than 2^32 - 1 jobs or chains");
  auto ends_text = [](const uint32_t *ends, size_t count, size_t total, const char *name) -> std::string {
    const size_t at = ends_problem(ends, count, total);
    if (at == ENDS_OK) return "";
    return std::string("plan rows: ") + name + (at < count ? " is not ascending at entry " + std::to_string(at) : " does not end at its count");
  };
  std::string bad = ends_text(p.rec_level_ends, p.nlevels, p.nrec, "rec_level_ends");
  if (bad.empty()) bad = ends_text(r.sha_level_ends, p.nlevels, r.nsha, "sha_level_ends");
  if (bad.empty()) bad = ends_text(q.u32_level_ends, p.nlevels, q.nu32, "u32_level_ends");
  if (bad.empty()) bad = ends_text(p.pos_level_ends, p.nlevels, p.nchains, "pos_level_ends");
  if (bad.empty() && lists_mem == LCP2_MEM_HOST) bad = ends_text(p.chain_ends, p.nchains, p.npos, "chain_ends");
  if (!bad.empty()) return ctx->fail(LCP2_E_INVALID, bad);
  return run_plan_rows(ctx, r, lists_mem, wires, ncols, n,
                       {"plan rows", "rec job ", "the valid rec jobs of its level, the rows of its chain before it, the other chains of its level and all "
                                                 "earlier levels are written, later levels are not"});
}
}  // namespace

extern "C" int lcp2_witness_plan_rows(lcp2_ctx *ctx, const lcp2_witness_plan *plan, lcp2_mem lists_mem, uint64_t *wires, uint32_t ncols, uint64_t n) {
  static_assert(sizeof(lcp2_pos_job) == 8 && sizeof(lcp2_pos_job) == sizeof(PosJobDev), "record layouts must agree");
  static_assert(LCP2_PLAN_IMM == PLAN_IMM && LCP2_PLAN_CELL == PLAN_CELL && LCP2_PLAN_PREV == PLAN_PREV && LCP2_PLAN_IMM == LCP2_REC_IMM &&
                LCP2_PLAN_CELL == LCP2_REC_CELL, "numbering must agree");
  if (!ctx || !plan || !wires) return LCP2_E_INVALID;
  return checked_plan_rows(ctx, {{*plan, nullptr, 0, nullptr}, nullptr, 0, nullptr}, lists_mem, wires, ncols, n);
}

// The plan that also holds plonky2_u32 / comparison jobs: with nu32 = 0 exactly lcp2_witness_plan_rows on plan->base
extern "C" int lcp2_witness_plan_rows_u32(lcp2_ctx *ctx, const lcp2_witness_plan_u32 *plan, lcp2_mem lists_mem, uint64_t *wires, uint32_t ncols,
                                          uint64_t n) {
  static_assert(sizeof(lcp2_u32_plan_job) == 16 && sizeof(lcp2_u32_plan_job) == sizeof(U32PlanJobDev), "record layouts must agree");
  if (!ctx || !plan || !wires) return LCP2_E_INVALID;
  return checked_plan_rows(ctx, {*plan, nullptr, 0, nullptr}, lists_mem, wires, ncols, n);
}

// The plan that also holds SHA-256 jobs: with nsha = 0 exactly lcp2_witness_plan_rows_u32 on plan->base
extern "C" int lcp2_witness_plan_rows_sha(lcp2_ctx *ctx, const lcp2_witness_plan_sha *plan, lcp2_mem lists_mem, uint64_t *wires, uint32_t ncols,
                                          uint64_t n) {
  static_assert(sizeof(lcp2_sha_plan_job) == 8 && sizeof(lcp2_sha_plan_job) == sizeof(ShaPlanJobDev), "record layouts must agree");
  if (!ctx || !plan || !wires) return LCP2_E_INVALID;
  return checked_plan_rows(ctx, *plan, lists_mem, wires, ncols, n);
}
