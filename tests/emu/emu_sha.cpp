// TEST HARNESS (not product code): csrc/sha_rows.hpp compiled for the CPU - the lanes of k_sha_jobs_level and k_sha_fill_rows
// (lcp2_sha256_witness) and of k_scatter_cells (lcp2_scatter_cells), the validation they share with the host entry points, and the
// kernels' grids as loops over lanes (blocks of 64 and of 256, as launch_sha_jobs_level / launch_sha_fill_rows size them).
// Built by tests/test_sha_rows.py with g++; never loaded by the package.
#include <vector>
#include "../../eth-lc-plonky2_amd/csrc/sha_rows.hpp"

using namespace lcp2;

extern "C" {

unsigned emu_sha_job_bytes() { return (unsigned)sizeof(ShaJobDev); }
unsigned emu_sha_cell_bytes() { return (unsigned)sizeof(CellDev); }
unsigned emu_sha_rows() { return SHA_ROWS; }
unsigned emu_sha_row_columns() { return SHA_ROW_COLUMNS; }
const char *emu_sha_problem_str(unsigned problem) { return sha_problem_str(problem); }

// sha_jobs_problem: the problem (0: none), *where = the job or level it names
unsigned emu_sha_jobs_problem(const ShaJobDev *jobs, unsigned long long njobs, const unsigned *level_start, unsigned nlevels,
                              unsigned long long nwords, unsigned long long n, unsigned *where) {
  const ShaProblem p = sha_jobs_problem(jobs, (size_t)njobs, level_start, nlevels, (size_t)nwords, n);
  if (where) *where = p.job;
  return p.problem;
}

// lcp2_sha256_witness without a device: the validation, then per level the grid of k_sha_jobs_level (blocks of 64 lanes), then
// the grid of k_sha_fill_rows (blocks of 256 lanes) storing into `wires` ([>= 108][n], column-major).  Returns the problem and
// writes nothing when the list is refused.  digests: njobs * 8 words, or null.
unsigned emu_sha256_witness(const ShaJobDev *jobs, unsigned long long njobs, const unsigned *level_start, unsigned nlevels,
                            const unsigned *words_in, unsigned long long nwords, unsigned long long *wires, unsigned long long n,
                            unsigned *digests) {
  if (njobs == 0) return 0;
  if (const ShaProblem p = sha_jobs_problem(jobs, (size_t)njobs, level_start, nlevels, (size_t)nwords, n); p.problem) return p.problem;
  std::vector<uint32_t> rec((size_t)njobs * SHA_REC_WORDS, 0xDEADBEEFu);  // the device's scratch is not cleared either
  for (unsigned l = 0; l < nlevels; l++) {
    const u32 first = level_start[l], count = level_start[l + 1] - level_start[l];
    for (u32 block = 0; block < (count + 63) / 64; block++)
      for (u32 lane = 0; lane < 64; lane++) {
        const u32 k = block * 64 + lane;
        if (k >= count) continue;
        const u32 j = first + k;
        sha_job_record(jobs[j], j, words_in, rec.data());
      }
  }
  const u64 threads = (u64)njobs * SHA_ROWS;
  for (u64 block = 0; block < (threads + 255) / 256; block++)
    for (u32 lane = 0; lane < 256; lane++) {
      const u64 gid = block * 256 + lane;
      if (gid >= threads) continue;
      const u32 j = (u32)(gid / SHA_ROWS), lr = (u32)(gid % SHA_ROWS);
      u64 *Wp = wires + ((u64)jobs[j].first_row + lr);
      sha_row_cells(rec.data() + (u64)j * SHA_REC_WORDS, lr, [&](u32 col, u64 v) { Wp[(u64)col * n] = v; });
    }
  if (digests)
    for (u64 j = 0; j < njobs; j++)
      for (u32 i = 0; i < 8; i++) digests[8 * j + i] = rec[j * SHA_REC_WORDS + SHA_REC_DIGEST + i];
  return 0;
}

// lcp2_scatter_cells without a device: 1 and nothing written when a row is out of range, else the grid of k_scatter_cells
unsigned emu_scatter_cells(const CellDev *cells, unsigned long long ncells, unsigned long long *wires, unsigned long long n) {
  if (scatter_cells_problem(cells, (size_t)ncells, n) != ncells) return 1;
  for (u64 block = 0; block < (ncells + 255) / 256; block++)
    for (u32 lane = 0; lane < 256; lane++) scatter_cell_lane(cells, ncells, block * 256 + lane, wires, n);
  return 0;
}

}  // extern "C"
