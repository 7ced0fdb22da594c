// What the witness entry points that take lists share on the host (witness_rows.hip, witness_fill.hip): the host-to-device staging of
// a call through the context's pinned buffer, and the refusal flag of a call whose kernels validate (row_flag.hpp).  No kernel
// unit includes this.
#pragma once
#include <algorithm>
#include <cstring>
#include "internal.hpp"
#include "row_flag.hpp"

namespace lcp2 {
// Host -> device staging of one call through the context's pinned buffer (a copy out of pinned memory is a plain DMA that the
// stream orders).  The buffer is free when a call begins: every entry point here waits for its transfers before it returns.
struct Stage {
  lcp2_ctx *ctx;
  size_t used = 0;  // bytes of the pinned buffer this call has handed out
  // the next `bytes` bytes of the pinned buffer, nullptr when they do not fit (or there is no buffer)
  char *room(size_t bytes) const { return ctx->pin && used + bytes <= lcp2_ctx::PIN_BYTES ? (char *)ctx->pin + used : nullptr; }
  // Behind what this call already staged, else from the caller's memory: `src` must stay until the stream is synchronised.
  // via_pin = false: never through the pinned buffer, for a list that goes up in pieces (the buffer serves one transfer per
  // call, and the copy of an earlier piece may still be reading it)
  int behind(void *dst, const void *src, size_t bytes, bool via_pin = true) {
    char *p = via_pin ? room(bytes) : nullptr;
    if (p) { memcpy(p, src, bytes); used += (bytes + 63) & ~(size_t)63; }
    LCP2_HIP(ctx, hipMemcpyAsync(dst, p ? p : src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return LCP2_OK;
  }
  // Whole payload through the whole pinned buffer, in pieces of its size: `src` is reusable on return, and so is the buffer for
  // the next call of whole(), which first waits for the copy this one left in flight.  Not to be mixed with behind() in one call
  int whole(void *dst, const void *src, size_t bytes) {
    if (!ctx->pin) {
      LCP2_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
      return LCP2_OK;
    }
    for (size_t at = 0; at < bytes; at += lcp2_ctx::PIN_BYTES) {
      const size_t piece = std::min(lcp2_ctx::PIN_BYTES, bytes - at);
      LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the copy out of the staging buffer that may still be in flight
      memcpy(ctx->pin, (const char *)src + at, piece);
      LCP2_HIP(ctx, hipMemcpyAsync((char *)dst + at, ctx->pin, piece, hipMemcpyHostToDevice, ctx->stream));
    }
    return LCP2_OK;
  }
};

// The refusal flag of a call whose kernels validate jobs (row_flag.hpp), in scratch slot 1: one word, the two of a plan, the three of a plan
// with u32 jobs, or the four of a plan with SHA jobs
struct RefusalFlag {
  lcp2_ctx *ctx;
  size_t nwords = 1;
  u64 *d = nullptr;
  u64 words[4] = {0, 0, 0, 0};
  int begin() {
    LCP2_TRY(scratch_ensure(ctx, 1, nwords * sizeof(u64), (void **)&d));
    LCP2_HIP(ctx, hipMemsetAsync(d, 0xFF, nwords * sizeof(u64), ctx->stream));  // ROW_NO_PROBLEM
    return LCP2_OK;
  }
  // after the last launch: launch errors first, then the words come back and the stream is waited for (the caller's lists may go;
  // every cell is written)
  int read() {
    LCP2_HIP(ctx, hipGetLastError());
    LCP2_HIP(ctx, hipMemcpyAsync(words, d, nwords * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    LCP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LCP2_OK;
  }
  // read() of one word.  A refusal is LCP2_E_INVALID, "<family>: job N: <reason> (found on the device: <written>)"
  int end(const char *family, const char *(*reason)(u32), const char *written) {
    LCP2_TRY(read());
    if (words[0] == ROW_NO_PROBLEM) return LCP2_OK;
    return ctx->fail(LCP2_E_INVALID, std::string(family) + ": job " + std::to_string(words[0] >> 8) + ": " + reason((u32)(words[0] & 0xFF)) +
                                         " (found on the device: " + written + ")");
  }
};
}  // namespace lcp2
