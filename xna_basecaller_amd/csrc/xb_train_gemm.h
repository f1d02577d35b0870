// xb_train_gemm.h -- the fp32 training products of xb_train_gemm.hip for callers inside csrc/: no argument checks, launches on
// the context's main stream, no synchronisation.  Private to csrc/; include after xb_ctx.h.
#pragma once

namespace xb {

// xb_wgrad_f32's sum over the rows: a running fp32 sum (four rows per MFMA) is closed every WGRAD_BLOCK_ROWS rows and added to
// the element's total, blocks in ascending order -- the blocked form of the two the contract allows.  A multiple of 32.
constexpr long WGRAD_BLOCK_ROWS = 1024;

int linear_f32_run(xb_ctx *ctx, const float *a, const float *w, const float *bias, int64_t M, int N, int K, int act, float scale, float *out);
int wgrad_f32_run(xb_ctx *ctx, const float *a, const float *b, int64_t M, int N, int K, float *dw, float *dcol, long block_rows = WGRAD_BLOCK_ROWS);
int head_dz_run(xb_ctx *ctx, const float *y, const float *dy, int64_t count, float scale, float *dz);

}  // namespace xb
