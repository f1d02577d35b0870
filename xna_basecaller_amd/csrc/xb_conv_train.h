// xb_conv_train.h -- the convolutions' training of xb_conv_train.hip for callers inside csrc/: no argument checks, launches on the
// context's main stream, no synchronisation.  Private to csrc/; include after xb_ctx.h.
//
// The route: xb::conv_is_narrow(Cin, Cout, K, stride) of xb_conv_plan.h, which reads the shape alone -- stride 1, at most 16
// channels on either side and Cin K <= 64: the direct kernels (conv1, conv2); everything else: im2col and the fp32 products
// (conv3).  The wide route's workspace (dz | col | dcol | wt, xb::conv_wide) and the narrow route's float64 partials
// (xb::conv_narrow) belong to the context and grow with the calls.
#pragma once

namespace xb {

// z, y of one layer.  col_keep (wide route only, or null): where col (Lout n, Cin K) is written instead of the workspace, for a
// backward that is given it.
int conv_forward_run(xb_ctx *ctx, const float *x, const float *w, const float *bias, int n, int Cin, int Lin, int Cout, int K, int stride,
                     int tnc, float *z, float *y, float *col_keep);
// dx (or null), dw, db of one layer.  col_kept (wide route only, or null): the forward's col; without it col is recomputed from x.
int conv_backward_run(xb_ctx *ctx, const float *dy, const float *x, const float *z, const float *w, int n, int Cin, int Lin, int Cout, int K,
                      int stride, int tnc, float *dx, float *dw, float *db, const float *col_kept);
// out (cols, rows) = in (rows, cols)^T, exact (xb_top.hip)
int transpose_run(xb_ctx *ctx, const float *in, int rows, int cols, float *out);

}  // namespace xb
