// xb_conv_train.hip -- the training forward and the backward of one `Convolution` layer of rnn_encoder (Conv1d with padding K / 2 and
// a bias, then swish), in fp32: xb_conv_train_forward_dev keeps the pre-activation z beside y, xb_conv_train_backward_dev makes dx,
// dw and db from dy, x and z.  Two routes, chosen by the shape alone (xb_conv_plan.h: conv_is_narrow): the narrow one is direct
// kernels for a few channels at stride 1 (conv1, conv2), memory-bound, one pass over the operands each way; the wide one is an
// im2col, the fp32 products of xb_train_gemm.hip and a gather col2im (conv3).  The contracts are in the public header.  No
// floating-point atomics: every sum has an order its shape alone decides.  Built without contraction, division correctly rounded
// (lt_sigmoid is the training recurrence's function, xb_math.h).
#include "xb_ctx.h"
#include "xb_math.h"
#include "xb_conv_plan.h"
#include "xb_train_gemm.h"
#include "xb_conv_train.h"

namespace {

struct ConvShape {
    int n, Cin, Cout, K, stride, pad, tnc;
    long Lin, Lout;
};

// where element (chunk b, channel co, position t) of z, y and dy lies: (n, Cout, Lout), or (Lout, n, Cout) with tnc
__device__ __forceinline__ size_t out_at(const ConvShape &s, int b, int co, long t)
{
    return s.tnc ? ((size_t)t * s.n + b) * s.Cout + co : ((size_t)b * s.Cout + co) * s.Lout + t;
}

// y = z sigma(z);  dy / dz = sigma(z) (1 + z (1 - sigma(z))): one rounding per operation
__device__ __forceinline__ float swish(float z) { return z * lt_sigmoid(z); }
__device__ __forceinline__ float swish_grad(float z)
{
    const float sg = lt_sigmoid(z);
    return sg * (1.0f + z * (1.0f - sg));
}

// ---- the narrow route -----------------------------------------------------------------------------------------------------------
constexpr int TL = xb::CONV_TILE;
constexpr int NARROW_SW = xb::CONV_NARROW_MAX_C * xb::CONV_NARROW_MAX_CK;                     // all weights, Cout padded to CO
constexpr int NARROW_SX = xb::CONV_NARROW_MAX_C * (TL - 1) + xb::CONV_NARROW_MAX_CK;          // Cin rows of TL + K - 1
constexpr int NARROW_SD = xb::CONV_NARROW_MAX_C * (TL - 1 + xb::CONV_NARROW_MAX_CK);          // CO rows of TL + K - 1

// the weights of CO output channels, zeros behind Cout, and the rows [first, first + W) of the Cin channels of chunk b, zeros
// outside [0, Lin): consecutive threads read consecutive samples
template <int CO>
__device__ __forceinline__ void narrow_stage(const ConvShape &s, const float *w, const float *x, int b, long first, int W, float *sw, float *sx)
{
    const int CK = s.Cin * s.K;
    for (int i = threadIdx.x; i < CO * CK; i += 256) sw[i] = i < s.Cout * CK ? w[i] : 0.0f;
    for (int i = threadIdx.x; i < s.Cin * W; i += 256) {
        const int ci = i / W, j = i - ci * W;
        const long xi = first + j;
        sx[i] = xi >= 0 && xi < s.Lin ? x[((size_t)b * s.Cin + ci) * s.Lin + xi] : 0.0f;
    }
}

// Workgroup (chunk b, tile of TL output positions), thread = one position and all Cout channels of it.  z = (sum over ci
// ascending, k ascending of fma(x, w, .)) + bias.
template <int CO>
__global__ __launch_bounds__(256) void conv_narrow_fwd_kernel(const float *x, const float *w, const float *bias, ConvShape s, int tiles, float *z,
                                                              float *y)
{
    __shared__ float sw[NARROW_SW], sx[NARROW_SX];
    const int tid = threadIdx.x, b = blockIdx.x / tiles, W = TL + s.K - 1, CK = s.Cin * s.K;
    const long p0 = (long)(blockIdx.x % tiles) * TL;
    narrow_stage<CO>(s, w, x, b, p0 - s.pad, W, sw, sx);
    __syncthreads();
    const long t = p0 + tid;
    if (t >= s.Lout) return;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = 0.0f;
    for (int ci = 0; ci < s.Cin; ++ci)
        for (int k = 0; k < s.K; ++k) {
            const float xv = sx[ci * W + tid + k];
#pragma unroll
            for (int co = 0; co < CO; ++co) acc[co] = __builtin_fmaf(xv, sw[co * CK + ci * s.K + k], acc[co]);
        }
#pragma unroll
    for (int co = 0; co < CO; ++co) {
        if (co >= s.Cout) continue;
        const float zv = (acc[co] + bias[co]) + 0.0f;
        const size_t at = out_at(s, b, co, t);
        z[at] = zv;
        y[at] = swish(zv) + 0.0f;
    }
}

// Workgroup (chunk b, tile of TL positions p0 .. p0 + TL - 1 of max(Lin, Lout)).  It stages dz = dy swish'(z) of the output
// positions its dx gathers from (TL + K - 1 of them) and the x window of its own output positions.
//   dx[b, ci, s], s in the tile: sum over co ascending, k ascending of fma(dz[b, co, s + pad - k], w[co, ci, k], .)
//   dw, db: the tile's own output positions t.  Wave q sums positions 64 q .. 64 q + 63 in ascending order in float64 (the
//   products of two floats are exact there), lane = output element; the four waves' sums are added as (0 + 1) + (2 + 3): one
//   float64 partial per element and workgroup, at part[blockIdx.x][element].
template <int CO>
__global__ __launch_bounds__(256) void conv_narrow_bwd_kernel(const float *dy, const float *x, const float *z, const float *w, ConvShape s, int tiles,
                                                              float *dx, double *part)
{
    __shared__ float sw[NARROW_SW], sx[NARROW_SX], sd[NARROW_SD];
    __shared__ double red[256];
    const int tid = threadIdx.x, b = blockIdx.x / tiles, W = TL + s.K - 1, CK = s.Cin * s.K;
    const long p0 = (long)(blockIdx.x % tiles) * TL;
    narrow_stage<CO>(s, w, x, b, p0 - s.pad, W, sw, sx);
    const long tb = p0 + s.pad - (s.K - 1);                 // the output position of sd's column 0
    for (int i = tid; i < CO * W; i += 256) {
        const int co = i / W, j = i - co * W;
        const long t = tb + j;
        float v = 0.0f;
        if (co < s.Cout && t >= 0 && t < s.Lout) {
            const size_t at = out_at(s, b, co, t);
            v = dy[at] * swish_grad(z[at]);
        }
        sd[i] = v;
    }
    __syncthreads();
    const long sp = p0 + tid;
    if (dx && sp < s.Lin) {
        for (int ci = 0; ci < s.Cin; ++ci) {
            float acc = 0.0f;
#pragma unroll
            for (int co = 0; co < CO; ++co)
                for (int k = 0; k < s.K; ++k) acc = __builtin_fmaf(sd[co * W + tid + s.K - 1 - k], sw[co * CK + ci * s.K + k], acc);
            dx[((size_t)b * s.Cin + ci) * s.Lin + sp] = acc + 0.0f;
        }
    }
    const int q = tid >> 6, lane = tid & 63, nw = s.Cout * CK, outputs = nw + s.Cout;
    const int shift = s.K - 1 - s.pad;                      // sd's column of output position p0
    double *mine = part + (size_t)blockIdx.x * outputs;
    for (int o0 = 0; o0 < outputs; o0 += 64) {
        const int o = o0 + lane;
        double sum = 0.0;
        if (o < nw) {
            const int co = o / CK, r = o - co * CK, ci = r / s.K, k = r - ci * s.K;
            const float *pd = sd + co * W + shift + 64 * q, *px = sx + ci * W + k + 64 * q;
            for (int tt = 0; tt < 64; ++tt) sum += (double)pd[tt] * (double)px[tt];
        } else if (o < outputs) {
            const float *pd = sd + (o - nw) * W + shift + 64 * q;
            for (int tt = 0; tt < 64; ++tt) sum += (double)pd[tt];
        }
        red[tid] = sum;
        __syncthreads();
        if (tid < 64 && o0 + tid < outputs) mine[o0 + tid] = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
        __syncthreads();
    }
}

// dw and db: the workgroups' partials added in ascending order in float64, rounded once
__global__ __launch_bounds__(64) void conv_narrow_sum_kernel(const double *part, size_t blocks, int nw, int outputs, float *dw, float *db)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= outputs) return;
    double sum = 0.0;
#pragma unroll 8
    for (size_t k = 0; k < blocks; ++k) sum += part[k * outputs + o];
    const float r = (float)sum + 0.0f;
    if (o < nw) dw[o] = r;
    else db[o - nw] = r;
}

// ---- the wide route -------------------------------------------------------------------------------------------------------------
// col (Lout n, Cin K): row t n + b, column ci K + k holds x[b, ci, t stride + k - pad], +0 in the padding
__global__ __launch_bounds__(256) void conv_im2col_kernel(const float *x, ConvShape s, size_t count, float *col)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int CK = s.Cin * s.K;
    const size_t row = i / CK;
    const int c = (int)(i - row * CK), ci = c / s.K, k = c - ci * s.K;
    const long t = (long)(row / s.n);
    const int b = (int)(row - (size_t)t * s.n);
    const long xi = t * s.stride + k - s.pad;
    col[i] = xi >= 0 && xi < s.Lin ? x[((size_t)b * s.Cin + ci) * s.Lin + xi] : 0.0f;
}

// where element i of z's layout lies among the rows (row t n + b, Cout columns)
__device__ __forceinline__ size_t row_of(const ConvShape &s, size_t i)
{
    if (s.tnc) return i;
    const size_t bc = i / s.Lout, t = i - bc * s.Lout, b = bc / s.Cout, co = bc - b * s.Cout;
    return (t * s.n + b) * s.Cout + co;
}

// z and y in their layout from the product's rows
__global__ __launch_bounds__(256) void conv_swish_kernel(const float *zr, ConvShape s, size_t count, float *z, float *y)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float zv = zr[row_of(s, i)] + 0.0f;
    z[i] = zv;
    y[i] = swish(zv) + 0.0f;
}

// dz as rows from dy and z in their layout
__global__ __launch_bounds__(256) void conv_dz_kernel(const float *dy, const float *z, ConvShape s, size_t count, float *dzr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    dzr[row_of(s, i)] = dy[i] * swish_grad(z[i]) + 0.0f;
}

// dx[b, ci, p] = sum over k ascending of dcol[row t n + b, ci K + k] where t stride + k - pad = p: at most ceil(K / stride) terms
__global__ __launch_bounds__(256) void conv_col2im_kernel(const float *dcol, ConvShape s, size_t count, float *dx)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const size_t bc = i / s.Lin;
    const long p = (long)(i - bc * s.Lin);
    const int b = (int)(bc / s.Cin), ci = (int)(bc - (size_t)b * s.Cin), CK = s.Cin * s.K;
    float acc = 0.0f;
    for (int k = 0; k < s.K; ++k) {
        const long num = p + s.pad - k;
        if (num < 0) break;
        if (num % s.stride) continue;
        const long t = num / s.stride;
        if (t < s.Lout) acc = acc + dcol[((size_t)t * s.n + b) * CK + ci * s.K + k];
    }
    dx[i] = acc + 0.0f;
}

ConvShape shape_of(int n, int Cin, int Lin, int Cout, int K, int stride, int tnc)
{
    return ConvShape{n, Cin, Cout, K, stride, K / 2, tnc ? 1 : 0, (long)Lin, xb::conv_out_len(Lin, K, stride)};
}

inline unsigned blocks_of(size_t count) { return (unsigned)((count + 255) / 256); }

template <typename Fn4, typename Fn8, typename Fn16>
void by_width(int Cout, Fn4 f4, Fn8 f8, Fn16 f16)
{
    if (Cout <= 4) f4();
    else if (Cout <= 8) f8();
    else f16();
}

const char *check_args(const xb_ctx *ctx, int n, int Cin, int Lin, int Cout, int K, int stride, std::initializer_list<const void *> ptrs, char *msg,
                       size_t msg_len)
{
    for (const void *p : ptrs) {
        if (!p) return "null device pointer";
        if (reinterpret_cast<uintptr_t>(p) & 15) {
            snprintf(msg, msg_len, "device pointer %p is not 16-byte aligned", p);
            return msg;
        }
    }
    const long Lout = n >= 1 && Cin >= 1 && Lin >= 1 && Cout >= 1 && K >= 1 && stride >= 1 ? xb::conv_out_len(Lin, K, stride) : 0;
    const bool sizes = Lout >= 1 && (long)Cin * K <= xb::CONV_MAX_CK;
    // every tensor of the call, col included, below 2^38 elements: the element kernels' grids and the products' row counts
    const double most = sizes ? std::max({(double)n * Cin * Lin, (double)n * Cout * (double)Lout, (double)n * Lout * ((double)Cin * K)}) : 0.0;
    if (!sizes || most >= 274877906944.0) {
        snprintf(msg, msg_len, "n = %d, Cin = %d, Lin = %d, Cout = %d, K = %d, stride = %d; accepted: each >= 1, Cin K <= %d, every tensor (col (Lout n, Cin K) "
                 "included) below 2^38 elements", n, Cin, Lin, Cout, K, stride, xb::CONV_MAX_CK);
        return msg;
    }
    return nullptr;
}

}  // namespace

namespace xb {

int conv_forward_run(xb_ctx *ctx, const float *x, const float *w, const float *bias, int n, int Cin, int Lin, int Cout, int K, int stride, int tnc,
                     float *z, float *y, float *col_keep)
{
    const ConvShape s = shape_of(n, Cin, Lin, Cout, K, stride, tnc);
    if (conv_is_narrow(Cin, Cout, K, stride)) {
        const int tiles = (int)((s.Lout + TL - 1) / TL);
        const dim3 grid((unsigned)((size_t)tiles * n));
        by_width(Cout, [&] { conv_narrow_fwd_kernel<4><<<grid, 256, 0, ctx->stream>>>(x, w, bias, s, tiles, z, y); },
                 [&] { conv_narrow_fwd_kernel<8><<<grid, 256, 0, ctx->stream>>>(x, w, bias, s, tiles, z, y); },
                 [&] { conv_narrow_fwd_kernel<16><<<grid, 256, 0, ctx->stream>>>(x, w, bias, s, tiles, z, y); });
        return launched(ctx, "xb_conv_train_forward");
    }
    const int CK = Cin * K;
    const size_t rows = (size_t)s.Lout * n;
    const ConvWide ws = conv_wide(rows, CK, Cout);
    if (int rc = grow(ctx, &ctx->convtrain.ws, ws.forward_floats * sizeof(float))) return rc;
    float *base = static_cast<float *>(ctx->convtrain.ws.p), *zr = base + ws.dz, *col = col_keep ? col_keep : base + ws.col;
    conv_im2col_kernel<<<blocks_of(rows * CK), 256, 0, ctx->stream>>>(x, s, rows * CK, col);
    if (int rc = launched(ctx, "xb_conv_train_forward")) return rc;
    if (int rc = linear_f32_run(ctx, col, w, bias, (int64_t)rows, Cout, CK, 0, 1.0f, zr)) return rc;
    conv_swish_kernel<<<blocks_of(rows * Cout), 256, 0, ctx->stream>>>(zr, s, rows * Cout, z, y);
    return launched(ctx, "xb_conv_train_forward");
}

int conv_backward_run(xb_ctx *ctx, const float *dy, const float *x, const float *z, const float *w, int n, int Cin, int Lin, int Cout, int K,
                      int stride, int tnc, float *dx, float *dw, float *db, const float *col_kept)
{
    const ConvShape s = shape_of(n, Cin, Lin, Cout, K, stride, tnc);
    if (conv_is_narrow(Cin, Cout, K, stride)) {
        const ConvNarrow c = conv_narrow(n, Cin, Lin, Cout, K);
        if (int rc = grow(ctx, &ctx->convtrain.part, c.scratch_doubles * sizeof(double))) return rc;
        double *part = static_cast<double *>(ctx->convtrain.part.p);
        const int tiles = (int)c.tiles;
        const dim3 grid((unsigned)c.blocks);
        by_width(Cout, [&] { conv_narrow_bwd_kernel<4><<<grid, 256, 0, ctx->stream>>>(dy, x, z, w, s, tiles, dx, part); },
                 [&] { conv_narrow_bwd_kernel<8><<<grid, 256, 0, ctx->stream>>>(dy, x, z, w, s, tiles, dx, part); },
                 [&] { conv_narrow_bwd_kernel<16><<<grid, 256, 0, ctx->stream>>>(dy, x, z, w, s, tiles, dx, part); });
        if (int rc = launched(ctx, "xb_conv_train_backward")) return rc;
        const int nw = Cout * Cin * K, outputs = (int)c.outputs;
        conv_narrow_sum_kernel<<<(unsigned)((outputs + 63) / 64), 64, 0, ctx->stream>>>(part, c.blocks, nw, outputs, dw, db);
        return launched(ctx, "xb_conv_train_backward");
    }
    const int CK = Cin * K;
    const size_t rows = (size_t)s.Lout * n;
    const ConvWide ws = conv_wide(rows, CK, Cout);
    if (int rc = grow(ctx, &ctx->convtrain.ws, ws.backward_floats * sizeof(float))) return rc;
    float *base = static_cast<float *>(ctx->convtrain.ws.p), *dzr = base + ws.dz, *dcol = base + ws.dcol, *wt = base + ws.wt;
    const float *col = col_kept;
    if (!col) {
        conv_im2col_kernel<<<blocks_of(rows * CK), 256, 0, ctx->stream>>>(x, s, rows * CK, base + ws.col);
        col = base + ws.col;
    }
    conv_dz_kernel<<<blocks_of(rows * Cout), 256, 0, ctx->stream>>>(dy, z, s, rows * Cout, dzr);
    if (int rc = launched(ctx, "xb_conv_train_backward")) return rc;
    if (int rc = wgrad_f32_run(ctx, dzr, col, (int64_t)rows, Cout, CK, dw, db)) return rc;
    if (!dx) return XB_OK;
    if (int rc = transpose_run(ctx, w, Cout, CK, wt)) return rc;
    if (int rc = linear_f32_run(ctx, dzr, wt, nullptr, (int64_t)rows, CK, Cout, 0, 1.0f, dcol)) return rc;
    const size_t count = (size_t)n * Cin * Lin;
    conv_col2im_kernel<<<blocks_of(count), 256, 0, ctx->stream>>>(dcol, s, count, dx);
    return launched(ctx, "xb_conv_train_backward");
}

}  // namespace xb

extern "C" {

XB_API int xb_conv_train_forward_dev(xb_ctx *ctx, const float *d_x, const float *d_w, const float *d_b, int n, int Cin, int Lin, int Cout, int K,
                                     int stride, int tnc, float *d_z, float *d_y)
{
    if (!ctx) return XB_ERR_INVALID;
    char msg[320];
    if (const char *why = check_args(ctx, n, Cin, Lin, Cout, K, stride, {d_x, d_w, d_b, d_z, d_y}, msg, sizeof msg))
        return fail(ctx, XB_ERR_INVALID, "xb_conv_train_forward: %s", why);
    if (int rc = enter(ctx, true)) return rc;
    return xb::conv_forward_run(ctx, d_x, d_w, d_b, n, Cin, Lin, Cout, K, stride, tnc, d_z, d_y, nullptr);
}

XB_API int xb_conv_train_backward_dev(xb_ctx *ctx, const float *d_dy, const float *d_x, const float *d_z, const float *d_w, int n, int Cin, int Lin,
                                      int Cout, int K, int stride, int tnc, float *d_dx, float *d_dw, float *d_db)
{
    if (!ctx) return XB_ERR_INVALID;
    char msg[320];
    if (const char *why = check_args(ctx, n, Cin, Lin, Cout, K, stride, {d_dy, d_x, d_z, d_w, d_dw, d_db}, msg, sizeof msg))
        return fail(ctx, XB_ERR_INVALID, "xb_conv_train_backward: %s", why);
    if (reinterpret_cast<uintptr_t>(d_dx) & 15) return fail(ctx, XB_ERR_INVALID, "xb_conv_train_backward: device pointer %p is not 16-byte aligned", (void *)d_dx);
    if (int rc = enter(ctx, true)) return rc;
    return xb::conv_backward_run(ctx, d_dy, d_x, d_z, d_w, n, Cin, Lin, Cout, K, stride, tnc, d_dx, d_dw, d_db, nullptr);
}

}  // extern "C"
