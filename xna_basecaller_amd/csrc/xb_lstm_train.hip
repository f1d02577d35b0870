// xb_lstm_train.hip -- one LSTM layer's recurrence for training: the forward that keeps what the backward needs (activated
// gates, cell states) and the backward through time.  The contracts are in the public header (xb_lstm_train_forward_dev,
// xb_lstm_train_backward_dev).  One launch per time step: the step boundary is the launch boundary, no workgroup waits for
// another inside a kernel (the inference recurrence of xb_lstm.hip is persistent; this one deliberately is not).  fp32
// throughout; the products run on the f32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain per output element, exact
// f32 operands), so a row's results depend on that row alone and a gradient of 1e-9 needs no scaling.  Built without
// contraction, division correctly rounded: the activations are the same operations in the forward and in the backward.
#include "xb_ctx.h"
#include "xb_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int JB = 16;          // hidden units of one workgroup: one MFMA tile of columns (per gate)
constexpr int LDP = JB + 1;     // floats per LDS row: the element pass reads 16 rows x 16 columns without a bank conflict

// One wave's share of a product: for RT tiles of 16 rows, acc[rt] += A[rows, k] * B[16 columns, k]^T over nk chunks of 16 k.
// Both operands are k-contiguous in memory (16 floats of a row per chunk, a float4 per lane); lane (r = lane & 15, q = lane >> 4)
// holds k = 16 kc + 4 q + m in its element m, and MFMA m of the chunk sums over the four q -- every k once, in an order that
// depends on nothing but nk.  Chunks alternate between two accumulators (the instruction's dependent latency is longer than
// its issue interval); the caller adds the two.  Rows past n are not computed (their tiles) or are copies of row n - 1 (a
// ragged tile: the caller does not store them).
template <int RT>
__device__ __forceinline__ void wave_product(const float *a_base, size_t lda, const float *b_row, int nk, int r0, int n, int lane,
                                             f32x4 (&acc0)[RT], f32x4 (&acc1)[RT])
{
    const int r = lane & 15, q = lane >> 4;
    const float *a_row[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int row = min(r0 + rt * 16 + r, n - 1);
        a_row[rt] = a_base + (size_t)row * lda + q * 4;
    }
    b_row += q * 4;
    // U chunks at a time, every load of the group issued before its first MFMA: a step is a chain of nk dependent
    // load -> MFMA rounds otherwise, and the loads' latency, not the MFMAs, is its time.  Even chunks go to acc0, odd to acc1,
    // in ascending order in the groups as in the tail: the sums do not depend on U.
    constexpr int U = RT == 1 ? 8 : 4;
    int kc = 0;
    for (; kc + U <= nk; kc += U) {
        f32x4 bv[U], av[RT][U];
#pragma unroll
        for (int u = 0; u < U; ++u) bv[u] = *reinterpret_cast<const f32x4 *>(b_row + (kc + u) * 16);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            if (r0 + rt * 16 < n) {                                     // the same for the whole workgroup
#pragma unroll
                for (int u = 0; u < U; ++u) av[rt][u] = *reinterpret_cast<const f32x4 *>(a_row[rt] + (kc + u) * 16);
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                if (r0 + rt * 16 < n) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        if (u & 1) acc1[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][u][m], bv[u][m], acc1[rt], 0, 0, 0);
                        else acc0[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][u][m], bv[u][m], acc0[rt], 0, 0, 0);
                    }
                }
    }
    for (; kc < nk; ++kc) {                                             // kc starts even here: U is
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(b_row + kc * 16);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            if (r0 + rt * 16 < n) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(a_row[rt] + kc * 16);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (kc & 1) acc1[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[m], acc1[rt], 0, 0, 0);
                    else acc0[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[m], acc0[rt], 0, 0, 0);
                }
            }
    }
}

struct FwdArgs {
    const float *gin_t;            // (n, 4F) of this step
    const float *w;                // (4F, F) weight_hh_l0
    const float *h_prev, *c_prev;  // (n, F) of the step processed before; both null at the first one (h = c = 0)
    float *y_t, *gates_t, *c_t;    // (n, F), (n, 4F), (n, F) of this step
    int n, F;
};

// Workgroup (blockIdx.x: RT * 16 rows, blockIdx.y: 16 hidden units j), four waves: wave g computes gate g's columns of
// h_prev W_hh^T over K = F, adds gin, applies the activation, stores the gate and leaves it in LDS; then all 256 threads form
// c and y of the tile's elements.
template <int RT>
__global__ __launch_bounds__(256) void lstm_train_fwd_kernel(FwdArgs a)
{
    __shared__ float act[4][RT * 16][LDP];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, col = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * RT * 16, j0 = blockIdx.y * JB, F = a.F, n = a.n;
    const size_t G = (size_t)4 * F;
    f32x4 acc0[RT], acc1[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc0[rt] = acc1[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (a.h_prev) wave_product<RT>(a.h_prev, (size_t)F, a.w + ((size_t)g * F + j0 + col) * F, F / 16, r0, n, lane, acc0, acc1);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = rt * 16 + q * 4 + i, row = r0 + rl;
            float v = 0.0f;
            if (row < n) {
                const size_t at = (size_t)row * G + (size_t)g * F + j0 + col;
                const float pre = a.gin_t[at] + (acc0[rt][i] + acc1[rt][i]);
                v = g == 2 ? lt_tanh(pre) : lt_sigmoid(pre);
                a.gates_t[at] = v;
            }
            act[g][rl][col] = v;
        }
    __syncthreads();
    for (int e = threadIdx.x; e < RT * 256; e += 256) {
        const int rl = e >> 4, jj = e & 15, row = r0 + rl;
        if (row >= n) continue;
        const size_t at = (size_t)row * F + j0 + jj;
        const float cp = a.c_prev ? a.c_prev[at] : 0.0f;
        const float c = __builtin_fmaf(act[1][rl][jj], cp, act[0][rl][jj] * act[2][rl][jj]);
        a.c_t[at] = c;
        a.y_t[at] = act[3][rl][jj] * lt_tanh(c);
    }
}

struct BwdArgs {
    const float *dy_t, *gates_t, *c_t;   // (n, F), (n, 4F), (n, F) of this step
    const float *c_prev;                 // (n, F) of the step the forward processed before this one; null at its first
    const float *dgin_s;                 // (n, 4F): dgin of the step the forward processed after this one; null at its last
    const float *wt;                     // (F, 4F): W_hh transposed
    float *dgin_t;                       // (n, 4F)
    float *carry;                        // (n, F): dc * f of the step processed before (not read where dgin_s is null), replaced
    int n, F;
};

// The same workgroup shape.  Wave g sums dgin[s] W_hh[:, j-block] over the K = F rows of gate g, the four partial tiles meet
// in LDS and are added in gate order; then every thread runs the chain of the header on its elements.  An element of the
// carry is read and written by the one thread that owns it.  Zeros are written as +0 (x + 0.0f): a gradient of zeros gives
// zero bytes whatever the signs of the stashed activations.
template <int RT>
__global__ __launch_bounds__(256) void lstm_train_bwd_kernel(BwdArgs a)
{
    __shared__ float part[4][RT * 16][LDP];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, col = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * RT * 16, j0 = blockIdx.y * JB, F = a.F, n = a.n;
    const size_t G = (size_t)4 * F;
    if (a.dgin_s) {
        f32x4 acc0[RT], acc1[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc0[rt] = acc1[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        wave_product<RT>(a.dgin_s + (size_t)g * F, G, a.wt + (size_t)(j0 + col) * G + (size_t)g * F, F / 16, r0, n, lane, acc0, acc1);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) part[g][rt * 16 + q * 4 + i][col] = acc0[rt][i] + acc1[rt][i];
        __syncthreads();
    }
    for (int e = threadIdx.x; e < RT * 256; e += 256) {
        const int rl = e >> 4, jj = e & 15, row = r0 + rl;
        if (row >= n) continue;
        const size_t at = (size_t)row * F + j0 + jj, ag = (size_t)row * G + j0 + jj;
        float dh = a.dy_t[at], carry = 0.0f;
        if (a.dgin_s) {
            dh += (part[0][rl][jj] + part[1][rl][jj]) + (part[2][rl][jj] + part[3][rl][jj]);
            carry = a.carry[at];
        }
        const float gi = a.gates_t[ag], gf = a.gates_t[ag + F], gg = a.gates_t[ag + 2 * (size_t)F], go = a.gates_t[ag + 3 * (size_t)F];
        const float cp = a.c_prev ? a.c_prev[at] : 0.0f;
        const float th = lt_tanh(a.c_t[at]);
        const float d_o = dh * th;
        const float dc = __builtin_fmaf(dh * go, (1.0f - th) * (1.0f + th), carry);
        a.carry[at] = dc * gf;
        a.dgin_t[ag] = (dc * gg) * (gi * (1.0f - gi)) + 0.0f;
        a.dgin_t[ag + F] = (dc * cp) * (gf * (1.0f - gf)) + 0.0f;
        a.dgin_t[ag + 2 * (size_t)F] = (dc * gi) * ((1.0f - gg) * (1.0f + gg)) + 0.0f;
        a.dgin_t[ag + 3 * (size_t)F] = d_o * (go * (1.0f - go)) + 0.0f;
    }
}

// w (R, C) -> wt (C, R), both dimensions multiples of 16
__global__ __launch_bounds__(256) void lstm_train_transpose_kernel(const float *w, float *wt, int R, int C)
{
    __shared__ float tile[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    tile[ty][tx] = w[((size_t)blockIdx.y * 16 + ty) * C + blockIdx.x * 16 + tx];
    __syncthreads();
    wt[((size_t)blockIdx.x * 16 + ty) * R + blockIdx.y * 16 + tx] = tile[tx][ty];
}

int check_shape(xb_ctx *ctx, const char *who, int T, int n, int F, std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs) {
        if (!p) return fail(ctx, XB_ERR_INVALID, "%s: null device pointer", who);
        if (reinterpret_cast<uintptr_t>(p) & 15) return fail(ctx, XB_ERR_INVALID, "%s: device pointer %p is not 16-byte aligned", who, p);
    }
    if (T < 1 || n < 1 || F < 16 || F > 1024 || F % 16)
        return fail(ctx, XB_ERR_INVALID, "%s: T = %d, n = %d, F = %d; accepted: T >= 1, n >= 1, F a multiple of 16 in 16 .. 1024", who, T, n, F);
    return XB_OK;
}

// rows of one workgroup: one 16-row tile up to 64 rows, four above (the weights' fragment is then used four times).  A row's
// arithmetic is the same either way.
inline int row_tiles(int n) { return n <= 64 ? 1 : 4; }

}  // namespace

extern "C" {

XB_API int xb_lstm_train_forward_dev(xb_ctx *ctx, const float *d_gin, const float *d_w_hh, int T, int n, int F, int reverse, float *d_y,
                                     float *d_gates, float *d_c)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_shape(ctx, "xb_lstm_train_forward", T, n, F, {d_gin, d_w_hh, d_y, d_gates, d_c})) return rc;
    if (int rc = enter(ctx, true)) return rc;
    const size_t nF = (size_t)n * F;
    const int rt = row_tiles(n);
    const dim3 grid((unsigned)((n + rt * 16 - 1) / (rt * 16)), (unsigned)(F / JB));
    for (int step = 0; step < T; ++step) {
        const size_t t = reverse ? (size_t)(T - 1 - step) : (size_t)step, tp = reverse ? t + 1 : t - 1;
        FwdArgs a;
        a.gin_t = d_gin + t * 4 * nF; a.w = d_w_hh;
        a.h_prev = step ? d_y + tp * nF : nullptr; a.c_prev = step ? d_c + tp * nF : nullptr;
        a.y_t = d_y + t * nF; a.gates_t = d_gates + t * 4 * nF; a.c_t = d_c + t * nF;
        a.n = n; a.F = F;
        if (rt == 1) hipLaunchKernelGGL(lstm_train_fwd_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(lstm_train_fwd_kernel<4>, grid, dim3(256), 0, ctx->stream, a);
    }
    return launched(ctx, "xb_lstm_train_forward");
}

XB_API int xb_lstm_train_backward_dev(xb_ctx *ctx, const float *d_dy, const float *d_w_hh, const float *d_gates, const float *d_c, int T,
                                      int n, int F, int reverse, float *d_dgin)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_shape(ctx, "xb_lstm_train_backward", T, n, F, {d_dy, d_w_hh, d_gates, d_c, d_dgin})) return rc;
    if (int rc = enter(ctx, true)) return rc;
    const size_t nF = (size_t)n * F;
    if (int rc = grow(ctx, &ctx->lstmtrain.carry, nF * sizeof(float))) return rc;
    if (int rc = grow(ctx, &ctx->lstmtrain.wt, (size_t)4 * F * F * sizeof(float))) return rc;
    float *wt = static_cast<float *>(ctx->lstmtrain.wt.p);
    if (T > 1) hipLaunchKernelGGL(lstm_train_transpose_kernel, dim3((unsigned)(F / 16), (unsigned)(4 * F / 16)), dim3(256), 0, ctx->stream, d_w_hh, wt, 4 * F, F);
    const int rt = row_tiles(n);
    const dim3 grid((unsigned)((n + rt * 16 - 1) / (rt * 16)), (unsigned)(F / JB));
    for (int step = T - 1; step >= 0; --step) {                            // step: the forward's processing order
        const size_t t = reverse ? (size_t)(T - 1 - step) : (size_t)step;
        const size_t tp = reverse ? t + 1 : t - 1, ts = reverse ? t - 1 : t + 1;
        BwdArgs a;
        a.dy_t = d_dy + t * nF; a.gates_t = d_gates + t * 4 * nF; a.c_t = d_c + t * nF;
        a.c_prev = step ? d_c + tp * nF : nullptr;
        a.dgin_s = step < T - 1 ? d_dgin + ts * 4 * nF : nullptr;
        a.wt = wt; a.dgin_t = d_dgin + t * 4 * nF; a.carry = static_cast<float *>(ctx->lstmtrain.carry.p);
        a.n = n; a.F = F;
        if (rt == 1) hipLaunchKernelGGL(lstm_train_bwd_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(lstm_train_bwd_kernel<4>, grid, dim3(256), 0, ctx->stream, a);
    }
    return launched(ctx, "xb_lstm_train_backward");
}

}  // extern "C"
