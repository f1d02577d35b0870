// xb_top.hip -- training the CRF head together with the top L LSTM layers, everything below them frozen: `bonito train -F` at
// --num-unfreeze-top 2 .. 6 with --no-amp.  The frozen bottom is the inference encoder's own pass, cut off after 5 - L LSTM
// layers (encoder_bottom_run, xb_run_encoder.hip) and joined into fp32; from there on a step is the chain tests/toptrain_dev.py
// composes -- the fp32 products of xb_train_gemm.hip, the training recurrence of xb_lstm_train.hip, xb_ctc_loss_grad, the norm and
// AdamW of xb_head.hip -- on the buffers csrc/xb_top_plan.h lays out, in one call.  Three small kernels of its own: the join of
// the two fp16 planes, an exact transpose, the sum of a layer's two biases.  xb_full_train_begin opens the same trainer at L = 5
// with the three convolutions trained as well (`bonito train --no-amp` without -f): their training forwards (xb_conv_train.hip)
// stand in for the frozen bottom, their backwards follow the lowest LSTM layer's, on the buffers csrc/xb_conv_plan.h adds in
// front of and behind the plan's.  The contracts are in the public header.  Built without contraction, as the translation
// units it chains.
#include "xb_ctx.h"
#include "xb_head_train.h"
#include "xb_top_plan.h"
#include "xb_train_gemm.h"
#include "xb_conv_plan.h"
#include "xb_conv_train.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// out = (float)hi + (float)lo, one fp32 addition: eight elements a thread (16 bytes of each plane in, two 16-byte stores out),
// the last count % 8 elements one by one
__global__ __launch_bounds__(256) void top_join_kernel(const half_t *hi, const half_t *lo, size_t count, float *out)
{
    const size_t at = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (at + 8 <= count) {
        const half8 h = *reinterpret_cast<const half8 *>(hi + at), l = *reinterpret_cast<const half8 *>(lo + at);
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = (float)h[j] + (float)l[j];
            b[j] = (float)h[4 + j] + (float)l[4 + j];
        }
        *reinterpret_cast<f32x4 *>(out + at) = a;
        *reinterpret_cast<f32x4 *>(out + at + 4) = b;
    } else {
        for (size_t i = at; i < count; ++i) out[i] = (float)hi[i] + (float)lo[i];
    }
}

// out (cols, rows) = in (rows, cols)^T through a 32 x 32 tile whose rows are padded by one float, so that the column-wise reads
// of the second half fall into 32 different banks
constexpr int TT = 32;
__global__ __launch_bounds__(256) void top_transpose_kernel(const float *in, int rows, int cols, float *out)
{
    __shared__ float tile[TT][TT + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * TT, c0 = blockIdx.x * TT;
#pragma unroll
    for (int k = 0; k < TT; k += 8) {
        const int r = r0 + ty + k, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + k][tx] = in[(size_t)r * cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TT; k += 8) {
        const int c = c0 + ty + k, r = r0 + tx;
        if (c < cols && r < rows) out[(size_t)c * rows + r] = tile[tx][ty + k];
    }
}

// b = b_ih + b_hh, one rounding
__global__ __launch_bounds__(256) void top_bias_sum_kernel(const float *b_ih, const float *b_hh, int len, float *b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < len) b[i] = b_ih[i] + b_hh[i];
}

int join_run(xb_ctx *ctx, const half_t *hi, const half_t *lo, size_t count, float *out)
{
    top_join_kernel<<<(unsigned)((count + 2047) / 2048), 256, 0, ctx->stream>>>(hi, lo, count, out);
    return launched(ctx, "xb_encode_bottom");
}

}  // namespace

int xb::transpose_run(xb_ctx *ctx, const float *in, int rows, int cols, float *out)
{
    top_transpose_kernel<<<dim3((unsigned)((cols + TT - 1) / TT), (unsigned)((rows + TT - 1) / TT)), 256, 0, ctx->stream>>>(in, rows, cols, out);
    return launched(ctx, "xb_transpose_f32");
}

namespace {

using xb::transpose_run;

int bias_sum_run(xb_ctx *ctx, const float *b_ih, const float *b_hh, int len, float *b)
{
    top_bias_sum_kernel<<<(unsigned)((len + 255) / 256), 256, 0, ctx->stream>>>(b_ih, b_hh, len, b);
    return launched(ctx, "xb_top_train_grad");
}

// the fp16 residual as second part of a layer output exists where the head's rule holds (head_usable): these two precisions
int bottom_usable(xb_ctx *ctx, const char *who)
{
    if (ctx->cfg.precision != XB_PREC_MIXED && ctx->cfg.precision != XB_PREC_F16X3)
        return fail(ctx, XB_ERR_INVALID, "%s: the layer outputs of this context carry no fp16 residual; create it with precision mixed or f16x3", who);
    return XB_OK;
}

// the bottom pass of `layers` LSTM layers and its output as fp32 (T, n, F)
int bottom_run(xb_ctx *ctx, const float *d_signal, int n, int layers, float *d_x0)
{
    if (int rc = encoder_bottom_run(ctx, d_signal, n, layers)) return rc;
    return join_run(ctx, ctx->x_hi[layers & 1], ctx->x_lo[layers & 1], (size_t)ctx->T * n * ctx->cfg.features, d_x0);
}

xb::TopPlan plan_of(const xb_ctx *ctx) { return xb::top_plan(ctx->top.L, ctx->cfg.features, ctx->O); }
xb::ConvPlan conv_plan_of(const xb_ctx *ctx) { return xb::conv_plan(ctx->cfg.chunk_len, ctx->cfg.features, ctx->cfg.winlen, ctx->cfg.stride); }

// floats of one flat buffer and from one buffer to the next; conv: the floats of the conv section in front (0: none)
size_t flat_stride(size_t conv, const xb::TopPlan &pl) { return (conv + pl.params + 3) & ~(size_t)3; }

// the trainer's buffers: four strides of the flat layout -- the conv section of a full trainer, then the plan's -- and the small
// buffer: the norm | the summed biases | a turned weight.  tp, tg: where the plan's section starts in p and g.
struct TopBuf {
    float *p, *g, *m, *v, *tp, *tg, *norm, *bias, *turned, *act;
    size_t params;
    TopBuf(xb_ctx *ctx, const xb::TopPlan &pl)
    {
        const size_t conv = ctx->top.full ? conv_plan_of(ctx).params : 0, stride = flat_stride(conv, pl);
        params = conv + pl.params;
        p = static_cast<float *>(ctx->top.train.p);
        g = p + stride; m = g + stride; v = m + stride;
        tp = p + conv; tg = g + conv;
        norm = static_cast<float *>(ctx->top.small.p);
        bias = norm + 64; turned = bias + pl.bias_sum;
        act = static_cast<float *>(ctx->top.act.p);
    }
};

int top_nomem(xb_ctx *ctx, const char *who, const xb::TopPlan &pl, size_t rows)
{
    double bytes = (double)pl.step_bytes(rows);
    if (ctx->top.full) {
        const xb::ConvPlan cp = conv_plan_of(ctx);
        bytes += sizeof(float) * (double)(cp.act(rows / (size_t)ctx->T).floats + 4 * cp.params);
    }
    return fail(ctx, XB_ERR_NOMEM, "%s: a step of %zu rows with %d unfrozen LSTM layers%s needs %.2f GB on the device beside the context's "
                "workspaces, and an allocation failed; lower the batch", who, rows, pl.L, ctx->top.full ? " and the convolutions" : "", bytes / 1e9);
}

// floats of a step's activations: the plan's, and behind them (from a 16-byte boundary) a full trainer's conv activations
size_t conv_act_at(const xb::TopPlan &pl, size_t rows) { return xb::conv_round4(pl.act_floats(rows)); }
size_t act_floats(const xb_ctx *ctx, const xb::TopPlan &pl, size_t rows)
{
    return ctx->top.full ? conv_act_at(pl, rows) + conv_plan_of(ctx).act(rows / (size_t)ctx->T).floats : pl.act_floats(rows);
}

// One gradient of the step: everything up to the norm.  The caller has validated, entered and staged the batch.
int top_grad_run(xb_ctx *ctx, const char *who, int n, const uint8_t *d_targets, int Lt, const int32_t *d_len, float *d_loss)
{
    const xb::TopPlan pl = plan_of(ctx);
    const TopBuf b(ctx, pl);
    const int L = pl.L, F = pl.F, C = pl.C, T = ctx->T;
    const size_t rows = (size_t)T * n;
    const float scale = ctx->cfg.scale;
    float *x0 = b.act + pl.x0(rows), *gin = b.act + pl.gin(rows), *dy = b.act + pl.dy(rows), *dgin = b.act + pl.dgin(rows);
    float *scores = b.act + pl.scores(rows), *dscores = b.act + pl.dscores(rows), *dz = b.act + pl.dz(rows);
    auto rev_of = [&](int i) { return (pl.layer_index(i) - 4) % 2 == 0 ? 1 : 0; };      // LSTM layer index even: backwards in time

    // a full trainer: the three conv forwards in place of the frozen bottom, conv3 writing x0 as (T, n, F)
    const xb::ConvPlan cp = conv_plan_of(ctx);
    const xb::ConvAct ca = cp.act((size_t)n);
    float *cv = ctx->top.full ? b.act + conv_act_at(pl, rows) : nullptr;
    const int L1 = (int)cp.L1, L2 = (int)cp.L2, C1 = xb::CONV_C1, C2 = xb::CONV_C2, K12 = xb::CONV_K12;
    if (ctx->top.full) {
        if (int rc = xb::conv_forward_run(ctx, ctx->d_signal, b.p + cp.off[0], b.p + cp.off[1], n, 1, cp.chunk, C1, K12, 1, 0, cv + ca.z1, cv + ca.y1, nullptr)) return rc;
        if (int rc = xb::conv_forward_run(ctx, cv + ca.y1, b.p + cp.off[2], b.p + cp.off[3], n, C1, L1, C2, K12, 1, 0, cv + ca.z2, cv + ca.y2, nullptr)) return rc;
        if (int rc = xb::conv_forward_run(ctx, cv + ca.y2, b.p + cp.off[4], b.p + cp.off[5], n, C2, L2, F, cp.W, cp.S, 1, cv + ca.z3, x0, cv + ca.col)) return rc;
    } else if (int rc = bottom_run(ctx, ctx->d_signal, n, pl.bottom_layers(), x0)) return rc;
    const float *x = x0;
    for (int i = 0; i < L; ++i) {
        const size_t *o = pl.layer(i);
        float *bias = b.bias + (size_t)i * 4 * F;
        if (int rc = bias_sum_run(ctx, b.tp + o[2], b.tp + o[3], 4 * F, bias)) return rc;
        if (int rc = xb::linear_f32_run(ctx, x, b.tp + o[0], bias, (int64_t)rows, 4 * F, F, 0, 1.0f, gin)) return rc;
        float *y = b.act + pl.y(rows, i);
        if (int rc = xb_lstm_train_forward_dev(ctx, gin, b.tp + o[1], T, n, F, rev_of(i), y, b.act + pl.gates(rows, i), b.act + pl.c(rows, i))) return rc;
        x = y;
    }
    if (int rc = xb::linear_f32_run(ctx, x, b.tp + pl.head_w(), b.tp + pl.head_b(), (int64_t)rows, C, F, 1, scale, scores)) return rc;
    if (int rc = ctc_grad_run(ctx, who, scores, T, n, 0, C, d_targets, Lt, d_len, 0.0f, 1, d_loss, dscores)) return rc;
    if (int rc = xb::head_dz_run(ctx, scores, dscores, (int64_t)(rows * C), scale, dz)) return rc;
    if (int rc = xb::wgrad_f32_run(ctx, dz, x, (int64_t)rows, C, F, b.tg + pl.head_w(), b.tg + pl.head_b())) return rc;
    if (int rc = transpose_run(ctx, b.tp + pl.head_w(), C, F, b.turned)) return rc;
    if (int rc = xb::linear_f32_run(ctx, dz, b.turned, nullptr, (int64_t)rows, F, C, 0, 1.0f, dy)) return rc;      // the head's dX = dZ W
    for (int i = L - 1; i >= 0; --i) {
        const size_t *o = pl.layer(i);
        const int rev = rev_of(i);
        const float *y = b.act + pl.y(rows, i), *xin = i ? b.act + pl.y(rows, i - 1) : x0;
        if (int rc = xb_lstm_train_backward_dev(ctx, dy, b.tp + o[1], b.act + pl.gates(rows, i), b.act + pl.c(rows, i), T, n, F, rev, dgin)) return rc;
        if (int rc = xb::wgrad_f32_run(ctx, dgin, xin, (int64_t)rows, 4 * F, F, b.tg + o[0], b.tg + o[2])) return rc;       // dW_ih and db
        XB_HIP(ctx, hipMemcpyAsync(b.tg + o[3], b.tg + o[2], sizeof(float) * 4 * F, hipMemcpyDeviceToDevice, ctx->stream));  // both biases receive it
        // dW_hh = sum_t dgin[t]^T y[the step processed before t]: the operands shifted against each other by one time step
        const float *wa = dgin + (rev ? (size_t)0 : (size_t)n * 4 * F), *wb = y + (rev ? (size_t)n * F : (size_t)0);
        if (int rc = xb::wgrad_f32_run(ctx, wa, wb, (int64_t)(T - 1) * n, 4 * F, F, b.tg + o[1], nullptr)) return rc;
        if (i || ctx->top.full) {                                                                                           // dx = dgin W_ih: the dy of the layer below
            if (int rc = transpose_run(ctx, b.tp + o[0], 4 * F, F, b.turned)) return rc;
            if (int rc = xb::linear_f32_run(ctx, dgin, b.turned, nullptr, (int64_t)rows, F, 4 * F, 0, 1.0f, dy)) return rc;
        }
    }
    if (ctx->top.full) {                                    // dy is d loss / d x0 in conv3's (T, n, F) layout; conv1's input has no gradient
        if (int rc = xb::conv_backward_run(ctx, dy, cv + ca.y2, cv + ca.z3, b.p + cp.off[4], n, C2, L2, F, cp.W, cp.S, 1, cv + ca.dy2, b.g + cp.off[4], b.g + cp.off[5], cv + ca.col)) return rc;
        if (int rc = xb::conv_backward_run(ctx, cv + ca.dy2, cv + ca.y1, cv + ca.z2, b.p + cp.off[2], n, C1, L1, C2, K12, 1, 0, cv + ca.dy1, b.g + cp.off[2], b.g + cp.off[3], nullptr)) return rc;
        if (int rc = xb::conv_backward_run(ctx, cv + ca.dy1, ctx->d_signal, cv + ca.z1, b.p + cp.off[0], n, 1, cp.chunk, C1, K12, 1, 0, nullptr, b.g + cp.off[0], b.g + cp.off[1], nullptr)) return rc;
    }
    return grad_norm_run(ctx, b.g, b.params, nullptr, 0, b.norm);
}

// xb_top_train_grad, and with `step` the update behind it
int top_call(xb_ctx *ctx, const char *who, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, bool step,
             float lr, float *loss, float *grad_norm)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->top.open) return fail(ctx, XB_ERR_STATE, "%s: no trainer is open; call xb_top_train_begin first", who);
    if (int rc = train_call_enter(ctx, who, signal, n, targets, Lt, lengths, step, lr, loss, grad_norm)) return rc;
    const xb::TopPlan pl = plan_of(ctx);
    const size_t N = (size_t)n, rows = (size_t)ctx->T * N;
    if (grow(ctx, &ctx->top.act, act_floats(ctx, pl, rows) * sizeof(float))) {
        ctx->top.rows = 0;                      // the old activations went with the failed allocation
        return top_nomem(ctx, who, pl, rows);
    }
    Staging st{ctx};
    const LabelBatch lb(st, n, Lt);
    if (int rc = st.ready()) return rc;
    ctx->top.rows = rows;
    const TopBuf b(ctx, pl);
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * N * ctx->cfg.chunk_len, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = lb.upload(ctx, targets, lengths)) return rc;
    if (int rc = top_grad_run(ctx, who, n, lb.targets, Lt, lb.len, lb.loss)) return rc;
    float norm = 0.0f, mean = 0.0f;
    if (int rc = train_read_back(ctx, b.norm, lb.loss, n, &norm, &mean)) return rc;
    if (step) {
        if (int rc = train_update(ctx, who, norm, lr, ctx->top.step + 1, b.p, b.g, b.m, b.v, b.params)) return rc;
        ++ctx->top.step;
        if (int rc = xb_synchronize(ctx)) return rc;
    }
    *loss = mean;
    *grad_norm = norm;
    return XB_OK;
}

}  // namespace

extern "C" {

XB_API int xb_encode_bottom_dev(xb_ctx *ctx, const float *d_signal, int n, int layers, float *d_x0)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, n)) return rc;
    if (!d_signal || !d_x0) return fail(ctx, XB_ERR_INVALID, "xb_encode_bottom: null device pointer");
    if (reinterpret_cast<uintptr_t>(d_x0) & 15) return fail(ctx, XB_ERR_INVALID, "xb_encode_bottom: x0 %p is not 16-byte aligned", (void *)d_x0);
    if (layers < 0 || layers > 5) return fail(ctx, XB_ERR_INVALID, "xb_encode_bottom: %d LSTM layers, accepted: 0 .. 5", layers);
    if (int rc = bottom_usable(ctx, "xb_encode_bottom")) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return bottom_run(ctx, d_signal, n, layers, d_x0);
}

XB_API int xb_transpose_f32_dev(xb_ctx *ctx, const float *d_in, int rows, int cols, float *d_out)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_in || !d_out || d_in == d_out) return fail(ctx, XB_ERR_INVALID, "xb_transpose_f32: two different device pointers are needed");
    if (rows < 1 || cols < 1 || (rows + TT - 1) / TT > 65535)
        return fail(ctx, XB_ERR_INVALID, "xb_transpose_f32: rows = %d, cols = %d; accepted: rows in 1 .. %d, cols >= 1", rows, cols, TT * 65535);
    if (int rc = enter(ctx, true)) return rc;
    return transpose_run(ctx, d_in, rows, cols, d_out);
}

// xb_top_train_begin, and with `full` xb_full_train_begin: the checks, the four flat buffers, the masters
static int train_begin(xb_ctx *ctx, const char *who, int layers, bool full, const float *params)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, 1)) return rc;
    if (!params) return fail(ctx, XB_ERR_INVALID, "%s: null host pointer", who);
    if (ctx->top.open) return fail(ctx, XB_ERR_STATE, "%s: a trainer is already open on this context", who);
    if (ctx->head.open) return fail(ctx, XB_ERR_STATE, "%s: a head trainer is open on this context; call xb_head_train_end first", who);
    const int F = ctx->cfg.features;
    const xb::TopPlan pl = xb::top_plan(layers, F, ctx->O);
    if (pl.error) return fail(ctx, XB_ERR_INVALID, "%s: %d unfrozen LSTM layers, accepted: 1 .. %d (the convolutions stay frozen)", who, layers, xb::TOP_MAX_LAYERS);
    if (F % 16 || F > 1024) return fail(ctx, XB_ERR_INVALID, "%s: the training recurrence takes features that are a multiple of 16 up to 1024, got %d", who, F);
    size_t conv = 0;
    if (full) {
        // the inference bottom never runs: no rule about its precision; the head's tanh needs its scale, as everywhere
        if (!(ctx->cfg.scale > 0.0f) || !std::isfinite(ctx->cfg.scale))
            return fail(ctx, XB_ERR_INVALID, "%s: the head needs its tanh with a positive scale, the context has scale %g", who, (double)ctx->cfg.scale);
        const xb::ConvPlan cp = conv_plan_of(ctx);
        if (cp.error || cp.T != ctx->T)
            return fail(ctx, XB_ERR_INVALID, "%s: a window of %d at stride %d on chunks of %d samples cannot be laid out (16 * window <= %d)", who,
                        ctx->cfg.winlen, ctx->cfg.stride, ctx->cfg.chunk_len, xb::CONV_MAX_CK);
        if (cp.params % 4)          // cannot happen while F % 16 == 0; the LSTM section's kernels read 16 bytes at a time
            return fail(ctx, XB_ERR_INVALID, "%s: the conv section of %zu floats leaves the LSTM section off a 16-byte boundary", who, cp.params);
        conv = cp.params;
    } else {
        if (int rc = head_usable(ctx, who)) return rc;
        if (int rc = bottom_usable(ctx, who)) return rc;
    }
    if (int rc = enter(ctx, false)) return rc;
    const size_t max_rows = (size_t)ctx->T * ctx->cfg.max_batch, stride = flat_stride(conv, pl);
    ctx->top.full = full;
    if (grow(ctx, &ctx->top.train, 4 * stride * sizeof(float)) || grow(ctx, &ctx->top.small, (64 + pl.small_floats()) * sizeof(float))) {
        const int rc = top_nomem(ctx, who, pl, max_rows);
        ctx->top.close();
        return rc;
    }
    ctx->top.L = layers;
    const TopBuf b(ctx, pl);
    XB_HIP(ctx, hipMemsetAsync(b.p, 0, 4 * stride * sizeof(float), ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(b.p, params, b.params * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = xb_synchronize(ctx)) { ctx->top.close(); return rc; }
    ctx->top.step = 0;
    ctx->top.rows = 0;
    ctx->top.open = true;
    return XB_OK;
}

XB_API int xb_top_train_begin(xb_ctx *ctx, int layers, const float *params)
{
    return train_begin(ctx, "xb_top_train_begin", layers, false, params);
}

XB_API int xb_full_train_begin(xb_ctx *ctx, const float *params)
{
    return train_begin(ctx, "xb_full_train_begin", xb::TOP_MAX_LAYERS, true, params);
}

XB_API int xb_top_train_grad(xb_ctx *ctx, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, float *loss,
                             float *grad_norm)
{
    return top_call(ctx, "xb_top_train_grad", signal, n, targets, Lt, lengths, false, 0.0f, loss, grad_norm);
}

XB_API int xb_top_train_step(xb_ctx *ctx, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, float lr,
                             float *loss, float *grad_norm)
{
    return top_call(ctx, "xb_top_train_step", signal, n, targets, Lt, lengths, true, lr, loss, grad_norm);
}

XB_API int xb_top_get_weights(xb_ctx *ctx, float *params)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->top.open) return fail(ctx, XB_ERR_STATE, "xb_top_get_weights: no trainer is open");
    if (!params) return fail(ctx, XB_ERR_INVALID, "xb_top_get_weights: null host pointer");
    if (int rc = enter(ctx, false)) return rc;
    const TopBuf b(ctx, plan_of(ctx));
    XB_HIP(ctx, hipMemcpyAsync(params, b.p, b.params * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

XB_API int xb_top_train_end(xb_ctx *ctx)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->top.open) return fail(ctx, XB_ERR_STATE, "xb_top_train_end: no trainer is open");
    if (int rc = enter(ctx, false)) return rc;
    if (int rc = xb_synchronize(ctx)) return rc;
    ctx->top.close();
    return XB_OK;
}

// the trainer's device state, for the tests that compose a step from its parts: the four flat buffers (xb::top_plan's layout,
// `params` floats each), the bottom's output, the scores and their gradient of the last step (null before the first, `rows`
// its T * n), and the step count.  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_top_state(xb_ctx *ctx, float **p, float **g, float **m, float **v, float **x0,
                                                                            float **scores, float **dscores, int64_t *rows, int64_t *step)
{
    if (!ctx || !ctx->top.open) return XB_ERR_STATE;
    const xb::TopPlan pl = plan_of(ctx);
    const TopBuf b(ctx, pl);
    const size_t r = ctx->top.rows;
    if (p) *p = b.p;
    if (g) *g = b.g;
    if (m) *m = b.m;
    if (v) *v = b.v;
    if (x0) *x0 = r ? b.act + pl.x0(r) : nullptr;
    if (scores) *scores = r ? b.act + pl.scores(r) : nullptr;
    if (dscores) *dscores = r ? b.act + pl.dscores(r) : nullptr;
    if (rows) *rows = (int64_t)r;
    if (step) *step = ctx->top.step;
    return XB_OK;
}

// xb_encode_bottom_dev in its two halves, for the timing tool: what = 1 the bottom pass alone (the planes stay in the context),
// what = 2 the join alone, of the planes the last pass of `layers` layers left.  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_bottom_part(xb_ctx *ctx, const float *d_signal, int n, int layers, float *d_x0,
                                                                              int what)
{
    if (!ctx || !d_signal || !d_x0 || layers < 0 || layers > 5 || (what != 1 && what != 2)) return XB_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(d_x0) & 15) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, n)) return rc;
    if (int rc = bottom_usable(ctx, "xb_internal_bottom_part")) return rc;
    if (int rc = enter(ctx, true)) return rc;
    if (what == 1) return encoder_bottom_run(ctx, d_signal, n, layers);
    return join_run(ctx, ctx->x_hi[layers & 1], ctx->x_lo[layers & 1], (size_t)ctx->T * n * ctx->cfg.features, d_x0);
}

// `bytes` bytes of device memory at d_src to the host, behind everything the context has enqueued: how the tests read what
// xb_internal_top_state points to.  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_peek(xb_ctx *ctx, const void *d_src, void *host, size_t bytes)
{
    if (!ctx || !d_src || !host) return XB_ERR_INVALID;
    if (int rc = enter(ctx, false)) return rc;
    if (int rc = xb_synchronize(ctx)) return rc;
    XB_HIP(ctx, hipMemcpy(host, d_src, bytes, hipMemcpyDeviceToHost));
    return XB_OK;
}

}  // extern "C"
