// xb_head.hip -- training the CRF head (the last layer, scores = scale * tanh(X W^T + b)) with everything below it frozen:
// the gradient of its parameters from the gradient of its output (xb_head_grad), the gradient's norm, AdamW, the re-pack of
// the updated weights into the forms the forward GEMM reads, and the trainer that chains them behind the encoder and
// xb_ctc_loss_grad.  The contracts are in the public header.  This translation unit is built without contraction: AdamW and the
// operand arithmetic of xb_head_grad are restated operation by operation in tests/adamw_ref.py and tests/headgrad_ref.py.
#include "xb_ctx.h"
#include "xb_head_split.h"
#include "xb_head_train.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KT = xb::HEAD_KT, TO = xb::HEAD_TO, TF = xb::HEAD_TF;
constexpr int LDK = KT + 8;                 // halfs per LDS row of one output row / feature: 80 bytes, so 16-byte reads stay aligned
constexpr int NORM_BLOCKS = 256;            // partial sums of the norm: fixed, whatever the device, so the order of the sum is too

// The power of two dZ is multiplied by before it is split into fp16 parts: |dZ| <= max|dY| * scale < 2^ex, so the scaled
// values stay below 2^14 (fp16 reaches 65504) and the largest sit 24 binades above fp16's smallest subnormal.  0 for a gradient
// of zeros or one that holds a NaN or an infinity.
__device__ __forceinline__ int head_exponent(unsigned amax_bits, float scale)
{
    const float a = __uint_as_float(amax_bits) * scale;
    if (!(a > 0.0f) || !(a < INFINITY)) return 0;
    int ex;
    (void)frexpf(a, &ex);
    return 14 - ex;
}

__global__ __launch_bounds__(256) void head_absmax_kernel(const float *dy, size_t count, unsigned *out)
{
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const unsigned v = __float_as_uint(dy[i]) & 0x7fffffffu;
        m = v > m ? v : m;
    }
    for (int o = 32; o; o >>= 1) {
        const unsigned v = (unsigned)__shfl_xor((int)m, o);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);        // an integer maximum: the same word in any order
}

struct HeadGradArgs {
    const float *y, *dy;           // (M, O)
    const half_t *x_hi, *x_lo;     // (M, F)
    long M;
    int O, F;
    float scale;
    const unsigned *amax;          // bits of max |dY|
    int o_tile0, o_tiles_launch;   // this launch: blocks of TO output rows [o_tile0, o_tile0 + gridDim.y), workspace rows o_tiles_launch * TO
    int nslabs;
    long ksteps;
    float *part_w;                 // [nslabs][o_tiles_launch * TO][F]
    double *part_b;                // [nslabs][o_tiles_launch * TO]
};

// One workgroup: a TO x TF tile of dW over the k-tiles of one slab.  Per k-tile of KT rows the four waves form dZ from Y and
// dY (fp32, scaled by 2^e, split into fp16 hi + lo) and copy X's two fp16 planes, both transposed into LDS so that a lane's
// eight k values are one 16-byte read; each wave then runs lo*hi, hi*lo, hi*hi on v_mfma_f32_16x16x32_f16 for its 32 x 64
// quarter.  db is the sum of the scaled fp32 dZ in float64, by the workgroups of the first feature tile.
__global__ __launch_bounds__(256) void head_grad_kernel(HeadGradArgs a)
{
    __shared__ __attribute__((aligned(16))) half_t sAh[TO * LDK];
    __shared__ __attribute__((aligned(16))) half_t sAl[TO * LDK];
    __shared__ __attribute__((aligned(16))) half_t sBh[TF * LDK];
    __shared__ __attribute__((aligned(16))) half_t sBl[TF * LDK];
    __shared__ double sDb[4 * TO];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ft = blockIdx.x, otl = blockIdx.y, slab = blockIdx.z;
    const int o0 = (a.o_tile0 + otl) * TO, f0 = ft * TF;
    const long s0 = a.ksteps * (long)slab / a.nslabs, s1 = a.ksteps * (long)(slab + 1) / a.nslabs;
    const int e = head_exponent(*a.amax, a.scale);
    const int wo = (wave & 1) * 32, wf = (wave >> 1) * 64, r = lane & 15, g = lane >> 4;
    const int ao = tid & 63, am = tid >> 6;        // staging of dZ: output row ao of the tile, k = am + 4 i
    const bool o_ok = o0 + ao < a.O;
    f32x4 acc[2][4];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    double db = 0.0;

    for (long st = s0; st < s1; ++st) {
        const long m0 = st * KT;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ml = am + 4 * i;
            const long m = m0 + ml;
            float dz = 0.0f;
            if (o_ok && m < a.M) {
                const size_t at = (size_t)m * a.O + (size_t)(o0 + ao);
                const float yv = a.y[at];
                // d (scale tanh z) / dz from its own output, scale - y^2 / scale, in the form that does not cancel where tanh saturates
                const float gv = ((a.scale - yv) * (a.scale + yv)) / a.scale;
                dz = ldexpf(a.dy[at], e) * gv;
            }
            const half_t h = (half_t)dz;
            sAh[ao * LDK + ml] = h;
            sAl[ao * LDK + ml] = (half_t)(dz - (float)h);
            db += (double)dz;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, f8 = idx & 15, ml = idx >> 4;
            const long m = m0 + ml;
            const int f = f0 + f8 * 8;
            half8 vh = {0, 0, 0, 0, 0, 0, 0, 0}, vl = {0, 0, 0, 0, 0, 0, 0, 0};
            if (m < a.M && f < a.F) {
                vh = *reinterpret_cast<const half8 *>(a.x_hi + (size_t)m * a.F + f);
                vl = *reinterpret_cast<const half8 *>(a.x_lo + (size_t)m * a.F + f);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sBh[(f8 * 8 + j) * LDK + ml] = vh[j];
                sBl[(f8 * 8 + j) * LDK + ml] = vl[j];
            }
        }
        __syncthreads();
        half8 ah[2], al[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = *reinterpret_cast<const half8 *>(&sAh[(wo + 16 * i + r) * LDK + 8 * g]);
            al[i] = *reinterpret_cast<const half8 *>(&sAl[(wo + 16 * i + r) * LDK + 8 * g]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const half8 bh = *reinterpret_cast<const half8 *>(&sBh[(wf + 16 * j + r) * LDK + 8 * g]);
            const half8 bl = *reinterpret_cast<const half8 *>(&sBl[(wf + 16 * j + r) * LDK + 8 * g]);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // the tile's partial sums: accumulator register q of lane (r, g) is output row 4 g + q, feature r of its 16 x 16 block
    const size_t rows_l = (size_t)a.o_tiles_launch * TO;
    float *pw = a.part_w + (size_t)slab * rows_l * a.F;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 4; ++j) {
            const int f = f0 + wf + 16 * j + r;
            if (f >= a.F) continue;
            for (int q = 0; q < 4; ++q) {
                const size_t row = (size_t)otl * TO + wo + 16 * i + 4 * g + q;
                pw[row * a.F + f] = acc[i][j][q];
            }
        }
    if (ft == 0) {
        sDb[am * TO + ao] = db;
        __syncthreads();
        if (tid < TO)
            a.part_b[(size_t)slab * rows_l + (size_t)otl * TO + tid] = ((sDb[tid] + sDb[TO + tid]) + sDb[2 * TO + tid]) + sDb[3 * TO + tid];
    }
}

// dW, db of output rows [o_begin, o_begin + rows): the slabs' partial sums in ascending slab order, then the scale undone
__global__ __launch_bounds__(256) void head_reduce_kernel(const float *part_w, const double *part_b, int nslabs, size_t rows_l, int o_begin,
                                                          int rows, int F, const unsigned *amax, float scale, float *dw, float *dbias)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)rows * F;
    const int e = head_exponent(*amax, scale);
    if (idx < cells) {
        float s = part_w[idx];
        for (int sl = 1; sl < nslabs; ++sl) s += part_w[(size_t)sl * rows_l * F + idx];
        dw[(size_t)o_begin * F + idx] = ldexpf(s, -e);
    } else if (idx < cells + (size_t)rows) {
        const size_t row = idx - cells;
        double s = part_b[row];
        for (int sl = 1; sl < nslabs; ++sl) s += part_b[(size_t)sl * rows_l + row];
        dbias[(size_t)o_begin + row] = (float)ldexp(s, -e);
    }
}

// sqrt(sum a^2 + sum b^2) in float64: NORM_BLOCKS partial sums over interleaved elements, each a tree over the workgroup's 256
// threads, then one tree over the partial sums -- the same order on every run and every device
__device__ __forceinline__ double block_tree_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void head_norm_partial_kernel(const float *a, size_t na, const float *b, size_t nb, double *part)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (size_t)NORM_BLOCKS * 256) {
        const double v = (double)(i < na ? a[i] : b[i - na]);
        s += v * v;
    }
    const double t = block_tree_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void head_norm_final_kernel(const double *part, float *out)
{
    __shared__ double sh[256];
    const double t = block_tree_sum(threadIdx.x < NORM_BLOCKS ? part[threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) *out = (float)sqrt(t);
}

// torch.optim.AdamW's single-tensor update, every operation rounded to nearest on its own (tests/adamw_ref.py is this text in numpy)
__global__ __launch_bounds__(256) void adamw_kernel(float *p, float *g, float *m, float *v, size_t len, float clip, float decay,
                                                    float step_size, float bc2_sqrt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const float b1 = 0.9f, b2 = 0.999f, c1 = (float)(1.0 - 0.9), c2 = (float)(1.0 - 0.999), eps = 1e-8f;
    // plain operators: this translation unit is built without contraction and with correctly rounded division and square root
    // (the __f*_rn intrinsics would do for the products and sums, but __fsqrt_rn is the approximate native square root here)
    const float gi = g[i] * clip;
    float pi = p[i] * decay;
    const float mi = b1 * m[i] + c1 * gi;
    const float vi = b2 * v[i] + (c2 * gi) * gi;
    const float den = sqrtf(vi) / bc2_sqrt + eps;
    pi = pi - (step_size * mi) / den;
    g[i] = gi; p[i] = pi; m[i] = mi; v[i] = vi;
}

// the head's weights (O, F) fp32 -> split fp16 rows (hi, lo) and the fragment-major image of the three-product GEMM, as
// xb::split_rows and xb::fragment_major (nsplit 3) build them: one thread per 16 bytes of each part, rows up to rows4 are zeros
__global__ __launch_bounds__(256) void head_repack_kernel(const float *w, int O, int F, half_t *hi, half_t *lo, unsigned char *f4, size_t kstride)
{
    const int nt32 = ((O + 255) & ~255) / 32, nk = F / 32;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nk * nt32 * 128) return;
    const int l = (int)(idx & 63), c = (int)((idx >> 6) & 1), nt = (int)((idx >> 7) % nt32), kt = (int)((idx >> 7) / nt32);
    const int row = nt * 32 + c * 16 + (l & 15), col = kt * 32 + (l >> 4) * 8;
    half8 h = {0, 0, 0, 0, 0, 0, 0, 0}, q = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < O) {
        const size_t at = (size_t)row * F + col;
        for (int j = 0; j < 8; ++j) {
            const float v = w[at + j];
            h[j] = (half_t)v;
            q[j] = (half_t)(v - (float)h[j]);
        }
        *reinterpret_cast<half8 *>(hi + at) = h;
        *reinterpret_cast<half8 *>(lo + at) = q;
    }
    unsigned char *blk = f4 + (size_t)kt * kstride + (size_t)nt * 4 * 1024 + (size_t)l * 16;
    *reinterpret_cast<half8 *>(blk + c * 1024) = h;
    *reinterpret_cast<half8 *>(blk + (2 + c) * 1024) = q;
}

// layout of xb_ctx::head.small: the max |dY| word, the norm, the norm's partial sums
unsigned *small_amax(xb_ctx *ctx) { return static_cast<unsigned *>(ctx->head.small.p); }
float *small_norm(xb_ctx *ctx) { return reinterpret_cast<float *>(static_cast<char *>(ctx->head.small.p) + 64); }
double *small_part(xb_ctx *ctx) { return reinterpret_cast<double *>(static_cast<char *>(ctx->head.small.p) + 256); }
int small_ready(xb_ctx *ctx) { return grow(ctx, &ctx->head.small, 256 + sizeof(double) * NORM_BLOCKS); }

}  // namespace

int head_usable(xb_ctx *ctx, const char *who)
{
    if (ctx->ns_lin != 3)
        return fail(ctx, XB_ERR_INVALID, "%s: the head of this context is not computed in three fp16 products; create it with precision "
                    "mixed or f16x3", who);
    if (!(ctx->cfg.scale > 0.0f) || !std::isfinite(ctx->cfg.scale))
        return fail(ctx, XB_ERR_INVALID, "%s: the head needs its tanh with a positive scale, the context has scale %g", who, (double)ctx->cfg.scale);
    return XB_OK;
}

namespace {

// X of a call: the caller's planes, or (both null) the last LSTM layer's output of the most recent encoder pass, whose rows the
// call must then cover
int head_operand(xb_ctx *ctx, const char *who, const void *x_hi, const void *x_lo, int64_t rows)
{
    if (rows < 1 || rows > ((int64_t)1 << 40)) return fail(ctx, XB_ERR_INVALID, "%s: %lld rows", who, (long long)rows);
    if ((x_hi == nullptr) != (x_lo == nullptr)) return fail(ctx, XB_ERR_INVALID, "%s: x_hi and x_lo are both given or both null", who);
    if (!x_hi && (ctx->enc_n < 1 || rows != (int64_t)ctx->T * ctx->enc_n))
        return fail(ctx, XB_ERR_STATE, "%s: without X the rows must be those of the last encoder pass (%d x %d), got %lld", who, ctx->T,
                    ctx->enc_n, (long long)rows);
    return XB_OK;
}

int head_grad_run(xb_ctx *ctx, const char *who, const float *d_y, const float *d_dy, const half_t *d_xh, const half_t *d_xl, int64_t M,
                  float *d_dw, float *d_db)
{
    const int O = ctx->O, F = ctx->cfg.features;
    if (!d_xh) { d_xh = ctx->x_hi[1]; d_xl = ctx->x_lo[1]; }
    if (((uintptr_t)d_xh | (uintptr_t)d_xl) & 15) return fail(ctx, XB_ERR_INVALID, "%s: x_hi and x_lo must be 16-byte aligned", who);
    const xb::HeadPlan plan = xb::head_plan((long)M, O, F, ctx->cu_count, xb::head_scratch_bound(getenv("XB_HEAD_SCRATCH_MB")));
    if (plan.error) return fail(ctx, XB_ERR_INVALID, "%s: one slab of %d output rows (%zu bytes) exceeds XB_HEAD_SCRATCH_MB", who, TO, plan.row_bytes);
    if (int rc = grow(ctx, &ctx->head.part, plan.bytes)) return rc;
    if (int rc = small_ready(ctx)) return rc;
    unsigned *amax = small_amax(ctx);
    const size_t cells = (size_t)M * O;
    XB_HIP(ctx, hipMemsetAsync(amax, 0, sizeof(unsigned), ctx->stream));
    head_absmax_kernel<<<(unsigned)std::min<size_t>(1024, (cells + 255) / 256), 256, 0, ctx->stream>>>(d_dy, cells, amax);
    if (int rc = launched(ctx, who)) return rc;
    HeadGradArgs a{};
    a.y = d_y; a.dy = d_dy; a.x_hi = d_xh; a.x_lo = d_xl; a.M = (long)M; a.O = O; a.F = F; a.scale = ctx->cfg.scale; a.amax = amax;
    a.o_tiles_launch = plan.o_tiles_per_launch; a.nslabs = plan.nslabs; a.ksteps = plan.ksteps;
    const size_t rows_l = (size_t)plan.o_tiles_per_launch * TO;
    a.part_w = static_cast<float *>(ctx->head.part.p);
    a.part_b = reinterpret_cast<double *>(a.part_w + (size_t)plan.nslabs * rows_l * F);
    for (int t0 = 0; t0 < plan.o_tiles; t0 += plan.o_tiles_per_launch) {
        const int tiles = std::min(plan.o_tiles_per_launch, plan.o_tiles - t0);
        a.o_tile0 = t0;
        head_grad_kernel<<<dim3(plan.f_tiles, tiles, plan.nslabs), 256, 0, ctx->stream>>>(a);
        if (int rc = launched(ctx, who)) return rc;
        const int o_begin = t0 * TO, rows = std::min(tiles * TO, O - o_begin);
        const size_t work = (size_t)rows * F + rows;
        head_reduce_kernel<<<(unsigned)((work + 255) / 256), 256, 0, ctx->stream>>>(a.part_w, a.part_b, plan.nslabs, rows_l, o_begin, rows, F, amax,
                                                                                  a.scale, d_dw, d_db);
        if (int rc = launched(ctx, who)) return rc;
    }
    return XB_OK;
}

}  // namespace

int grad_norm_run(xb_ctx *ctx, const float *d_a, size_t na, const float *d_b, size_t nb, float *d_norm)
{
    if (int rc = small_ready(ctx)) return rc;
    head_norm_partial_kernel<<<NORM_BLOCKS, 256, 0, ctx->stream>>>(d_a, na, d_b, nb, small_part(ctx));
    if (int rc = launched(ctx, "xb_grad_norm")) return rc;
    head_norm_final_kernel<<<1, 256, 0, ctx->stream>>>(small_part(ctx), d_norm);
    if (int rc = launched(ctx, "xb_grad_norm")) return rc;
    return XB_OK;
}

int adamw_run(xb_ctx *ctx, float *p, float *g, float *m, float *v, size_t len, float clip, float decay, float step_size, float bc2_sqrt)
{
    adamw_kernel<<<(unsigned)((len + 255) / 256), 256, 0, ctx->stream>>>(p, g, m, v, len, clip, decay, step_size, bc2_sqrt);
    return launched(ctx, "xb_adamw_step");
}

namespace {

int repack_run(xb_ctx *ctx, const float *d_w, const float *d_b)
{
    const int O = ctx->O, F = ctx->cfg.features;
    const size_t threads = (size_t)(F / 32) * (((O + 255) & ~255) / 32) * 128;
    head_repack_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, ctx->stream>>>(d_w, O, F, ctx->wl_hi, ctx->wl_lo, ctx->wl_f4, ctx->wl_ks);
    if (int rc = launched(ctx, "xb_head_repack")) return rc;
    XB_HIP(ctx, hipMemcpyAsync(ctx->bl, d_b, sizeof(float) * (size_t)O, hipMemcpyDeviceToDevice, ctx->stream));
    return XB_OK;
}

// the floats of the trainer's buffer: parameters, first and second moments, gradient, each (W | b)
struct TrainBuf {
    size_t len;
    float *p, *m, *v, *g;
    explicit TrainBuf(xb_ctx *ctx) : len((size_t)ctx->O * ctx->cfg.features + ctx->O)
    {
        p = static_cast<float *>(ctx->head.train.p);
        m = p + len; v = m + len; g = v + len;
    }
};

}  // namespace

// AdamW's scalars of step `step` at learning rate lr, computed in double and rounded once (torch's defaults: betas 0.9 / 0.999,
// weight decay 0.01)
void adamw_scalars(double lr, long step, float *decay, float *step_size, float *bc2_sqrt)
{
    *decay = (float)(1.0 - lr * 0.01);
    *step_size = (float)(lr / (1.0 - std::pow(0.9, (double)step)));
    *bc2_sqrt = (float)std::sqrt(1.0 - std::pow(0.999, (double)step));
}

// ---- the tail every trainer's step shares (xb_head_train.h) ----

int train_call_enter(xb_ctx *ctx, const char *who, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths,
                     bool step, float lr, const float *loss, const float *grad_norm)
{
    if (int rc = check_ready(ctx, n)) return rc;
    if (!signal || !targets || !lengths || !loss || !grad_norm) return fail(ctx, XB_ERR_INVALID, "%s: null argument", who);
    if (step && (!(lr >= 0.0f) || !std::isfinite(lr))) return fail(ctx, XB_ERR_INVALID, "%s: learning rate %g", who, (double)lr);
    if (int rc = label_batch_check(ctx, who, targets, n, Lt, lengths)) return rc;
    return enter(ctx, false);
}

int train_read_back(xb_ctx *ctx, const float *d_norm, const float *d_loss, int n, float *norm, float *mean_loss)
{
    std::vector<float> losses((size_t)n);
    XB_HIP(ctx, hipMemcpyAsync(norm, d_norm, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(losses.data(), d_loss, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = xb_synchronize(ctx)) return rc;
    double sum = 0.0;
    for (float l : losses) sum += (double)l;
    *mean_loss = (float)(sum / (double)n);
    return XB_OK;
}

int train_update(xb_ctx *ctx, const char *who, float norm, float lr, long step, float *p, float *g, float *m, float *v, size_t len)
{
    if (!std::isfinite(norm)) return fail(ctx, XB_ERR_DEVICE, "%s: the gradient's norm is not finite; the weights are unchanged", who);
    // clip_grad_norm_(max_norm = 2.0): the factor in double from the fp32 norm, rounded once
    const float clip = (float)std::min(1.0, 2.0 / ((double)norm + 1e-6));
    float decay, step_size, bc2_sqrt;
    adamw_scalars((double)lr, step, &decay, &step_size, &bc2_sqrt);
    return adamw_run(ctx, p, g, m, v, len, clip, decay, step_size, bc2_sqrt);
}

extern "C" {

XB_API int xb_head_grad_dev(xb_ctx *ctx, const float *d_y, const float *d_dy, const uint16_t *d_x_hi, const uint16_t *d_x_lo, int64_t rows,
                            float *d_dw, float *d_db)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, 1)) return rc;
    if (!d_y || !d_dy || !d_dw || !d_db) return fail(ctx, XB_ERR_INVALID, "xb_head_grad: null device pointer");
    if (int rc = head_usable(ctx, "xb_head_grad")) return rc;
    if (int rc = head_operand(ctx, "xb_head_grad", d_x_hi, d_x_lo, rows)) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return head_grad_run(ctx, "xb_head_grad", d_y, d_dy, reinterpret_cast<const half_t *>(d_x_hi), reinterpret_cast<const half_t *>(d_x_lo), rows,
                         d_dw, d_db);
}

XB_API int xb_head_grad(xb_ctx *ctx, const float *y, const float *dy, const uint16_t *x_hi, const uint16_t *x_lo, int64_t rows, float *dw,
                        float *db)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, 1)) return rc;
    if (!y || !dy || !dw || !db) return fail(ctx, XB_ERR_INVALID, "xb_head_grad: null host pointer");
    if (int rc = head_usable(ctx, "xb_head_grad")) return rc;
    if (int rc = head_operand(ctx, "xb_head_grad", x_hi, x_lo, rows)) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t O = (size_t)ctx->O, F = (size_t)ctx->cfg.features, M = (size_t)rows;
    Staging st{ctx};
    const auto d_y = st.take<float>(M * O), d_dy = st.take<float>(M * O);
    const auto s_xh = st.take<half_t>(x_hi ? M * F : 0), s_xl = st.take<half_t>(x_hi ? M * F : 0);      // without X: two empty pieces
    const auto d_dw = st.take<float>(O * F), d_db = st.take<float>(O);
    if (int rc = st.ready()) return rc;
    half_t *d_xh = x_hi ? (half_t *)s_xh : nullptr, *d_xl = x_hi ? (half_t *)s_xl : nullptr;
    XB_HIP(ctx, hipMemcpyAsync(d_y, y, M * O * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_dy, dy, M * O * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (x_hi) {
        XB_HIP(ctx, hipMemcpyAsync(d_xh, x_hi, M * F * 2, hipMemcpyHostToDevice, ctx->stream));
        XB_HIP(ctx, hipMemcpyAsync(d_xl, x_lo, M * F * 2, hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = head_grad_run(ctx, "xb_head_grad", d_y, d_dy, d_xh, d_xl, rows, d_dw, d_db)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(dw, d_dw, O * F * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(db, d_db, O * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

XB_API int xb_grad_norm_dev(xb_ctx *ctx, const float *d_dw, int64_t len_w, const float *d_db, int64_t len_b, float *d_norm)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_norm || len_w < 0 || len_b < 0 || (len_w && !d_dw) || (len_b && !d_db)) return fail(ctx, XB_ERR_INVALID, "xb_grad_norm: bad argument");
    if (int rc = enter(ctx, true)) return rc;
    return grad_norm_run(ctx, d_dw, (size_t)len_w, d_db, (size_t)len_b, d_norm);
}

XB_API int xb_adamw_step_dev(xb_ctx *ctx, float *d_p, float *d_g, float *d_m, float *d_v, int64_t len, float clip, float decay,
                             float step_size, float bc2_sqrt)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_p || !d_g || !d_m || !d_v || len < 1) return fail(ctx, XB_ERR_INVALID, "xb_adamw_step: bad argument");
    if (int rc = enter(ctx, true)) return rc;
    return adamw_run(ctx, d_p, d_g, d_m, d_v, (size_t)len, clip, decay, step_size, bc2_sqrt);
}

XB_API int xb_head_repack_dev(xb_ctx *ctx, const float *d_w, const float *d_b)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, 1)) return rc;
    if (!d_w || !d_b) return fail(ctx, XB_ERR_INVALID, "xb_head_repack: null device pointer");
    if (int rc = head_usable(ctx, "xb_head_repack")) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return repack_run(ctx, d_w, d_b);
}

// the head's three images and bias as the forward reads them, for the tests.  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_head_image(xb_ctx *ctx, uint16_t *hi, uint16_t *lo, unsigned char *f4,
                                                                             size_t f4_bytes, float *bias)
{
    if (!ctx || !hi || !lo || !f4 || !bias) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, 1)) return rc;
    const size_t O = (size_t)ctx->O, F = (size_t)ctx->cfg.features, image = (F / 32) * ctx->wl_ks;
    if (f4_bytes != image) return fail(ctx, XB_ERR_INVALID, "xb_internal_head_image: the image has %zu bytes, got room for %zu", image, f4_bytes);
    if (int rc = xb_synchronize(ctx)) return rc;
    XB_HIP(ctx, hipMemcpy(hi, ctx->wl_hi, O * F * 2, hipMemcpyDeviceToHost));
    XB_HIP(ctx, hipMemcpy(lo, ctx->wl_lo, O * F * 2, hipMemcpyDeviceToHost));
    XB_HIP(ctx, hipMemcpy(f4, ctx->wl_f4, image, hipMemcpyDeviceToHost));
    XB_HIP(ctx, hipMemcpy(bias, ctx->bl, O * sizeof(float), hipMemcpyDeviceToHost));
    return XB_OK;
}

// xb::head_plan for the CPU tests: out = {error, ksteps, nslabs, o_tiles, f_tiles, o_tiles_per_launch, launches, row_bytes, bytes,
// order_kept}; bound_mb as the text of XB_HEAD_SCRATCH_MB (null: the default).  Touches no device.  Not part of the public header.
extern "C" __attribute__((visibility("default"))) void xb_internal_head_plan(int64_t M, int O, int F, int cu_count, const char *bound_mb,
                                                                             int64_t out[10])
{
    const xb::HeadPlan p = xb::head_plan((long)M, O, F, cu_count, xb::head_scratch_bound(bound_mb));
    const int64_t v[10] = {p.error, p.ksteps, p.nslabs, p.o_tiles, p.f_tiles, p.o_tiles_per_launch, p.launches, (int64_t)p.row_bytes,
                           (int64_t)p.bytes, p.order_kept};
    memcpy(out, v, sizeof v);
}

XB_API int xb_head_train_begin(xb_ctx *ctx, const float *w, const float *b)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = check_ready(ctx, 1)) return rc;
    if (!w || !b) return fail(ctx, XB_ERR_INVALID, "xb_head_train_begin: null host pointer");
    if (ctx->head.open) return fail(ctx, XB_ERR_STATE, "xb_head_train_begin: a trainer is already open on this context");
    if (ctx->top.open) return fail(ctx, XB_ERR_STATE, "xb_head_train_begin: a top-layer trainer is open on this context; call xb_top_train_end first");
    if (int rc = head_usable(ctx, "xb_head_train_begin")) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t OF = (size_t)ctx->O * ctx->cfg.features, O = (size_t)ctx->O;
    if (int rc = grow(ctx, &ctx->head.train, 4 * (OF + O) * sizeof(float))) return rc;
    const TrainBuf t(ctx);
    XB_HIP(ctx, hipMemsetAsync(t.p, 0, 4 * t.len * sizeof(float), ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(t.p, w, OF * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(t.p + OF, b, O * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    // the forward reads what the master weights say from the first step on
    if (int rc = repack_run(ctx, t.p, t.p + OF)) return rc;
    if (int rc = xb_synchronize(ctx)) return rc;
    ctx->head.step = 0;
    ctx->head.open = true;
    return XB_OK;
}

XB_API int xb_head_train_step(xb_ctx *ctx, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, float lr,
                              float *loss, float *grad_norm)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->head.open) return fail(ctx, XB_ERR_STATE, "xb_head_train_step: no trainer is open; call xb_head_train_begin first");
    if (int rc = train_call_enter(ctx, "xb_head_train_step", signal, n, targets, Lt, lengths, true, lr, loss, grad_norm)) return rc;
    const size_t N = (size_t)n, O = (size_t)ctx->O, OF = O * ctx->cfg.features, T = (size_t)ctx->T;
    if (int rc = grow(ctx, &ctx->head.grad, T * N * O * sizeof(float))) return rc;
    Staging st{ctx};
    const LabelBatch lb(st, n, Lt);
    if (int rc = st.ready()) return rc;
    if (int rc = small_ready(ctx)) return rc;
    float *d_grad = static_cast<float *>(ctx->head.grad.p);
    const TrainBuf t(ctx);
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * N * ctx->cfg.chunk_len, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = lb.upload(ctx, targets, lengths)) return rc;
    if (int rc = encoder_run(ctx, ctx->d_signal, n, ctx->scores, ctx->O)) return rc;
    if (int rc = ctc_grad_run(ctx, "xb_head_train_step", ctx->scores, ctx->T, n, 0, ctx->O, lb.targets, Lt, lb.len, 0.0f, 1, lb.loss, d_grad)) return rc;
    if (int rc = head_grad_run(ctx, "xb_head_train_step", ctx->scores, d_grad, nullptr, nullptr, (int64_t)(T * N), t.g, t.g + OF)) return rc;
    if (int rc = grad_norm_run(ctx, t.g, OF, t.g + OF, O, small_norm(ctx))) return rc;
    float norm = 0.0f, mean = 0.0f;
    if (int rc = train_read_back(ctx, small_norm(ctx), lb.loss, n, &norm, &mean)) return rc;
    // (W | b) are contiguous in each of p, g, m, v and the update is elementwise: one launch over both
    if (int rc = train_update(ctx, "xb_head_train_step", norm, lr, ctx->head.step + 1, t.p, t.g, t.m, t.v, t.len)) return rc;
    if (int rc = repack_run(ctx, t.p, t.p + OF)) return rc;
    ++ctx->head.step;
    *loss = mean;
    *grad_norm = norm;
    return xb_synchronize(ctx);
}

XB_API int xb_head_get_weights(xb_ctx *ctx, float *w, float *b)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->head.open) return fail(ctx, XB_ERR_STATE, "xb_head_get_weights: no trainer is open");
    if (!w || !b) return fail(ctx, XB_ERR_INVALID, "xb_head_get_weights: null host pointer");
    if (int rc = enter(ctx, false)) return rc;
    const size_t OF = (size_t)ctx->O * ctx->cfg.features;
    const TrainBuf t(ctx);
    XB_HIP(ctx, hipMemcpyAsync(w, t.p, OF * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(b, t.p + OF, (size_t)ctx->O * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// the trainer's device state, for the tests that compose a step from its parts: p, m, v, g, each (W | b).  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_head_state(xb_ctx *ctx, float **p, float **m, float **v, float **g, int64_t *step)
{
    if (!ctx || !ctx->head.open) return XB_ERR_STATE;
    const TrainBuf t(ctx);
    if (p) *p = t.p;
    if (m) *m = t.m;
    if (v) *v = t.v;
    if (g) *g = t.g;
    if (step) *step = ctx->head.step;
    return XB_OK;
}

XB_API int xb_head_train_end(xb_ctx *ctx)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->head.open) return fail(ctx, XB_ERR_STATE, "xb_head_train_end: no trainer is open");
    if (int rc = enter(ctx, false)) return rc;
    if (int rc = xb_synchronize(ctx)) return rc;
    ctx->head.close();
    return XB_OK;
}

}  // extern "C"
