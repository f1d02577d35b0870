// xb_train_gemm.hip -- the products of training that carry no recurrence, in fp32 on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32: exact f32 operands, so a gradient of 1e-9 needs no power-of-two scaling): xb_linear_f32_dev
// (out = act(A W^T + bias), both operands k-contiguous), xb_wgrad_f32_dev (dW = A^T B and the column sums of A, both operands
// row-major over the summed dimension) and xb_head_dz_dev (the head's tanh derivative from its own output).  The contracts are
// in the public header.  No floating-point atomics, no partial
// sums between workgroups: an output element is summed by one wave in an order its shape alone decides.  Built without
// contraction, division correctly rounded (lt_tanh is the LSTM training kernels' function, xb_math.h).
#include "xb_ctx.h"
#include "xb_math.h"
#include "xb_train_gemm.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TM = 64, TN = 64;      // output tile of one workgroup: wave w owns rows 16 w .. 16 w + 15 and all 64 columns
constexpr int KC = 32;               // k of one staging round of xb_linear (two MFMA chunks of 16)
constexpr int LDK = KC + 4;          // floats per LDS row: 144 bytes -- float4 reads stay aligned, and the 16 rows a quarter-wave
                                     // reads start in 16 different groups of four banks (36 r mod 64 covers the multiples of 4)
constexpr int MC = 32;               // rows of one staging round of xb_wgrad
constexpr int LDO = TN + 16;         // floats per LDS row there: the four rows a wave reads at once start 16 banks apart

// ---- out = act(A W^T + bias) -------------------------------------------------------------------------------------------------
struct LinArgs {
    const float *a, *w, *bias;
    float *out;
    long M;
    int N, K, act;
    float scale;
};

// A staging round: rows [r0, r0 + 64) of `src` (rows x K, k-contiguous), k in [k0, k0 + 32), zeros past the edges, into registers
// (8 floats per thread) and from there into LDS.  VEC: K % 4 == 0 and a 16-byte aligned base, one float4 per load.
template <bool VEC>
__device__ __forceinline__ void lin_fetch(const float *src, long rows, int K, long r0, int k0, int tid, f32x4 (&v)[2])
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, rl = idx >> 3, kq = (idx & 7) * 4;
        const long row = r0 + rl;
        const int k = k0 + kq;
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row < rows) {
            const float *p = src + (size_t)row * K + k;
            if (VEC) {
                if (k < K) x = *reinterpret_cast<const f32x4 *>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k + j < K) x[j] = p[j];
            }
        }
        v[i] = x;
    }
}
__device__ __forceinline__ void lin_stash(float *s, int tid, const f32x4 (&v)[2])
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, rl = idx >> 3, kq = (idx & 7) * 4;
        *reinterpret_cast<f32x4 *>(s + rl * LDK + kq) = v[i];
    }
}

// Workgroup (blockIdx.x: 64 columns, blockIdx.y: 64 rows).  Per round of 32 k both tiles go through LDS (the next round's loads
// are issued before this round's MFMAs); lane (r = lane & 15, q = lane >> 4) holds k = k0 + 16 c + 4 q + m in element m of its
// float4, MFMA m of chunk c sums the four q.  An element's order of summation is k's alone: chunks ascending, m ascending.
template <bool VEC>
__global__ __launch_bounds__(256) void linear_f32_kernel(LinArgs a)
{
    __shared__ __attribute__((aligned(16))) float sA[TM * LDK];
    __shared__ __attribute__((aligned(16))) float sW[TN * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const long m0 = (long)blockIdx.y * TM;
    const int n0 = blockIdx.x * TN;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 va[2], vw[2];
    lin_fetch<VEC>(a.a, a.M, a.K, m0, 0, tid, va);
    lin_fetch<VEC>(a.w, a.N, a.K, n0, 0, tid, vw);
    for (int k0 = 0; k0 < a.K; k0 += KC) {
        __syncthreads();                                   // the previous round's reads are done
        lin_stash(sA, tid, va);
        lin_stash(sW, tid, vw);
        __syncthreads();
        if (k0 + KC < a.K) {
            lin_fetch<VEC>(a.a, a.M, a.K, m0, k0 + KC, tid, va);
            lin_fetch<VEC>(a.w, a.N, a.K, n0, k0 + KC, tid, vw);
        }
#pragma unroll
        for (int c = 0; c < KC / 16; ++c) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(&sA[(wave * 16 + r) * LDK + c * 16 + q * 4]);
            f32x4 bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const f32x4 *>(&sW[(j * 16 + r) * LDK + c * 16 + q * 4]);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[j][m], acc[j], 0, 0, 0);
        }
    }
    // accumulator register i of lane (r, q): row 4 q + i, column r of the 16 x 16 block
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + j * 16 + r;
        if (col >= a.N) continue;
        const float b = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = m0 + wave * 16 + q * 4 + i;
            if (row >= a.M) continue;
            float z = acc[j][i];
            if (a.bias) z = z + b;
            if (a.act == 1) z = a.scale * lt_tanh(z);
            a.out[(size_t)row * a.N + col] = z;
        }
    }
}

// ---- dW = A^T B, dcol = column sums of A ---------------------------------------------------------------------------------------
struct WgArgs {
    const float *a, *b;     // (M, N), (M, K)
    float *dw, *dcol;       // (N, K), (N) or null
    long M, block_rows;
    int N, K;
};

// rows [m0, m0 + 32) x columns [c0, c0 + 64) of src (rows x ld), zeros past the edges
template <bool VEC>
__device__ __forceinline__ void wg_fetch(const float *src, long rows, int ld, long m0, int c0, int tid, f32x4 (&v)[2])
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, ml = idx >> 4, cq = (idx & 15) * 4;
        const long m = m0 + ml;
        const int c = c0 + cq;
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
        if (m < rows) {
            const float *p = src + (size_t)m * ld + c;
            if (VEC) {
                if (c < ld) x = *reinterpret_cast<const f32x4 *>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < ld) x[j] = p[j];
            }
        }
        v[i] = x;
    }
}
__device__ __forceinline__ void wg_stash(float *s, int tid, const f32x4 (&v)[2])
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, ml = idx >> 4, cq = (idx & 15) * 4;
        *reinterpret_cast<f32x4 *>(s + ml * LDO + cq) = v[i];
    }
}

// Workgroup (blockIdx.x: 64 columns f of dW, blockIdx.y: 64 rows o of dW) walks all of M in ascending order.  The operands
// arrive m-major; they are laid into LDS as they come (coalesced) and TURNED by the read: the MFMA wants, from lane (r, q),
// a[m = 4 s + q][o = r] and b[m = 4 s + q][f = r] -- one word of LDS row 4 s + q each.  Sum of an element: MFMA s adds rows
// 4 s .. 4 s + 3 to the running sum, s ascending; every block_rows rows the running sum is added to the total and starts again
// from zero (xb_train_gemm.h: WGRAD_BLOCK_ROWS).  dcol: the workgroups of blockIdx.x == 0, float64, thread (o, g) sums rows
// g, g + 4, ... in ascending order, the four g are added in order and rounded once.
template <bool VEC_A, bool VEC_B>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(WgArgs a)
{
    __shared__ __attribute__((aligned(16))) float sA[MC * LDO];
    __shared__ __attribute__((aligned(16))) float sB[MC * LDO];
    __shared__ double sD[4 * TM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int o0 = blockIdx.y * TM, f0 = blockIdx.x * TN;
    const bool want_col = a.dcol && blockIdx.x == 0;
    const int co = tid & 63, cg = tid >> 6;
    f32x4 acc[4], tot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = tot[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    double col = 0.0;
    f32x4 va[2], vb[2];
    if (a.M > 0) {
        wg_fetch<VEC_A>(a.a, a.M, a.N, 0, o0, tid, va);
        wg_fetch<VEC_B>(a.b, a.M, a.K, 0, f0, tid, vb);
    }
    long in_block = 0;
    for (long m0 = 0; m0 < a.M; m0 += MC) {
        __syncthreads();
        wg_stash(sA, tid, va);
        wg_stash(sB, tid, vb);
        __syncthreads();
        if (m0 + MC < a.M) {
            wg_fetch<VEC_A>(a.a, a.M, a.N, m0 + MC, o0, tid, va);
            wg_fetch<VEC_B>(a.b, a.M, a.K, m0 + MC, f0, tid, vb);
        }
#pragma unroll
        for (int s = 0; s < MC / 4; ++s) {
            const float av = sA[(4 * s + q) * LDO + wave * 16 + r];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sB[(4 * s + q) * LDO + j * 16 + r], acc[j], 0, 0, 0);
        }
        if (want_col) {
#pragma unroll
            for (int i = 0; i < MC / 4; ++i) col += (double)sA[(cg + 4 * i) * LDO + co];
        }
        in_block += MC;
        if (in_block >= a.block_rows) {                    // block_rows is a multiple of MC
#pragma unroll
            for (int j = 0; j < 4; ++j) { tot[j] = tot[j] + acc[j]; acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
            in_block = 0;
        }
    }
    // accumulator register i of lane (r, q): row o = 4 q + i, column f = r of the 16 x 16 block; x + 0.0f writes a zero as +0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = f0 + j * 16 + r;
        if (f >= a.K) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = o0 + wave * 16 + q * 4 + i;
            if (o < a.N) a.dw[(size_t)o * a.K + f] = (tot[j][i] + acc[j][i]) + 0.0f;
        }
    }
    if (want_col) {
        sD[cg * TM + co] = col;
        __syncthreads();
        if (tid < TM && o0 + tid < a.N)
            a.dcol[o0 + tid] = (float)(((sD[tid] + sD[TM + tid]) + sD[2 * TM + tid]) + sD[3 * TM + tid]) + 0.0f;
    }
}

// ---- element kernels -----------------------------------------------------------------------------------------------------------
// d (scale tanh z) / dz from its own output, in the form that does not cancel where tanh saturates (xb_head_grad's, without its
// power-of-two factor): one rounding per operation
__global__ __launch_bounds__(256) void head_dz_kernel(const float *y, const float *dy, size_t count, float scale, float *dz)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float yv = y[i];
    const float gv = ((scale - yv) * (scale + yv)) / scale;
    dz[i] = dy[i] * gv;
}

bool vec_ok(const float *p, int ld) { return (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the grid's y dimension holds 65535 blocks: M up to 64 * 65535 rows per launch, more in several
constexpr long ROWS_PER_LAUNCH = (long)TM * 65535;

}  // namespace

namespace xb {

int linear_f32_run(xb_ctx *ctx, const float *a, const float *w, const float *bias, int64_t M, int N, int K, int act, float scale, float *out)
{
    for (long m0 = 0; m0 < (long)M; m0 += ROWS_PER_LAUNCH) {
        LinArgs g{a + (size_t)m0 * K, w, bias, out + (size_t)m0 * N, std::min<long>(ROWS_PER_LAUNCH, (long)M - m0), N, K, act, scale};
        const dim3 grid((unsigned)((N + TN - 1) / TN), (unsigned)((g.M + TM - 1) / TM));
        if (vec_ok(a, K) && vec_ok(w, K)) linear_f32_kernel<true><<<grid, 256, 0, ctx->stream>>>(g);
        else linear_f32_kernel<false><<<grid, 256, 0, ctx->stream>>>(g);
    }
    return launched(ctx, "xb_linear_f32");
}

int wgrad_f32_run(xb_ctx *ctx, const float *a, const float *b, int64_t M, int N, int K, float *dw, float *dcol, long block_rows)
{
    WgArgs g{a, b, dw, dcol, (long)M, block_rows, N, K};
    const dim3 grid((unsigned)((K + TN - 1) / TN), (unsigned)((N + TM - 1) / TM));
    const bool va = vec_ok(a, N), vb = vec_ok(b, K);
    if (va && vb) wgrad_f32_kernel<true, true><<<grid, 256, 0, ctx->stream>>>(g);
    else if (va) wgrad_f32_kernel<true, false><<<grid, 256, 0, ctx->stream>>>(g);
    else if (vb) wgrad_f32_kernel<false, true><<<grid, 256, 0, ctx->stream>>>(g);
    else wgrad_f32_kernel<false, false><<<grid, 256, 0, ctx->stream>>>(g);
    return launched(ctx, "xb_wgrad_f32");
}

int head_dz_run(xb_ctx *ctx, const float *y, const float *dy, int64_t count, float scale, float *dz)
{
    head_dz_kernel<<<(unsigned)(((size_t)count + 255) / 256), 256, 0, ctx->stream>>>(y, dy, (size_t)count, scale, dz);
    return launched(ctx, "xb_head_dz");
}

}  // namespace xb

extern "C" {

XB_API int xb_linear_f32_dev(xb_ctx *ctx, const float *d_a, const float *d_w, const float *d_bias, int64_t M, int N, int K, int act,
                             float scale, float *d_out)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_a || !d_w || !d_out) return fail(ctx, XB_ERR_INVALID, "xb_linear_f32: null device pointer");
    if (M < 1 || N < 1 || K < 1 || M > ((int64_t)1 << 40) || (act != 0 && act != 1))
        return fail(ctx, XB_ERR_INVALID, "xb_linear_f32: M = %lld, N = %d, K = %d, act = %d; accepted: each size >= 1, act 0 or 1", (long long)M, N, K, act);
    if (act == 1 && !std::isfinite(scale)) return fail(ctx, XB_ERR_INVALID, "xb_linear_f32: scale %g", (double)scale);
    if (int rc = enter(ctx, true)) return rc;
    return xb::linear_f32_run(ctx, d_a, d_w, d_bias, M, N, K, act, scale, d_out);
}

XB_API int xb_wgrad_f32_dev(xb_ctx *ctx, const float *d_a, const float *d_b, int64_t M, int N, int K, float *d_dw, float *d_dcol)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_dw || (M > 0 && (!d_a || !d_b))) return fail(ctx, XB_ERR_INVALID, "xb_wgrad_f32: null device pointer");
    if (M < 0 || N < 1 || K < 1 || M > ((int64_t)1 << 40) || (N + TM - 1) / TM > 65535)
        return fail(ctx, XB_ERR_INVALID, "xb_wgrad_f32: M = %lld, N = %d, K = %d; accepted: M >= 0, N in 1 .. %d, K >= 1", (long long)M, N, K, TM * 65535);
    if (int rc = enter(ctx, true)) return rc;
    return xb::wgrad_f32_run(ctx, d_a, d_b, M, N, K, d_dw, d_dcol, xb::WGRAD_BLOCK_ROWS);
}

// xb_wgrad_f32_dev with another length of the row blocks (a multiple of 32; any value >= M: one running sum), for the
// measurement that chose WGRAD_BLOCK_ROWS.  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_wgrad_blocked(xb_ctx *ctx, const float *d_a, const float *d_b, int64_t M, int N,
                                                                                int K, float *d_dw, float *d_dcol, int64_t block_rows)
{
    if (!ctx || !d_dw || M < 0 || N < 1 || K < 1 || block_rows < 32 || block_rows % 32) return XB_ERR_INVALID;
    if (int rc = enter(ctx, true)) return rc;
    return xb::wgrad_f32_run(ctx, d_a, d_b, M, N, K, d_dw, d_dcol, (long)block_rows);
}

XB_API int xb_head_dz_dev(xb_ctx *ctx, const float *d_y, const float *d_dy, int64_t count, float scale, float *d_dz)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_y || !d_dy || !d_dz) return fail(ctx, XB_ERR_INVALID, "xb_head_dz: null device pointer");
    if (count < 1 || count > ((int64_t)1 << 40)) return fail(ctx, XB_ERR_INVALID, "xb_head_dz: %lld elements", (long long)count);
    if (!(scale > 0.0f) || !std::isfinite(scale)) return fail(ctx, XB_ERR_INVALID, "xb_head_dz: scale %g, a positive number is needed", (double)scale);
    if (int rc = enter(ctx, true)) return rc;
    return xb::head_dz_run(ctx, d_y, d_dy, count, scale, d_dz);
}

}  // extern "C"
