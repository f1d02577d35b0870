// xb_decode.hip -- CRF posterior + max-plus decode for gfx950 (MI355X).
//
// Replaces SeqdistModel.decode_batch (ub-bonito/bonito/crf/model.py:215-218) =
//   seqdist posteriors (Log semiring fwd/bwd scans, crf/model.py:41-46)
//   -> +1e-8 -> log -> seqdist posteriors with the Max semiring -> argmax % (n_base+1)
//   (crf/model.py:92-95), then path_to_str (crf/model.py:97-100) and the left-pack of
//   compute_scores (crf/basecall.py:60-67).
//
// One workgroup per chunk; a CRF state is served by LPS = 1 or 2 adjacent lanes that split its E = nb+1 edges in
// two halves.  The state vectors (alpha, beta, max-plus alpha/beta) live in LDS and are exchanged once per time step
// behind a single LDS-only barrier.  Three sweeps over the scores:
//   1. Log forward           (write alpha)
//   2. Log backward fused with Max backward (read alpha; write bmax) -- also writes the log-posteriors
//      Q = log(P + 1e-8) of every edge, (T, N, S*E) fp32, scattered by destination edge into an LDS row and stored as
//      coalesced rows one step late
//   3. Max forward over Q + per-step arg-max of the max-marginals (read Q, bmax), then pack.
// The quality variant (QS, xb_decode_q) adds a fourth phase after sweep 3: per-step path posteriors from the stashed
// alpha / beta rows, then per-base quality characters, packed beside the bases (see "qualities" below).
// The letter-probability variant (UB, xb_decode_ub; implies QS) also sums, in sweep 2, each step's move-edge posteriors
// per emitted letter (nb floats per step into a per-chunk workspace) and, in the pack, turns them into per-base windowed
// probability bytes of every letter (see "letter probabilities" below).
//
// What bounds a step is the LENGTH OF ITS DEPENDENCY CHAIN, not bytes or instruction count (a dependent VALU
// instruction issues every ~8 cycles, independent ones every ~2.4 per SIMD: tools/valu_probe.hip), so the kernel is
// built to keep the chain short:
//   * sweeps 1 and 3 are "destination owned": a lane's score / Q values are E (or E/2) CONTIGUOUS floats of the row,
//     loaded straight into a register ring RDEPTH steps ahead (no LDS staging); the state vector is kept in LDS in a
//     transposed order, position (i % hi) * nb + i / hi, so that the nb source states of a destination are contiguous;
//     a state's own previous value (the stay edge) never leaves its registers;
//   * sweep 2 is "source owned"; its strided score reads go through an LDS-staged row, and the state -> lane map is
//     permuted (lane group = nb sources that share their destinations) so that those reads are at most 2-way conflicted;
//   * reductions use v_max_f32_dpp / v_add_f32_dpp directly (hipcc emits v_mov_b32_dpp + a separate op + s_nops for the
//     update_dpp builtin); the per-step arg-max is a wave max + ballot (lane order == flat edge order, so the lowest
//     matching lane IS the lowest flat index), per-wave partials go to a 128-step LDS ring and are finalised 64 steps
//     at a time, one step per lane;
//   * the log polynomial is evaluated in Estrin form (depth 4 instead of 8).
//
// Floating-point contract (shared by specification with oracle/xna_oracle.c, written independently): IEEE binary32,
// no contraction (this file is built with -ffp-contract=off), fma only where __builtin_fmaf is written, exp/log are the
// fixed polynomials below, logsumexp = max / exps summed in edge order / log, ties resolve to the lowest
// flat edge index.  The recursions stay in the log domain on purpose (see the oracle's header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "xb_internal.h"
#include "xb_math.h"

namespace {


// ---- the contract's exp / log, scalar and two-wide.  The two-wide forms run the SAME IEEE operations on both
// elements with v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 (a plain wave64 VALU instruction and a packed one both occupy
// the SIMD for 4 cycles, and the kernel is bound by VALU issue); only the integer steps stay per element.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 splat2(float x) { return (f32x2){x, x}; }
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ f32x2 xb_expf2(f32x2 x)
{
    x.x = __builtin_amdgcn_fmed3f(x.x, -87.0f, 88.0f);
    x.y = __builtin_amdgcn_fmed3f(x.y, -87.0f, 88.0f);
    const f32x2 t = fma2(x, splat2(1.44269504088896341f), splat2(XB_EXP_MAGIC));
    const f32x2 n = t - splat2(XB_EXP_MAGIC);
    f32x2 r = fma2(n, splat2(-0.693359375f), x);
    r = fma2(n, splat2(2.12194440e-4f), r);
    f32x2 p = splat2(1.9875691500e-4f);
    p = fma2(p, r, splat2(1.3981999507e-3f));
    p = fma2(p, r, splat2(8.3334519073e-3f));
    p = fma2(p, r, splat2(4.1665795894e-2f));
    p = fma2(p, r, splat2(1.6666665459e-1f));
    p = fma2(p, r, splat2(5.0000001201e-1f));
    const f32x2 r2 = r * r;
    const f32x2 y = fma2(p, r2, r) + splat2(1.0f);
    const f32x2 sc = {xb_exp_scale(t.x), xb_exp_scale(t.y)};
    return y * sc;
}

__device__ __forceinline__ f32x2 xb_logf2(f32x2 x)
{
    f32x2 f, fe;
    {
        float f0, f1, e0, e1;
        xb_log_reduce(x.x, f0, e0);
        xb_log_reduce(x.y, f1, e1);
        f = (f32x2){f0, f1};
        fe = (f32x2){e0, e1};
    }
    const f32x2 z = f * f;
    const f32x2 z2 = z * z;
    const f32x2 z4 = z2 * z2;
    const f32x2 q01 = fma2(splat2(-2.4999993993e-1f), f, splat2(3.3333331174e-1f));
    const f32x2 q23 = fma2(splat2(-1.6668057665e-1f), f, splat2(2.0000714765e-1f));
    const f32x2 q45 = fma2(splat2(-1.2420140846e-1f), f, splat2(1.4249322787e-1f));
    const f32x2 q67 = fma2(splat2(-1.1514610310e-1f), f, splat2(1.1676998740e-1f));
    const f32x2 q03 = fma2(q23, z, q01);
    const f32x2 q47 = fma2(q67, z, q45);
    const f32x2 q07 = fma2(q47, z2, q03);
    const f32x2 p = fma2(splat2(7.0376836292e-2f), z4, q07);
    f32x2 y = (f * z) * p;
    y = fma2(fe, splat2(-2.12194440e-4f), y);
    y = fma2(splat2(-0.5f), z, y);
    f32x2 r = f + y;
    r = fma2(fe, splat2(0.693359375f), r);
    return r;
}

// log of N values, two at a time (the odd last one alone)
template <int N>
__device__ __forceinline__ void xb_log_n(const float (&x)[N], float (&y)[N])
{
#pragma unroll
    for (int r = 0; r + 1 < N; r += 2) {
        const f32x2 v = xb_logf2((f32x2){x[r], x[r + 1]});
        y[r] = v.x;
        y[r + 1] = v.y;
    }
    if (N & 1) y[N - 1] = xb_logf(x[N - 1]);
}

// exp of N values, two at a time (the odd last one alone)
template <int N>
__device__ __forceinline__ void xb_exp_n(const float (&x)[N], float (&y)[N])
{
#pragma unroll
    for (int r = 0; r + 1 < N; r += 2) {
        const f32x2 v = xb_expf2((f32x2){x[r], x[r + 1]});
        y[r] = v.x;
        y[r + 1] = v.y;
    }
    if (N & 1) y[N - 1] = xb_expf(x[N - 1]);
}

__device__ __forceinline__ float maxf(float a, float b) { return b > a ? b : a; }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also fences global memory, i.e. emits
// s_waitcnt vmcnt(0), which would drain the prefetch ring (a full HBM latency) at every time step.
// Inside the sweeps the only cross-thread data is in LDS; the global stashes are re-read by the thread that
// wrote them (and the sweeps are separated by real __syncthreads()).
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- cross-lane arithmetic on DPP, one instruction per step ---------------------------------------------------
// (2 wait states between a VALU write of a register and a DPP read of it: the s_nop 1 in front of every step)
// max over the 64 lanes, valid in lane 63; lanes without a DPP source keep their own value
__device__ __forceinline__ float wave_max63(float v)
{
    asm volatile(
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}
// the same for four independent values at once: the four chains interleave, which also provides the two wait states
// between a register's write and its next DPP read (no s_nop between the levels)
__device__ __forceinline__ void wave_max63_x4(float &a, float &b, float &c, float &d)
{
#define XB_L4(ctrl) \
    "v_max_f32_dpp %0, %0, %0 " ctrl "\n\tv_max_f32_dpp %1, %1, %1 " ctrl "\n\t" \
    "v_max_f32_dpp %2, %2, %2 " ctrl "\n\tv_max_f32_dpp %3, %3, %3 " ctrl "\n\t"
    asm volatile("s_nop 1\n\t"
                 XB_L4("row_shr:1 row_mask:0xf bank_mask:0xf")
                 XB_L4("row_shr:2 row_mask:0xf bank_mask:0xf")
                 XB_L4("row_shr:4 row_mask:0xf bank_mask:0xf")
                 XB_L4("row_shr:8 row_mask:0xf bank_mask:0xf")
                 XB_L4("row_bcast:15 row_mask:0xa bank_mask:0xf")
                 XB_L4("row_bcast:31 row_mask:0xc bank_mask:0xf")
                 "s_nop 1"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef XB_L4
}
// max / sum with the partner lane of a pair (lanes 2s, 2s+1): both lanes receive the result
__device__ __forceinline__ float pair_max(float v)
{
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 0" : "+v"(v));
    return v;
}
// Sum, in edge order 0..E-1, of the E values a lane pair holds (lane 0: edges [0, H) in ex[0..], lane 1: edges [H, E)):
// every term is fetched from the lane that holds it by a fused broadcast-add, so both lanes run the identical chain
// e_0, + e_1, .. + e_{E-1}.  ONE asm statement: all ex[] are inputs, i.e. written before it starts (the leading s_nop
// covers the VALU-write -> DPP-read wait states of the last one); inside, only `s` is written and it is never DPP-read.
#define XB_BC0 "quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t"
#define XB_BC1 "quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t"
template <int E>
__device__ __forceinline__ float pair_sum_ordered(const float (&ex)[(E + 1) / 2])
{
    float s;
    static_assert(E >= 5 && E <= 7, "pair_sum_ordered is written out for 4, 5 and 6 bases");
    if constexpr (E == 5)
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %0, %1 " XB_BC0 "v_add_f32_dpp %0, %2, %0 " XB_BC0 "v_add_f32_dpp %0, %3, %0 " XB_BC0
                     "v_add_f32_dpp %0, %1, %0 " XB_BC1 "v_add_f32_dpp %0, %2, %0 " XB_BC1 "s_nop 0"
                     : "=&v"(s) : "v"(ex[0]), "v"(ex[1]), "v"(ex[2]));
    else if constexpr (E == 6)
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %0, %1 " XB_BC0 "v_add_f32_dpp %0, %2, %0 " XB_BC0 "v_add_f32_dpp %0, %3, %0 " XB_BC0
                     "v_add_f32_dpp %0, %1, %0 " XB_BC1 "v_add_f32_dpp %0, %2, %0 " XB_BC1 "v_add_f32_dpp %0, %3, %0 " XB_BC1 "s_nop 0"
                     : "=&v"(s) : "v"(ex[0]), "v"(ex[1]), "v"(ex[2]));
    else
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %0, %1 " XB_BC0 "v_add_f32_dpp %0, %2, %0 " XB_BC0 "v_add_f32_dpp %0, %3, %0 " XB_BC0
                     "v_add_f32_dpp %0, %4, %0 " XB_BC0
                     "v_add_f32_dpp %0, %1, %0 " XB_BC1 "v_add_f32_dpp %0, %2, %0 " XB_BC1 "v_add_f32_dpp %0, %3, %0 " XB_BC1 "s_nop 0"
                     : "=&v"(s) : "v"(ex[0]), "v"(ex[1]), "v"(ex[2]), "v"(ex[3]));
    return s;
}
#undef XB_BC0
#undef XB_BC1

// Inclusive sum scan over each 16-lane DPP row (Hillis-Steele: x[l] = x[l - d] + x[l] for l >= d, d = 1, 2, 4, 8; a lane
// without a source in its row keeps its value), so that lane 15 of a row ends with the row's sum in that tree order
__device__ __forceinline__ float row16_scan(float v)
{
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}

// CNT consecutive floats from a 4-byte aligned address in the widest pieces (global_load_dwordx4 / x2 / dword)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int CNT>
__device__ __forceinline__ void load_seg(const float *p, float (&r)[CNT])
{
    int o = 0;
    if constexpr (CNT >= 4) {
        const f32x4u v = *reinterpret_cast<const f32x4u *>(p);
        r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
        o = 4;
    }
    if constexpr ((CNT & 3) >= 2) {
        const f32x2u v = *reinterpret_cast<const f32x2u *>(p + (CNT & ~3));
        r[(CNT & ~3)] = v[0]; r[(CNT & ~3) + 1] = v[1];
        o = (CNT & ~3) + 2;
    }
    if constexpr (CNT & 1) r[CNT - 1] = p[CNT - 1];
    (void)o;
}

// Ring depths and occupancy (round 4, tools/r04_decode_variants.sh, profiles/r04_decode_variants.txt): with rings of 4 / 8 steps
// (rounds 2-3: 8 / 16) the nb = 6 kernel fits 168 registers, i.e. three workgroups per CU instead of two (LDS allows three);
// the pass over a co-scheduled pair's 1024 chunks gets 1.9 % (nb 6) / 3.5 % (nb 5) faster, 512 chunks are unchanged, and the
// 1024-thread variants spill less.  The hint is a MINIMUM of three waves per SIMD (a 1024-thread workgroup needs four).
#ifndef XB_DEC_RDEPTH          // (tuning builds override these)
#define XB_DEC_RDEPTH 4
#endif
#ifndef XB_DEC_RDEPTH13
#define XB_DEC_RDEPTH13 8
#endif
#ifndef XB_DEC_WAVES_ATTR
#define XB_DEC_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(3)))
#endif
constexpr int RDEPTH = XB_DEC_RDEPTH;       // register-ring depth (time steps in flight), sweep 2 (a whole staged row per step)
constexpr int RDEPTH13 = XB_DEC_RDEPTH13;   // sweeps 1 and 3: a lane's ring entry is only E (or E/2) floats
constexpr int LRING = 128;    // arg-max partial ring (steps); finalised 64 at a time

// coalesced row staging for sweep 2: NR 16-byte groups per thread, loaded RDEPTH steps ahead, written to LDS per step
template <int NR, int BS>
struct RowRegs {
    f32x4 r[NR];
    __device__ __forceinline__ void load(const float *row, int lim, int tid)
    {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int g = (tid + BS * i) * 4;
            r[i] = *reinterpret_cast<const f32x4 *>(row + (g < lim ? g : 0));
        }
    }
    __device__ __forceinline__ void store(float *lds, int tid) const
    {
#pragma unroll
        for (int i = 0; i < NR; ++i) *reinterpret_cast<f32x4 *>(lds + (tid + BS * i) * 4) = r[i];
    }
};
// the same with 4-byte loads for rows that are not 16-byte aligned (scores handed in with an odd row length)
template <int NR, int BS>
struct RowRegs1 {
    float r[NR];
    __device__ __forceinline__ void load(const float *row, int lim, int tid)
    {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int g = tid + BS * i;
            r[i] = row[g < lim ? g : 0];
        }
    }
    __device__ __forceinline__ void store(float *lds, int tid) const
    {
#pragma unroll
        for (int i = 0; i < NR; ++i) lds[tid + BS * i] = r[i];
    }
};

// Edge bookkeeping of a lane.  A state's E edges are split in two halves [0, H) and [H, E), H = ceil(E/2).
// LPS == 1: the lane owns all E edges (local index r = edge).  LPS == 2: lane `ph` of the pair owns half `ph`
// (local index r = edge - ph * H; the second half has E - H <= H edges, its last local index may be invalid).
template <int E, int LPS>
struct Edges {
    static constexpr int H = (E + 1) / 2;
    static constexpr int EPER = LPS == 1 ? E : H;
};

// NB bases, BS threads (multiple of 64, >= LPS * S), HB: the scores carry the blank column, LPS lanes per state,
// VW: 4 = 16-byte staging loads in sweep 2 (row stride and base 16-byte aligned), 1 = 4-byte loads
// SCAN = true: the xb_crf_scans variant (optional beta / posterior outputs, early return after sweep 1 or 2); the decode
// proper is compiled without those paths (measured: 1-2 % of the decode time when they are run-time branches).
// QS = true: the xb_decode_q variant -- sweep 2 stores the Log backward rows (beta_out), sweep 3 keeps the arg-max state of
// every step, and phase 4 turns them into per-base qualities and moves.  The instantiations with QS = false compile none of it.
// UB = true (with QS): the xb_decode_ub variant -- sweep 2 also reduces each step's move-edge posteriors per letter into
// p.ubuf, and the pack writes every base's letter-probability bytes.  The instantiations with UB = false compile none of it.
template <int NB, int BS, bool HB, int LPS, int VW, bool SCAN, bool QS, bool UB>
__global__ __launch_bounds__(BS) XB_DEC_WAVES_ATTR void crf_decode_kernel(xb::DecodeParams p)
{
    constexpr int E = NB + 1;
    constexpr int H = Edges<E, LPS>::H;
    constexpr int EPER = Edges<E, LPS>::EPER;
    constexpr int NW = BS / 64;
    // Score columns a lane loads per row in sweep 1.  With the blank column: its EPER edge columns (the second lane of a
    // pair loads the LAST EPER columns of the state so that it never reads past the row).  Without it: all NB columns
    // (LPS 1), or E - H columns (LPS 2: first lane columns 0.., second lane columns H-1..).
    constexpr int CPL = HB ? EPER : (LPS == 1 ? NB : E - H);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int S = p.S, hi = p.hi, T = p.T, N = p.N, cin = p.cin, ldq = p.ldq;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x;
    const int st = tid / LPS;
    const int ph = LPS == 1 ? 0 : (tid & 1);      // half served by this lane
    const bool act = st < S;
    const int stc = act ? st : S - 1;              // clamped state (always a valid column)
    const int kcnt = LPS == 1 ? E : (ph == 0 ? H : E - H);   // valid local edge indices: r < kcnt

    // staging pieces per thread: BS * NRS * VW >= S * E >= cin.  BS >= LPS * S, so NRS * VW * LPS >= E is enough (round 5: with two
    // lanes per state half the pieces -- nb = 5: one 16-byte piece per thread instead of two, the staged rows 4 KiB instead of
    // 8 KiB, 25 KB of LDS per workgroup instead of 41 KB: FOUR workgroups per CU, as the registers allow, instead of three)
    constexpr int NRS = VW == 4 ? (E + 4 * LPS - 1) / (4 * LPS) : (E + LPS - 1) / LPS;
    constexpr int cpad = BS * NRS * VW;                // staged row (floats)
    const int lim_m = VW == 4 ? (cin + 3) & ~3 : cin;  // vector loads may touch the row's padding columns
    const int Tpad = (T + RDEPTH13 - 1) / RDEPTH13 * RDEPTH13;   // multiple of both ring depths

    float *sM = reinterpret_cast<float *>(smem_raw);             // [2][cpad]  staged score row (sweep 2)
    float *sQ = sM + 2 * cpad;                                    // [2][cpad]  Q rows being assembled (sweep 2)
    float *sA = sQ + 2 * cpad;                                    // [2][S]  alpha (transposed order) / beta
    float *sX = sA + 2 * S;                                       // [2][S]  max-plus alpha (transposed order) / beta
    float *sG = sX + 2 * S;                                       // [S]     scratch (logZ)
    float *sRv = sG + S;                                          // [LRING][NW] arg-max partials: value
    int *sRi = reinterpret_cast<int *>(sRv + LRING * NW);         // [LRING][NW] arg-max partials: flat edge index
    float *sBc = reinterpret_cast<float *>(sRi + LRING * NW);     // [4] broadcast scratch
    int8_t *sLab = reinterpret_cast<int8_t *>(sBc + 4);           // [T]
    int16_t *sPath = reinterpret_cast<int16_t *>(sLab + ((T + 1) & ~1));   // [T] QS only: arg-max state per step (S <= 1024)
    // [2][S] UB only: move mass of every source state per step (sweep 2), at the next 4-byte boundary behind sPath
    float *sU = reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(sPath + T + 1) & ~(uintptr_t)3);

    const float *sc = p.scores + (size_t)n * p.ld;
    const size_t tstride = (size_t)N * p.ld;
    float *alpha = p.alpha + (size_t)n * S;
    float *bmax = p.bmax + (size_t)n * S;
    const size_t sstride = (size_t)N * S;
    float *qrow = p.qbuf + (size_t)n * ldq;
    const size_t qstride = (size_t)N * ldq;
    const float blank = p.blank;

    // logsumexp tail shared by sweeps 1 and 2: x[r] (invalid entries = -inf), mx = max over the state's edges.
    // The exps are summed in edge order 0..E-1 (the contract's order; LPS == 2: pair_sum_ordered).
    auto lse_tail = [&](const float (&x)[EPER], float mx) -> float {
        float d[EPER], ex[EPER];
#pragma unroll
        for (int r = 0; r < EPER; ++r) d[r] = x[r] - mx;
        xb_exp_n<EPER>(d, ex);
        float s;
        if constexpr (LPS == 1) {
            s = ex[0];
#pragma unroll
            for (int r = 1; r < EPER; ++r) s += ex[r];
        } else {
            s = pair_sum_ordered<E>(ex);
        }
        return mx + xb_logf(s);
    };

    // slot of state i in the transposed state vector of the destination-owned sweeps: the nb sources
    // (k-1) * hi + j / nb, k = 1..nb, of a destination j are the contiguous slots (j / nb) * nb + (k - 1)
    const int dj = stc, djq = dj / NB;
    const int tpos = (dj % hi) * NB + dj / hi;
    // LDS slot read for local edge r: r0slot for r == 0 (the stay edge = the state's own slot for the first half),
    // sbase + r for r >= 1
    const int sbase = djq * NB + (ph == 0 ? -1 : H - 1);
    const int r0slot = ph == 0 ? tpos : djq * NB + H - 1;

    // ------------------------------------------------------------------ sweep 1: Log forward
    {
        const int j = dj;
        // first score column this lane loads, and the register index of local edge r: mv[r + moff]
        const int col0 = HB ? (ph == 0 ? j * E : j * E + E - EPER) : (ph == 0 ? j * NB : j * NB + H - 1);
        if (tid < S) { sA[tid] = 0.0f; alpha[tid] = 0.0f; }        // alpha_0 = 0 in any order
        float ring[RDEPTH13][CPL];
#pragma unroll
        for (int d = 0; d < RDEPTH13; ++d) load_seg<CPL>(sc + (size_t)(d < T ? d : T - 1) * tstride + col0, ring[d]);
        float aown = 0.0f;
        for (int t0 = 0; t0 < Tpad; t0 += RDEPTH13) {
#pragma unroll
          for (int d = 0; d < RDEPTH13; ++d) {
            const int t = t0 + d;                                // >= T in the padding iterations
            float mv[CPL];
#pragma unroll
            for (int r = 0; r < CPL; ++r) mv[r] = ring[d][r];
            load_seg<CPL>(sc + (size_t)(t + RDEPTH13 < T ? t + RDEPTH13 : T - 1) * tstride + col0, ring[d]);
            lds_barrier();
            if (t < T) {                                         // block-uniform
                const float *a0 = sA + (t & 1) * S;
                float x[EPER];
                float mx = -__builtin_inff();
#pragma unroll
                for (int r = 0; r < EPER; ++r) {
                    // score of local edge r.  Register index: with the blank column first half r, second half
                    // r + (EPER - (E - H)); without it first half r - 1 (r >= 1; r == 0 is the constant blank), second
                    // half r.  Indices are compile-time per half, the half is selected per lane.
                    constexpr int SH = EPER - (E - H);           // 0 or 1
                    float m0v, m1v;                              // value if this lane serves half 0 / half 1
                    if (HB) {
                        m0v = mv[r < CPL ? r : CPL - 1];
                        m1v = mv[r + SH < CPL ? r + SH : CPL - 1];
                    } else {
                        m0v = r == 0 ? blank : mv[r - 1 < CPL ? r - 1 : CPL - 1];
                        m1v = mv[r < CPL ? r : CPL - 1];
                    }
                    const float mk = (LPS == 1 || ph == 0) ? m0v : m1v;
                    float ak;
                    if (r == 0) ak = LPS == 1 ? aown : a0[r0slot];
                    else ak = a0[sbase + r];
                    x[r] = r < kcnt ? mk + ak : -__builtin_inff();
                    mx = maxf(mx, x[r]);
                }
                if (LPS == 2) mx = pair_max(mx);
                const float v = lse_tail(x, mx);
                aown = v;
                if (ph == 0 && act) {
                    sA[((t + 1) & 1) * S + tpos] = v;
                    alpha[(size_t)(t + 1) * sstride + j] = v;
                }
            }
          }
        }
        __syncthreads();
    }

    // logZ = logsumexp_j alpha_T[j], summed in order j = 0..S-1 (alpha_T sits in LDS in transposed order)
    {
        const float *aT = sA + (T & 1) * S;
        const int tp = tid < S ? (tid % hi) * NB + tid / hi : 0;
        const float mine = aT[tp];
        const float wm = wave_max63(tid < S ? mine : -__builtin_inff());
        if (lane == 63) sRv[wave] = wm;                          // the partial ring is free until sweep 3
        __syncthreads();
        float mx = sRv[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) mx = maxf(mx, sRv[w]);
        if (tid < S) sG[tid] = xb_expf(mine - mx);
        __syncthreads();
        if (tid == 0) {
            float s = sG[0];
            for (int j = 1; j < S; ++j) s += sG[j];
            const float lz = mx + xb_logf(s);
            sBc[1] = lz;
            if (p.logz) p.logz[n] = lz;
        }
        __syncthreads();
    }
    const float logZ = sBc[1];
    if (SCAN && p.stop_after == 1) return;      // forward scores / partition function only (uniform)
#ifdef XB_LSTM_STAMPS
    if (p.debug_stop == 1) return;   // diagnostic build only: time sweep 1 alone
#endif

    // -------------------------------------------- sweep 2: Log backward + Max backward (fused)
    {
        // source state of this lane (pair), permuted: consecutive groups of NB sources share their NB destinations
        // (i = (st % NB) * hi + st / NB), so the strided reads of the staged row are contiguous inside a group
        const int i = (stc % NB) * hi + stc / NB;
        const int kk = stc % NB + 1;                               // = i / hi + 1: column of the new-base edges
        const int jb = (stc / NB) * NB;                            // = (i % hi) * NB: first destination
        float *beta_out = (SCAN || QS) && p.beta_out ? p.beta_out + (size_t)n * S : nullptr;     // uniform
        const bool post_mode = SCAN && p.post_mode != 0;
        if (tid < S) {
            sA[(T & 1) * S + tid] = 0.0f;
            sX[(T & 1) * S + tid] = 0.0f;
            bmax[(size_t)T * sstride + tid] = 0.0f;
            if (beta_out) beta_out[(size_t)T * sstride + tid] = 0.0f;
        }
        // per-lane constants of local edge r: destination state and staged-row index of its score
        // (e = 0: stay, j = i, column 0; e >= 1: j = jb + e - 1, column kk)
        int dstj[EPER], midx[EPER], qidx[EPER];
        const bool stay0 = LPS == 1 || ph == 0;                    // local edge 0 is the stay edge
#pragma unroll
        for (int r = 0; r < EPER; ++r) {
            const int e = (LPS == 1 ? 0 : ph * H) + r;
            const bool val = r < kcnt;
            const int j = e == 0 ? i : (val ? jb + e - 1 : jb);
            dstj[r] = j;
            midx[r] = HB ? j * E + (e == 0 ? 0 : kk) : (e == 0 ? 0 : j * NB + kk - 1);
            qidx[r] = j * E + ((r == 0 && stay0) ? 0 : kk);       // slot of the edge's Q value in the row being assembled
        }
        int wi = i;                                                // slot of this lane's state in the beta vectors
#ifdef XB_LSTM_STAMPS
        // diagnostic build only (XB_DECODE_LINEAR_LDS=1, results are WRONG): every per-edge LDS access of this sweep at a
        // lane-linear address, i.e. free of bank conflicts -- what the conflicts cost at most (profiles/r04_decode_lds_conflicts.txt)
        if (p.debug_lds) {
#pragma unroll
            for (int r = 0; r < EPER; ++r) {
                dstj[r] = tid % S;
                midx[r] = (tid + BS * r) % cpad;
                qidx[r] = (tid + BS * r) % cpad;
            }
            wi = tid % S;
        }
#endif
        // the Q row of step t is complete once every thread has passed the barrier of step t-1:
        // it is stored (coalesced 16-byte groups) during iteration t-1
        auto store_qrow = [&](int t) {
            const float *src = sQ + (t & 1) * cpad;
            float *dst = qrow + (size_t)t * qstride;
            for (int g = tid * 4; g < ldq; g += BS * 4)
                *reinterpret_cast<f32x4 *>(dst + g) = *reinterpret_cast<const f32x4 *>(src + g);
        };
        // UB: e_t[b] of step t from the move masses of its hi sources b*hi .. b*hi+hi-1 (source order in sU), once every
        // thread has passed the barrier of step t-1.  Lane 16 b + g sums the sources g, g + 16, .. of letter b in increasing
        // order from 0; row16_scan then adds the 16 lanes of the row and lane 15 stores e_t[b] to the chunk's ubuf slice.
        auto ub_reduce = [&](int t) {
            if constexpr (UB) {
#pragma unroll
                for (int l0 = 0; l0 < NB * 16; l0 += BS) {
                    if (l0 + wave * 64 < NB * 16) {              // wave-uniform
                        const int c = l0 + tid, b = c >> 4, g = c & 15;
                        const float *row = sU + (t & 1) * S + (b < NB ? b : 0) * hi;
                        float x = 0.0f;
                        for (int q = g; q < hi; q += 16) x += row[q];
                        x = row16_scan(x);
                        if (g == 15 && b < NB) p.ubuf[((size_t)n * T + t) * NB + b] = x;
                    }
                }
            }
        };
        typename std::conditional<VW == 4, RowRegs<NRS, BS>, RowRegs1<NRS, BS>>::type ring[RDEPTH];
        float aring[RDEPTH];
#pragma unroll
        for (int d = 0; d < RDEPTH; ++d) {
            const int t = T - 1 - d >= 0 ? T - 1 - d : 0;
            ring[d].load(sc + (size_t)t * tstride, lim_m, tid);
            aring[d] = alpha[(size_t)t * sstride + i];
        }
        for (int s0 = 0; s0 < Tpad; s0 += RDEPTH) {
#pragma unroll
          for (int d = 0; d < RDEPTH; ++d) {
            const int t = T - 1 - (s0 + d);                      // < 0 in the padding iterations
            float *m = sM + (t & 1) * cpad;
            ring[d].store(m, tid);
            const float a0 = aring[d];
            {
                const int tn = t - RDEPTH >= 0 ? t - RDEPTH : 0;
                ring[d].load(sc + (size_t)tn * tstride, lim_m, tid);
                aring[d] = alpha[(size_t)tn * sstride + i];
            }
            lds_barrier();
            if (t >= 0 && t + 1 < T) store_qrow(t + 1);
            if (UB && t >= 0 && t + 1 < T) ub_reduce(t + 1);
            if (t >= 0) {                                        // block-uniform
                float *qs = sQ + (t & 1) * cpad;
                const float *b1 = sA + ((t + 1) & 1) * S;
                const float *m1 = sX + ((t + 1) & 1) * S;
                float u[EPER], y[EPER], mjv[EPER];
                float mx = -__builtin_inff(), mm = -__builtin_inff();
#pragma unroll
                for (int r = 0; r < EPER; ++r) {
                    const bool val = r < kcnt;
                    float mv = m[midx[r]];
                    if (!HB && r == 0) mv = stay0 ? blank : mv;
                    const float bj = b1[dstj[r]];
                    mjv[r] = m1[dstj[r]];
                    u[r] = ((a0 + mv) + bj) - logZ;              // log-posterior of the edge
                    y[r] = val ? mv + bj : -__builtin_inff();    // beta recursion term
                    mx = maxf(mx, y[r]);
                }
                if (LPS == 2) mx = pair_max(mx);
                // one two-wide exp per edge: (posterior, logsumexp term)
                float P[EPER], ex[EPER];
#pragma unroll
                for (int r = 0; r < EPER; ++r) {
                    const f32x2 v = xb_expf2((f32x2){u[r], y[r] - mx});
                    P[r] = v.x;
                    ex[r] = v.y;
                }
                float sm;
                if constexpr (LPS == 1) {
                    sm = ex[0];
#pragma unroll
                    for (int r = 1; r < EPER; ++r) sm += ex[r];
                } else {
                    sm = pair_sum_ordered<E>(ex);
                }
                if constexpr (UB) {
                    // move mass of source i: its nb move edges' posteriors summed in edge order 1..nb (from an exact 0 in
                    // place of the stay edge), both halves of a pair in one chain
                    float pm[EPER];
#pragma unroll
                    for (int r = 0; r < EPER; ++r) pm[r] = (r == 0 && stay0) ? 0.0f : P[r];
                    float ms;
                    if constexpr (LPS == 1) {
                        ms = pm[0];
#pragma unroll
                        for (int r = 1; r < EPER; ++r) ms += pm[r];
                    } else {
                        ms = pair_sum_ordered<E>(pm);
                    }
                    if (ph == 0 && act) sU[(t & 1) * S + i] = ms;
                }
                if (post_mode) {                                 // uniform, xb_crf_scans: the row carries P itself (stored here,
#pragma unroll                                                   // so that P is dead before the logs in the decode proper)
                    for (int r = 0; r < EPER; ++r)
                        if (r < kcnt && act) qs[qidx[r]] = P[r];
                }
                // the EPER logs of Q = log(P + 1e-8) and the log of the logsumexp, two at a time
                float la[EPER + 1], lo[EPER + 1];
#pragma unroll
                for (int r = 0; r < EPER; ++r) la[r] = P[r] + 1e-8f;
                la[EPER] = sm;
                xb_log_n<EPER + 1>(la, lo);
                const float bv = mx + lo[EPER];
#pragma unroll
                for (int r = 0; r < EPER; ++r) {
                    if (r < kcnt) {
                        if (act && !post_mode) qs[qidx[r]] = lo[r];
                        mm = maxf(mm, lo[r] + mjv[r]);
                    }
                }
                if (LPS == 2) mm = pair_max(mm);
                if (ph == 0 && act) {
                    sA[(t & 1) * S + wi] = bv;
                    sX[(t & 1) * S + wi] = mm;
                    bmax[(size_t)t * sstride + i] = mm;
                    if (beta_out) beta_out[(size_t)t * sstride + i] = bv;
                }
            }
          }
        }
        lds_barrier();
        store_qrow(0);
        if (UB) ub_reduce(0);
        __syncthreads();
    }

    if (SCAN && p.stop_after == 2) return;      // scans only (uniform)
#ifdef XB_LSTM_STAMPS
    if (p.debug_stop == 2) return;   // diagnostic build only: sweeps 1+2
#endif
    // --------------------------- sweep 3: Max forward over Q + per-step arg-max of the max-marginals
    {
        const int j = dj;
        constexpr int SH = EPER - (E - H);                        // register shift of the second half (0 or 1)
        const int col0 = ph == 0 ? j * E : j * E + E - EPER;      // this lane's first Q column (never past the row)
        const int k0 = LPS == 1 ? 0 : ph * H;
        if (tid < S) sX[tid] = 0.0f;
        float qring[RDEPTH13][EPER];
        float mring[RDEPTH13];
#pragma unroll
        for (int d = 0; d < RDEPTH13; ++d) {
            const int t = d < T ? d : T - 1;
            load_seg<EPER>(qrow + (size_t)t * qstride + col0, qring[d]);
            mring[d] = bmax[(size_t)(t + 1) * sstride + j];
        }
        // finalise the labels of steps [tb, tb + 64): lane l of the calling wave takes step tb + l
        auto finalise = [&](int tb) {
            const int t = tb + lane;
            if (t < T) {
                const float *rv = sRv + (t & (LRING - 1)) * NW;
                const int *ri = sRi + (t & (LRING - 1)) * NW;
                float bv = rv[0];
                int bi = ri[0];
#pragma unroll
                for (int w = 1; w < NW; ++w) {
                    const float v = rv[w];
                    const int c = ri[w];
                    if (v > bv || (v == bv && c < bi)) { bv = v; bi = c; }
                }
                sLab[t] = (int8_t)(bi % E);
                if constexpr (QS) sPath[t] = (int16_t)(bi / E);     // the destination state: the path's state at t + 1
            }
        };
        float aown = 0.0f;
        static_assert(RDEPTH13 % 4 == 0 && RDEPTH13 % RDEPTH == 0, "the arg-max reductions are batched four steps at a time");
        for (int t0 = 0; t0 < Tpad; t0 += RDEPTH13) {
          float bestv[RDEPTH13];
          int bestc[RDEPTH13];
#pragma unroll
          for (int d = 0; d < RDEPTH13; ++d) {
            const int t = t0 + d;                                // >= T in the padding iterations
            float qv[EPER];
#pragma unroll
            for (int r = 0; r < EPER; ++r) qv[r] = qring[d][r];
            const float m1j = mring[d];
            {
                const int tn = t + RDEPTH13 < T ? t + RDEPTH13 : T - 1;
                load_seg<EPER>(qrow + (size_t)tn * qstride + col0, qring[d]);
                mring[d] = bmax[(size_t)(tn + 1) * sstride + j];
            }
            lds_barrier();
            // every 64 steps one wave (taking turns) finalises the 64 steps before this one: their partials were all
            // written before this barrier, and the ring slots being rewritten meanwhile are at least 56 steps away
            if ((t & 63) == 0 && t > 0 && t <= T && wave == ((t >> 6) % NW)) finalise(t - 64);
            bestv[d] = -__builtin_inff();
            bestc[d] = 0x7fffffff;
            if (t < T) {                                         // block-uniform
                const float *am = sX + (t & 1) * S;
                float mm = -__builtin_inff();
                float best = -__builtin_inff();
                int bc = 0x7fffffff;
#pragma unroll
                for (int r = 0; r < EPER; ++r) {
                    const float Q = (LPS == 1 || ph == 0) ? qv[r] : qv[r + SH < EPER ? r + SH : EPER - 1];
                    float av;
                    if (r == 0) av = LPS == 1 ? aown : am[r0slot];
                    else av = am[sbase + r];
                    if (r < kcnt) {
                        mm = maxf(mm, Q + av);
                        const float scv = (av + Q) + m1j;
                        if (scv > best) { best = scv; bc = j * E + k0 + r; }   // increasing flat index
                    }
                }
                if (LPS == 2) mm = pair_max(mm);
                aown = mm;
                if (ph == 0 && act) sX[((t + 1) & 1) * S + tpos] = mm;
                bestv[d] = act ? best : -__builtin_inff();
                bestc[d] = bc;
            }
            // Arg-max over the workgroup's edges, four steps at a time (the four reduction chains interleave; done per
            // step, the serial chain would be the longest part of the step).  Lanes are in flat-index order (state major,
            // the two halves of a state on adjacent lanes) and each lane holds its lowest-index maximiser, so the lowest
            // lane that attains the wave maximum holds the wave's lowest flat index.
            if ((d & 3) == 3) {
                float w0 = bestv[d - 3], w1 = bestv[d - 2], w2 = bestv[d - 1], w3 = bestv[d];
                wave_max63_x4(w0, w1, w2, w3);
                const float wv[4] = {w0, w1, w2, w3};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int tq = t - 3 + q;
                    const float wmx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wv[q]), 63));
                    const unsigned long long hit = __ballot(bestv[d - 3 + q] == wmx);
                    const int wl = __builtin_amdgcn_readfirstlane(hit ? (int)__builtin_ctzll(hit) : 0);
                    const int wc = __builtin_amdgcn_readlane(bestc[d - 3 + q], wl);
                    if (lane == 0 && tq < T) {
                        sRv[(tq & (LRING - 1)) * NW + wave] = wmx;
                        sRi[(tq & (LRING - 1)) * NW + wave] = wc;
                    }
                }
            }
          }
        }
        __syncthreads();
        // the loop finalised steps [0, done): its iterations t = 64, 128, .. <= min(T, Tpad - 1)
        {
            const int last = T < Tpad - 1 ? T : Tpad - 1;
            const int done = (last / 64) * 64;
            if (wave == 0) for (int tb = done; tb < T; tb += 64) finalise(tb);
        }
        __syncthreads();
    }

    // ------------------------------------------------ phase 4 (QS): qualities
    // Per step t the posterior mass of the path state s = sPath[t] and of its nb left- and nb right-shifted neighbours at
    // scan index t + 1, P(x) = exp((alpha_{t+1}[x] + beta_{t+1}[x]) - logZ), summed in the beam search's order (xb_beam.hip),
    // clamped to [0, 1] and raised to 0.4.  Steps are spread over the workgroup; p_t goes to this chunk's slice of the Q
    // buffer, which sweep 3 has finished with (step t at row t / ldq, column t % ldq: ldq contiguous floats per row).
    // The per-base characters are formed in the pack below, one base per emitting step.
    auto pslot = [&](int t) -> float * { return qrow + (size_t)(t / ldq) * qstride + (t % ldq); };
    if constexpr (QS) {
        constexpr int NG = 2 * NB + 1;
        for (int t = tid; t < T; t += BS) {
            const int s = sPath[t];
            const int l0 = s / NB, r0 = (s % hi) * NB;
            const float *a1 = alpha + (size_t)(t + 1) * sstride, *b1 = p.beta_out + (size_t)n * S + (size_t)(t + 1) * sstride;
            int xs[NG];
            xs[0] = s;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                xs[1 + 2 * b] = l0 + hi * b;
                xs[2 + 2 * b] = r0 + b;
            }
            float av[NG], bv[NG], x[NG], P[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                av[g] = a1[xs[g]];
                bv[g] = b1[xs[g]];
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) x[g] = (av[g] + bv[g]) - logZ;
            xb_exp_n<NG>(x, P);
            float pr = P[0];
#pragma unroll
            for (int g = 1; g < NG; ++g) pr = pr + P[g];
            pr = pr > 1.0f ? 1.0f : pr;
            pr = pr < 0.0f ? 0.0f : pr;
            *pslot(t) = pr > 0.0f ? xb_expf(0.4f * xb_logf(pr)) : 0.0f;
        }
        if (p.moves)
            for (int t = tid; t < T; t += BS) p.moves[(size_t)n * T + t] = sLab[t] != 0 ? 1 : 0;
        __syncthreads();
    }
    // quality character of the base emitted at step t: its run is t .. u-1, u = the next emitting step (or T)
    auto qchar = [&](int t) -> int8_t {
        float bp = 0.0f, tot = 0.0f;
        for (int u = t; u < T && (u == t || sLab[u] == 0); ++u) {
            const float pr = *pslot(u), wrong = (1.0f - pr) / (float)(NB - 1);
            bp = bp + pr;
            float one = pr;
#pragma unroll
            for (int j = 1; j < NB; ++j) one = one + wrong;
            tot = tot + one;
        }
        const float e = 1.0f - bp / tot;
        float q = e > 0.0f ? xb_logf(e) * -4.3429448190325175f : 3.402823466e+38f;
        q = q * p.qscale;
        q = q + p.qoffset;
        q = q < 1.0f ? 1.0f : q;
        q = q > 50.0f ? 50.0f : q;
        return (int8_t)(int)(33.5f + q);
    };
    (void)qchar;
    // letter probabilities (UB) of the base emitted at step t, its i-th: window = the steps after the previous emitting step
    // up to before the next one (or 0 / T-1 at the chunk ends); mass[b] = e_u[b] summed over the window in increasing u,
    // tot = mass summed in letter order, byte = min(255, (int)(256 * mass / tot)), all 0 when tot = 0
    auto ubytes = [&](int t, int pos) {
        int u0 = t - 1;
        while (u0 >= 0 && sLab[u0] == 0) --u0;
        int u1 = t + 1;
        while (u1 < T && sLab[u1] == 0) ++u1;
        const float *e = p.ubuf + (size_t)n * T * NB;
        float mass[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) mass[b] = 0.0f;
        for (int u = u0 + 1; u < u1; ++u) {
#pragma unroll
            for (int b = 0; b < NB; ++b) mass[b] = mass[b] + e[(size_t)u * NB + b];
        }
        float tot = mass[0];
#pragma unroll
        for (int b = 1; b < NB; ++b) tot = tot + mass[b];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            int v = 0;
            if (tot > 0.0f) {
                v = (int)(256.0f * (mass[b] / tot));
                v = v > 255 ? 255 : v;
            }
            p.probs[((size_t)n * NB + b) * T + pos] = (uint8_t)v;
        }
    };
    (void)ubytes;

    // ------------------------------------------------ labels out + path_to_str + left-pack
    if (p.labels)
        for (int t = tid; t < T; t += BS) p.labels[(size_t)n * T + t] = sLab[t];
    if (p.seq || p.seq_len) {
        int *sCnt = reinterpret_cast<int *>(sM);      // BS+1 ints; the row staging is free now
        const int per = (T + BS - 1) / BS;
        const int lo = tid * per, hiT = (lo + per < T) ? lo + per : T;
        int cnt = 0;
        for (int t = lo; t < hiT; ++t) cnt += sLab[t] != 0;
        sCnt[tid + 1] = cnt;
        __syncthreads();
        if (tid == 0) {
            sCnt[0] = 0;
            for (int w = 1; w <= BS; ++w) sCnt[w] += sCnt[w - 1];
        }
        __syncthreads();
        const int total = sCnt[BS];
        if (p.seq) {
            int8_t *out = p.seq + (size_t)n * T;
            int pos = sCnt[tid];
            for (int t = lo; t < hiT; ++t) {
                const int l = sLab[t];
                if (l != 0) {
                    if constexpr (QS) p.qstr[(size_t)n * T + pos] = qchar(t);     // packed in parallel with the bases
                    if constexpr (UB) ubytes(t, pos);
                    out[pos++] = (int8_t)p.alphabet[l];
                }
            }
            for (int t = total + tid; t < T; t += BS) out[t] = 0;
            if constexpr (QS)
                for (int t = total + tid; t < T; t += BS) p.qstr[(size_t)n * T + t] = 0;
            if constexpr (UB)
                for (int b = 0; b < NB; ++b)
                    for (int t = total + tid; t < T; t += BS) p.probs[((size_t)n * NB + b) * T + t] = 0;
        }
        if (p.seq_len && tid == 0) p.seq_len[n] = total;
    }
}

template <int NB, int BS, int LPS, bool SCAN, bool QS, bool UB>
hipError_t launch_nb_bs(const xb::DecodeParams &p, int vw, hipStream_t stream)
{
    // must mirror the kernel's LDS carve
    constexpr int E = NB + 1;
    auto lds_bytes = [&](int w) {
        const int nrs = w == 4 ? (E + 4 * LPS - 1) / (4 * LPS) : (E + LPS - 1) / LPS;      // the kernel's NRS
        const size_t cpad = (size_t)BS * nrs * w;
        size_t b = sizeof(float) * (4 * cpad + 5 * (size_t)p.S + (size_t)LRING * (BS / 64)) +
                   sizeof(int) * (size_t)LRING * (BS / 64) + sizeof(float) * 4 + (size_t)p.T;
        if (QS) b += 1 + sizeof(int16_t) * (size_t)p.T;        // sPath behind sLab, at the next even byte
        if (UB) b = ((b + 3) & ~(size_t)3) + sizeof(float) * 2 * (size_t)p.S;   // sU behind sPath, at the next 4-byte boundary
        return (b + 15) & ~(size_t)15;
    };
    // the four-wide row loads pad a state's edges to a multiple of four: where that no longer fits (4^5 states), one by one
    if (vw == 4 && lds_bytes(4) > 160 * 1024) vw = 1;
    const size_t lds = lds_bytes(vw);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    dim3 grid(p.N), block(BS);
#define XB_LAUNCH(HB, VW)                                                                                          \
    do {                                                                                                           \
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&crf_decode_kernel<NB, BS, HB, LPS, VW, SCAN, QS, UB>),         \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                           \
        hipLaunchKernelGGL((crf_decode_kernel<NB, BS, HB, LPS, VW, SCAN, QS, UB>), grid, block, lds, stream, p);                 \
    } while (0)
    if (p.has_blank) {
        if (vw == 4) XB_LAUNCH(true, 4); else XB_LAUNCH(true, 1);
    } else {
        if (vw == 4) XB_LAUNCH(false, 4); else XB_LAUNCH(false, 1);
    }
#undef XB_LAUNCH
    return hipGetLastError();
}

// Block = smallest multiple of 64 threads (from a short list, pruned per alphabet) that holds LPS lanes for each state.
template <int NB, int LPS, bool SCAN, bool QS = false, bool UB = false>
hipError_t launch_nb_lps(const xb::DecodeParams &p, int vw, hipStream_t stream)
{
    const int need = LPS * p.S;
    if (need <= 64) return launch_nb_bs<NB, 64, LPS, SCAN, QS, UB>(p, vw, stream);
    if (need <= 128) return launch_nb_bs<NB, 128, LPS, SCAN, QS, UB>(p, vw, stream);
    if (need <= 256) return launch_nb_bs<NB, 256, LPS, SCAN, QS, UB>(p, vw, stream);
    if constexpr (NB == 6) {
        if (need <= 448) return launch_nb_bs<NB, 448, LPS, SCAN, QS, UB>(p, vw, stream);     // 2 x 216 states
    } else {
        if (need <= 640) return launch_nb_bs<NB, 640, LPS, SCAN, QS, UB>(p, vw, stream);     // 5^4 states / 2 x 4^4
        if constexpr (NB == 4 && LPS == 1) {
            if (need <= 1024) return launch_nb_bs<NB, 1024, LPS, SCAN, QS, UB>(p, vw, stream);   // 4^5 states
        }
    }
    return hipErrorInvalidValue;
}
template <int NB>
hipError_t launch_nb(const xb::DecodeParams &p, int vw, hipStream_t stream)
{
    // the letter-probability variant (validated by launch_crf_decode: the quality variant's outputs and ubuf set)
    if (p.probs) {
        if (xb::decode_lanes_per_state(p.S, p.N) == 2) return launch_nb_lps<NB, 2, false, true, true>(p, vw, stream);
        return launch_nb_lps<NB, 1, false, true, true>(p, vw, stream);
    }
    // the quality variant, with either lane split (validated by launch_crf_decode: full decode, beta_out and seq set)
    if (p.qstr) {
        if (xb::decode_lanes_per_state(p.S, p.N) == 2) return launch_nb_lps<NB, 2, false, true>(p, vw, stream);
        return launch_nb_lps<NB, 1, false, true>(p, vw, stream);
    }
    // the scan variant exists with one lane per state only (the results do not depend on the lane split)
    if (p.stop_after || p.beta_out || p.post_mode) return launch_nb_lps<NB, 1, true>(p, vw, stream);
    if (xb::decode_lanes_per_state(p.S, p.N) == 2) return launch_nb_lps<NB, 2, false>(p, vw, stream);
    return launch_nb_lps<NB, 1, false>(p, vw, stream);
}

}  // namespace

namespace xb {

int decode_lanes_per_state(int S, int N)
{
    if (const char *e = getenv("XB_DECODE_LPS")) {
        const int v = atoi(e);
        if ((v == 1 || v == 2) && v * S <= 1024) return v;
    }
    // Two lanes per state halve the per-lane chain of exps at the price of a workgroup twice as wide (the pair's per-state
    // work is done by both lanes).  That pays while the batch leaves a CU only ~2 workgroups; with more chunks per CU the
    // narrower workgroup wins.  Measured on MI355X, T = 2000 (ms, 2 lanes vs 1 lane): S = 125: N = 512 3.78 vs 4.77,
    // N = 1024 7.16 vs 6.22, N = 2048 12.99 vs 12.20; S = 216: N = 512 8.72 vs 6.28, N = 1024 17.41 vs 12.22.
    return (2 * S <= 256 && N <= 768) ? 2 : 1;
}

// Host-side launch.  Shapes are validated here so the kernel's indexing assumptions hold:
//   S = NB^state_len <= 1024, cin = S*(NB+1) or S*NB, ld >= cin (the pack scratch of BS+1 ints always
//   fits the staging area).
hipError_t launch_crf_decode(const DecodeParams &p, hipStream_t stream)
{
    if (p.S < 1 || p.S > 1024 || p.T < 1 || p.N < 1) return hipErrorInvalidValue;
    if (p.S % p.nb != 0 || p.hi * p.nb != p.S) return hipErrorInvalidValue;
    const int E = p.nb + 1;
    if (p.cin != (p.has_blank ? p.S * E : p.S * p.nb) || p.ld < p.cin) return hipErrorInvalidValue;
    if (!p.qbuf || p.ldq % 4 != 0 || p.ldq < p.S * E || reinterpret_cast<uintptr_t>(p.qbuf) % 16 != 0) return hipErrorInvalidValue;
    if (p.qstr && (!p.seq || !p.beta_out || p.stop_after || p.post_mode)) return hipErrorInvalidValue;
    if (p.probs && (!p.qstr || !p.ubuf)) return hipErrorInvalidValue;
    int vw = 1;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p.scores);
    // vector loads may run into the row's padding columns (ld >= cin rounded up), never past the row
    if (p.ld % 4 == 0 && p.ld >= ((p.cin + 3) & ~3) && a % 16 == 0) vw = 4;
    switch (p.nb) {
    case 4: return launch_nb<4>(p, vw, stream);
    case 5: return launch_nb<5>(p, vw, stream);
    case 6: return launch_nb<6>(p, vw, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace xb
