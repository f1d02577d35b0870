// xb_dtw.hip -- xb_dtw_segment: DTW alignment of signal chunks to the expected current levels of their references (the
// reference's src/tools/dtw_segmentation.py; contract: the public header).  Built with -ffp-contract=off: one float64
// addition per cell, bit-equal to the CPU restatement (tests/dtw_ref.py).
//
// One wave per chunk, one launch for up to `count` chunks.  The M = ref_rep * K columns lie across the lanes, C consecutive
// columns per lane (C = 1, 2 or 4 by the widest chunk of the call), in stripes of W = 64 C columns.  A cell needs the
// PREVIOUS row only (g(i-1, j), g(i-1, j-1)), so all lanes work on the same row: per row a lane takes its left neighbour's
// last column of the previous row with one DPP wave shift (two 32-bit moves), the row's sample is wave-uniform, and the
// wave's compare masks ARE the row's choice bits (1 = the diagonal step was taken), 64 columns per 8-byte word.
//
// Feasible cells only: a stripe of columns j0 .. j1 runs rows j0 .. N - M + j1 (j <= i, and M - 1 - j <= N - 1 - i for its
// last column), clipped to the rows the slanted band lets it touch; inside a band every cell is tested exactly as the
// contract writes it.  The corner triangles of a stripe (at most W - 1 rows each) are the only cells computed that no path
// can use; nothing reads them.
//
// Per 64 rows the lanes fetch the batch's samples, the hand-off column of the stripe to the left and (banded) the band
// centres i M / N, one row per lane; a row takes its own with v_readlane.  Choice words and the stripe's last column are
// collected the same way (lane t keeps row t's) and leave with one coalesced store per 64 rows.  The previous row lives in
// 2 C registers per lane; nothing per cell goes to memory but its bit.
//
// Scratch per chunk (owned by the context, sized by the library): ceil(M / W) stripes x roundup64(N - M + W) rows x C words
// of choice bits plus two hand-off columns of N doubles -- 430 KB + 58 KB for 3600 samples against 1200 columns.  The trace
// walks back from (N - 1, M - 1) with wave-uniform control: a batch of choice words (64 rows x C words, one row per lane) is
// fetched into registers, a row's word comes out with v_readlane; lane 0 writes a breakpoint whenever the path leaves a base.
#include <hip/hip_runtime.h>

#include "xb_internal.h"

namespace {

using xb::DtwParams;

constexpr int DPP_WAVE_SHR1 = 0x138;     // lane l takes lane l - 1, lane 0 keeps `old`

__device__ inline double dtw_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// x of the lane to the left; lane 0 takes `first`
__device__ inline double dtw_from_left(double x, double first)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(x), DPP_WAVE_SHR1, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(x), DPP_WAVE_SHR1, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// x of lane l (wave-uniform l) on every lane
__device__ inline double dtw_lane(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

__device__ inline unsigned long long dtw_lane(unsigned long long x, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// rows lo .. hi stripe st (columns st W ..) can reach: j <= i for its first column, M - 1 - j <= N - 1 - i for its last, and
// under a band of half-width wb >= 0 the rows with |j - i M / N| <= wb for one of its columns -- those lie in
// [(j0 - wb) N / M, (j1 + wb) N / M]; a column and a row of slack on either side cover the rounding of the exact test
template <int W, bool BAND>
__device__ inline void dtw_rows(int st, int N, int M, double wb, int &lo, int &hi)
{
    const int j0 = st * W, j1 = (j0 + W < M ? j0 + W : M) - 1;
    lo = j0;
    hi = N - M + j1;
    if (BAND && wb >= 0.0) {
        const double s = (double)N / (double)M;
        double a = floor(((double)j0 - wb - 1.0) * s) - 1.0, b = ceil(((double)j1 + wb + 1.0) * s) + 1.0;
        a = a > -1.0 ? a : -1.0;
        b = b < (double)N ? b : (double)N;
        lo = lo > (int)a ? lo : (int)a;
        hi = hi < (int)b ? hi : (int)b;
    }
}

template <int C, bool BAND>
__global__ __launch_bounds__(64) void dtw_segment_kernel(const DtwParams p)
{
    constexpr int LC = C == 1 ? 0 : (C == 2 ? 1 : 2), W = 64 * C, LW = 6 + LC;
    const int lane = threadIdx.x;
    const int chunk = p.first + blockIdx.x;
    const int N = p.N, rep = p.rep;
    const int o0 = p.off[chunk], K = p.off[chunk + 1] - o0, M = K * rep;
    const double *lev = p.levels + o0;
    const float *q = p.signal + (size_t)chunk * N;
    int32_t *bp = p.bp + (size_t)chunk * p.Kmax;
    const double INF = dtw_inf();
    const double wb = BAND && p.window ? p.window[chunk] : -1.0;
    const double wtest = wb >= 0.0 ? wb : INF;                           // no band: every cell passes
    unsigned long long *words = p.scratch + (size_t)blockIdx.x * p.slot_words;
    double *bnd = reinterpret_cast<double *>(words + p.choice_words);    // two hand-off columns of N values
    const int nst = (M + W - 1) >> LW;
    const size_t SB = xb::dtw_stripe_words(N, M <= N ? M : N, C);

    bool ok = M <= N;
    double cost = INF;
    int lo_prev = 0, hi_prev = -1;
    for (int st = 0; ok && st < nst; ++st) {
        int lo, hi;
        dtw_rows<W, BAND>(st, N, M, wb, lo, hi);
        if (lo > hi) {                                                    // a column no allowed cell reaches: no path
            ok = false;
            break;
        }
        const int j0 = st * W, rows = hi - lo + 1;
        const bool last = st + 1 == nst;
        unsigned long long *sw = words + (size_t)st * SB;
        const double *bin = bnd + (size_t)((st + 1) & 1) * N;
        double *bout = bnd + (size_t)(st & 1) * N;
        double r[C], gp[C], jd[C];
        unsigned long long wacc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = j0 + lane * C + c;
            r[c] = j < M ? lev[j / rep] : 0.0;
            jd[c] = (double)j;
            gp[c] = INF;
            wacc[c] = 0;
        }
        double bacc = INF;
        for (int b0 = 0; b0 < rows; b0 += 64) {
            const int ib = lo + b0 + lane;                               // this lane's row of the batch
            const bool mine = ib <= hi;
            const float qb = mine ? q[ib] : 0.0f;
            double db = INF;                                             // g(ib - 1, j0 - 1): what lane 0 takes from the left
            if (st == 0) db = ib == 0 ? 0.0 : INF;                       // g(0, 0) = d(0, 0) + 0
            else if (mine && ib - 1 >= lo_prev && ib - 1 <= hi_prev) db = bin[ib - 1];
            double cb = 0.0;
            if (BAND) cb = (double)ib * (double)M / (double)N;
            const int nb = rows - b0 < 64 ? rows - b0 : 64;
            for (int t = 0; t < nb; ++t) {
                const double qd = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qb), t));
                const double left = dtw_from_left(gp[C - 1], dtw_lane(db, t));
                const double ci = BAND ? dtw_lane(cb, t) : 0.0;
                double gn[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double stay = gp[c], diag = c ? gp[c - 1] : left;
                    const bool take = diag < stay;                       // ties stay
                    const double best = take ? diag : stay;
                    double g = fabs(qd - r[c]) + best;
                    if (BAND) g = fabs(jd[c] - ci) <= wtest ? g : INF;
                    gn[c] = g;
                    const unsigned long long m = __ballot(take);
                    if (lane == t) wacc[c] = m;
                }
#pragma unroll
                for (int c = 0; c < C; ++c) gp[c] = gn[c];
                if (!last) {
                    const double v = dtw_lane(gp[C - 1], 63);
                    if (lane == t) bacc = v;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) sw[(size_t)(b0 + lane) * C + c] = wacc[c];
            if (!last && mine) bout[ib] = bacc;
        }
        if (last && hi == N - 1) {                                       // the last row ran: g(N - 1, M - 1)
            const int je = M - 1 - j0, ce = je & (C - 1);
            double v = gp[0];
#pragma unroll
            for (int c = 1; c < C; ++c) v = ce == c ? gp[c] : v;
            cost = dtw_lane(v, je >> LC);
        }
        lo_prev = lo;
        hi_prev = hi;
        __threadfence();                                                 // the next stripe / the trace read what other lanes stored
    }
    ok = ok && cost < INF;

    if (ok) {
        int i = N - 1, j = M - 1, k = K - 1, jr = rep - 1;
        if (lane == 0) bp[k] = N;
        int cur_st = -1, cur_b = -1, lo = 0, hi = -1;
        unsigned long long tile[C];
#pragma unroll
        for (int c = 0; c < C; ++c) tile[c] = 0;
        while (i > 0) {
            const int st = j >> LW;
            if (st != cur_st) {
                dtw_rows<W, BAND>(st, N, M, wb, lo, hi);
                cur_st = st;
                cur_b = -1;
            }
            const int rrel = i - lo;
            if (rrel < 0 || i > hi) { ok = false; break; }               // never on a path the forward pass found
            if ((rrel >> 6) != cur_b) {
                cur_b = rrel >> 6;
                const unsigned long long *sw = words + (size_t)st * SB + ((size_t)cur_b * 64 + lane) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) tile[c] = sw[c];
            }
            const int cc = j & (C - 1);
            unsigned long long w = tile[0];
#pragma unroll
            for (int c = 1; c < C; ++c) w = cc == c ? tile[c] : w;
            w = dtw_lane(w, rrel & 63);
            --i;
            if ((w >> ((j & (W - 1)) >> LC)) & 1) {
                if (j == 0) { ok = false; break; }
                --j;
                if (jr == 0) {                                           // row i is the last sample of base k - 1
                    --k;
                    jr = rep - 1;
                    if (lane == 0) bp[k] = i + 1;
                } else {
                    --jr;
                }
            }
        }
        ok = ok && j == 0;
    }
    if (!ok) {                                                           // the reference's naive split
        cost = INF;
        const int each = N / K, more = N % K;
        for (int k = lane; k < K; k += 64) bp[k] = (k + 1) * each + (k + 1 < more ? k + 1 : more);
    }
    for (int k = K + lane; k < p.Kmax; k += 64) bp[k] = 0;
    if (lane == 0) {
        p.ok[chunk] = ok ? 1 : 0;
        p.cost[chunk] = cost;
    }
}

template <int C>
void dtw_launch(const DtwParams &p, bool band, hipStream_t stream)
{
    if (band) hipLaunchKernelGGL((dtw_segment_kernel<C, true>), dim3(p.count), dim3(64), 0, stream, p);
    else hipLaunchKernelGGL((dtw_segment_kernel<C, false>), dim3(p.count), dim3(64), 0, stream, p);
}

}  // namespace

namespace xb {

hipError_t launch_dtw(const DtwParams &p, int cols, bool band, hipStream_t stream)
{
    switch (cols) {
    case 1: dtw_launch<1>(p, band, stream); break;
    case 2: dtw_launch<2>(p, band, stream); break;
    default: dtw_launch<4>(p, band, stream); break;
    }
    return hipGetLastError();
}

}  // namespace xb
