// xb_ctc.hip -- the CTC-CRF lattice: seqdist.ctc_simple's recursion over the stay / move edges of a label row
// (CTC_CRF.ctc_loss / ctc_viterbi_alignments, ub-bonito/bonito/crf/model.py:102-135), one pair of sweeps (CtcSweep) behind three
// kernels (xb_internal.h CtcParams, CtcLossParams, CtcGradParams; the contracts are in the public header):
//   ctc_scan_kernel   xb_ctc_logz, xb_ctc_alignments: the scores as given; Log forward and backward with the restricted
//                     posteriors stored, or Max forward and the back-trace of the best path;
//   ctc_loss_kernel   xb_ctc_loss, xb_validate_chunks: the Log forward sweep on the encoder's RAW scores in either layout;
//   ctc_grad_kernel   xb_ctc_loss_grad, every trainer's step: both Log sweeps on RAW scores, the restricted posteriors summed
//                     per score column into d loss / d scores (the sweeps' loop bodies in a copy of its own, see there).
// What they share:
//   - the gather columns of prepare_ctc_scores come from the uint8 labels in the kernel (ctc_columns, xb_ctc_lattice.h);
//   - RAW scores are normalised where they are used, s - logz_crf / T: one correctly rounded division per chunk, one
//     subtraction per score, as Model.normalise does on the host.  Folding T * c into the result would save the subtractions
//     and round differently.  The scan kernel's scores are used as they are: no subtraction at all;
//   - a position feeds itself and its right neighbour alone, so the ones beyond the chunk's own length, tlen - sl, never reach
//     the end cell: the loss and gradient kernels compute the chunk's own positions only.  The scan computes the row's full
//     width, because its outputs have it: the restricted posterior of a cell beyond the chunk's end is xb_expf of about -1e38,
//     which clamps its argument and gives exp(-87) = 1.6458115e-38f, not zero (and other values in a chunk without a path);
//   - one workgroup per chunk, position l on thread l % threads (PMAX positions per thread; ctc_launch, xb_ctc_lattice.h); the
//     position vector is double buffered in LDS with one barrier per time step, the scores of a position come through a
//     CTC_RD-deep register ring;
//   - the arithmetic: xb_expf / xb_logf, sum2 = max, exp, exp, add, log, the stay term before the move term.  Built without
//     contraction; written independently of oracle/xna_oracle.c: xo_ctc_logz and bit-equal to it.
#include <type_traits>

#include "xb_internal.h"
#include "xb_math.h"

namespace {

using xb::CTC_MAX_THREADS;
using xb::CTC_PMAX;
constexpr int CTC_RD = 4;                        // the score ring's depth in time steps
constexpr float CTC_ZERO = -1e38f;               // seqdist's Log.zero / Max.zero

template <bool MAXS>
__device__ __forceinline__ float ctc_sum2(float x0, float x1)
{
    const float m = x0 > x1 ? x0 : x1;
    if (MAXS) return m;
    return m + xb_logf(xb_expf(x0 - m) + xb_expf(x1 - m));
}

// The two sweeps over n positions of one chunk whose paths end in position `end` - 1, for the thread's positions
// l = tid + k BS, k < PMAX.
// HB: the scores have the blank column (else the stay score is the constant `blank`); NORM: RAW scores, `- c` at the use.
template <int PMAX, bool HB, bool NORM>
struct CtcSweep {
    int tid, BS, n, end, T, vs;
    float *vec;                  // LDS [2][n + 2]: slot l + 1 = position l, slots 0 and n + 1 = `zero`
    const float *srow;           // the chunk's scores at step 0; tstride floats to the next step
    size_t tstride;
    float c, stay_nb;            // NORM: logz_crf / T; the stay score of the blank-less layout
    // the thread's gather columns: stay (own), the move into the position (l - 1 -> l) and out of it (l -> l + 1)
    int cs[PMAX], cin[PMAX], cout[PMAX];
    // The ring holds RAW scores and `- c` happens where they are used: a load with arithmetic behind it, or one under a
    // per-position predicate, makes the compiler wait for it on the spot (vmcnt(0) every step).  So every load of the sweeps is
    // unconditional -- a slot without a position reads column 0 of the row -- and nothing touches its value before its step.
    float rs[CTC_RD][PMAX], rm[CTC_RD][PMAX], ra[CTC_RD][PMAX];

    __device__ __forceinline__ void init(float *vec_, const float *srow_, size_t tstride_, int T_, int n_, int end_, float c_,
                                         float blank)
    {
        tid = threadIdx.x; BS = blockDim.x; n = n_; end = end_; T = T_; vs = n_ + 2;
        vec = vec_; srow = srow_; tstride = tstride_;
        c = c_; stay_nb = NORM ? blank - c_ : blank;
    }

    // cpm: the move column into the position in the posteriors' (blank) layout
    __device__ __forceinline__ void columns(const uint8_t *lab, int nb, int sl, int (&cpm)[PMAX])
    {
#pragma unroll
        for (int k = 0; k < PMAX; ++k) {
            const int l = tid + k * BS;
            cs[k] = cin[k] = cout[k] = cpm[k] = 0;
            if (l < n) {
                xb::ctc_columns<HB>(lab, l, nb, sl, cs[k], cin[k], cpm[k]);
                if (l + 1 < n) {
                    int s1, p1;
                    xb::ctc_columns<HB>(lab, l + 1, nb, sl, s1, cout[k], p1);
                }
            }
        }
    }

    __device__ __forceinline__ float stay(float raw) const { return HB ? (NORM ? raw - c : raw) : stay_nb; }
    __device__ __forceinline__ float move(float raw) const { return NORM ? raw - c : raw; }

    __device__ __forceinline__ void fetch(int t, float (&s_)[PMAX], float (&m_)[PMAX], const int (&cmv)[PMAX])
    {
        const float *row = srow + (size_t)(t < 0 ? 0 : (t >= T ? T - 1 : t)) * tstride;
#pragma unroll
        for (int k = 0; k < PMAX; ++k) {
            if (HB) s_[k] = row[cs[k]];
            m_[k] = row[cmv[k]];
        }
    }

    // alpha_{t+1}[l] = sum2(alpha_t[l] + stay[t][l], alpha_t[l-1] + move[t][l-1]) -> alpha_T[end - 1], behind a barrier.
    // STASH: alpha_t[l] to stash[t * n + l], t = 0 .. T
    template <bool MAXS, bool STASH>
    __device__ __forceinline__ float forward(float *stash)
    {
        for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTC_ZERO;
        __syncthreads();
        if (tid == 0) vec[1] = 0.0f;                             // alpha_0: `one` at position 0
        if (STASH) {
#pragma unroll
            for (int k = 0; k < PMAX; ++k) {
                const int l = tid + k * BS;
                if (l < n) stash[l] = l == 0 ? 0.0f : CTC_ZERO;
            }
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < CTC_RD; ++d) fetch(d, rs[d], rm[d], cin);
        int cur = 0;
        for (int t0 = 0; t0 < T; t0 += CTC_RD) {
#pragma unroll
            for (int d = 0; d < CTC_RD; ++d) {
                const int t = t0 + d;
                if (t < T) {                                   // uniform
                    const float *vc = vec + cur * vs;
                    float *vn = vec + (cur ^ 1) * vs;
#pragma unroll
                    for (int k = 0; k < PMAX; ++k) {
                        const int l = tid + k * BS;
                        if (l < n) {
                            const float x0 = vc[l + 1] + stay(rs[d][k]);
                            const float x1 = l > 0 ? vc[l] + move(rm[d][k]) : CTC_ZERO;
                            const float v = ctc_sum2<MAXS>(x0, x1);
                            vn[l + 1] = v;
                            if (STASH) stash[(size_t)(t + 1) * n + l] = v;
                        }
                    }
                    fetch(t + CTC_RD, rs[d], rm[d], cin);
                    __syncthreads();
                    cur ^= 1;
                }
            }
        }
        return vec[cur * vs + end];
    }

    // Log: beta_t[l] = sum2(stay[t][l] + beta_{t+1}[l], move[t][l] + beta_{t+1}[l+1]) over forward's stash.  Per step t, from
    // T - 1 down: emit(t, l, a, st, mv, bn, bx, lz) for each of the thread's positions -- alpha_t[l], the two scores as used, beta_{t+1}
    // of l and of l + 1 (`zero` behind the last position): the restricted posteriors are exp(((a + st) + bn) - lz) for the stay
    // edge and exp(((a + mv) + bx) - lz) for the move out of l -- then, behind the step's barrier, after(t).
    template <typename Emit, typename After>
    __device__ __forceinline__ void backward(const float *stash, float lz, Emit &&emit, After &&after)
    {
        __syncthreads();                                       // every thread has read alpha_T
        for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTC_ZERO;
        __syncthreads();
        if (tid == 0) vec[end] = 0.0f;                         // beta_T: `one` at the end position
        __syncthreads();
        auto fetch_back = [&](int t, float (&s_)[PMAX], float (&m_)[PMAX], float (&a_)[PMAX]) {
            fetch(t, s_, m_, cout);
            const float *arow = stash + (size_t)(t < 0 ? 0 : t) * n;
#pragma unroll
            for (int k = 0; k < PMAX; ++k) a_[k] = arow[tid + k * BS < n ? tid + k * BS : 0];
        };
#pragma unroll
        for (int d = 0; d < CTC_RD; ++d) fetch_back(T - 1 - d, rs[d], rm[d], ra[d]);
        int cur = 0;
        for (int t0 = T - 1; t0 >= 0; t0 -= CTC_RD) {
#pragma unroll
            for (int d = 0; d < CTC_RD; ++d) {
                const int t = t0 - d;
                if (t >= 0) {                                  // uniform
                    const float *vc = vec + cur * vs;
                    float *vn = vec + (cur ^ 1) * vs;
#pragma unroll
                    for (int k = 0; k < PMAX; ++k) {
                        const int l = tid + k * BS;
                        if (l < n) {
                            const float a = ra[d][k], st = stay(rs[d][k]), mv = move(rm[d][k]);
                            const float bn = vc[l + 1];
                            const float bx = l + 1 < n ? vc[l + 2] : CTC_ZERO;
                            emit(t, l, a, st, mv, bn, bx, lz);
                            const float x0 = st + bn;
                            const float x1 = l + 1 < n ? mv + bx : CTC_ZERO;
                            vn[l + 1] = ctc_sum2<false>(x0, x1);
                        }
                    }
                    fetch_back(t - CTC_RD, rs[d], rm[d], ra[d]);
                    __syncthreads();
                    cur ^= 1;
                    after(t);
                }
            }
        }
    }
};

// ---- the scans on given scores (xb_ctc_logz, xb_ctc_alignments) -------------------------------------------------------------
template <int PMAX, bool MAXS, bool STASH>
__global__ __launch_bounds__(CTC_MAX_THREADS) void ctc_scan_kernel(xb::CtcParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctc_smem[];
    const int tid = threadIdx.x, b = blockIdx.x, T = p.T, np = p.Lt - (p.sl - 1);
    const int len = p.tlen[b];
    if (len < p.sl || len > p.Lt) {
        if (tid == 0) atomicOr(p.error, 2u);
        return;
    }
    const int n = np;                                            // the row's positions, <= PMAX * blockDim.x; the chunk ends at len - sl
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    CtcSweep<PMAX, true, false> s;
    s.init(reinterpret_cast<float *>(ctc_smem), p.scores + (size_t)b * p.C, (size_t)p.N * p.C, T, n, len + 1 - p.sl, 0.0f, 0.0f);
    int cpm[PMAX];
    s.columns(lab, p.nb, p.sl, cpm);
    float *stash = STASH ? p.alpha + (size_t)b * (T + 1) * np : nullptr;         // alpha_t[l] at t * n + l
    const float lz = s.template forward<MAXS, STASH>(stash);
    if (tid == 0 && p.logz) p.logz[b] = lz;
    if (!STASH) return;
    if (!MAXS) {
        s.backward(stash, lz,
                   [&](int t, int l, float a, float st, float mv, float bn, float bx, float lz_) {
                       if (p.gstay) p.gstay[((size_t)t * p.N + b) * np + l] = xb_expf(((a + st) + bn) - lz_);
                       if (p.gmove && l + 1 < n) p.gmove[((size_t)t * p.N + b) * (np - 1) + l] = xb_expf(((a + mv) + bx) - lz_);
                   },
                   [](int) {});
    } else if (p.gstay) {
        // ---- back-trace of the max path (one lane; T dependent steps): the alignment rows were zeroed by the host
        __threadfence_block();
        if (tid == 0) {
            int l = s.end - 1, cs, cm, cp;
            xb::ctc_columns<true>(lab, l, p.nb, p.sl, cs, cm, cp);
            for (int t = T - 1; t >= 0; --t) {
                const float *row = s.srow + (size_t)t * s.tstride;
                const float *a = stash + (size_t)t * n;
                const float x0 = a[l] + row[cs];
                const float x1 = l > 0 ? a[l - 1] + row[cm] : CTC_ZERO;
                if (!(x0 >= x1)) {                          // the move edge was strictly better (ties prefer the stay edge)
                    l -= 1;
                    xb::ctc_columns<true>(lab, l, p.nb, p.sl, cs, cm, cp);
                }
                p.gstay[((size_t)t * p.N + b) * np + l] = 1.0f;
            }
        }
    }
}

// uniform: a length outside [sl, Lt] or a label above nb inside it
__device__ __forceinline__ int ctc_bad_row(const uint8_t *lab, int len, int Lt, int nb, int sl)
{
    int bad = len < sl || len > Lt;
    if (!bad)
        for (int j = threadIdx.x; j < len; j += blockDim.x) bad |= lab[j] > nb;
    return __syncthreads_or(bad);
}

// ---- the validation loss (xb_ctc_loss) ---------------------------------------------------------------------------------------
template <int PMAX, bool HB>
__global__ __launch_bounds__(CTC_MAX_THREADS) void ctc_loss_kernel(xb::CtcLossParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctc_smem[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int len = p.tlen[b];
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    if (ctc_bad_row(lab, len, p.Lt, p.nb, p.sl)) {
        if (tid == 0) atomicOr(p.error, 4u);
        return;
    }
    CtcSweep<PMAX, HB, true> s;
    const int n = len + 1 - p.sl;                                // this chunk's positions, 1 .. Lt - sl + 1 <= PMAX * blockDim.x
    s.init(reinterpret_cast<float *>(ctc_smem), p.scores + (size_t)b * p.ld, (size_t)p.N * p.ld, p.T, n, n,
           p.logz_crf[b] / (float)p.T, p.blank);
    int cpm[PMAX];
    s.columns(lab, p.nb, p.sl, cpm);
    const float lz = s.template forward<false, false>(nullptr);  // alpha_T[len - sl]
    if (tid == 0) {
        if (p.logz) p.logz[b] = lz;
        p.loss[b] = -(lz / (float)len);
    }
}

// ---- the loss with its gradient (xb_ctc_loss_grad) ---------------------------------------------------------------------------
// ctc_grad_kernel: the forward sweep with alpha stashed, then the backward sweep with the restricted posteriors scattered over
// their score columns.  Positions that share a column (a repeated k-mer: a homopolymer run, a recurring k-mer) are linked once
// per chunk into chains of ascending position; per time step the posteriors go to LDS and the chain's first position adds its
// chain serially from 0.0f -- the order np.add.at gives, the same on every run, no floating-point atomic anywhere.  It writes
// (sum - P) * w for the columns the chunk's positions map to; ctc_grad_fill_kernel writes (0.0f - P) * w into all the others, at
// memory speed and off the lattice's latency chain.
// Its two loop bodies are CtcSweep's written out again, on the shared columns, constants and sum2: through CtcSweep and its
// per-step functors the call took 2.8 % longer at 64 chunks (3.30 against 3.21 ms, profiles/ctc_lattice_refactor_ab.txt), and a
// trainer's step waits for it.  tests/test_gpu_ctcgrad.py holds the two to the same bytes (the host route runs ctc_scan_kernel).
// LDS: vec [2][np + 2] | g [2][2][np] (during the chain build: the positions' columns) | next [2][np] u16 | not-head [2][np] u8.
constexpr int CTCG_NONE = 0xffff;

template <int PMAX, bool HB>
__global__ __launch_bounds__(CTC_MAX_THREADS) void ctc_grad_kernel(xb::CtcGradParams q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctc_smem[];
    const xb::CtcLossParams &p = q.l;
    const int tid = threadIdx.x, BS = blockDim.x, b = q.first + blockIdx.x, T = p.T, nb = p.nb, sl = p.sl;
    const int npmax = p.Lt - (sl - 1);
    float *vec = reinterpret_cast<float *>(ctc_smem);           // [2][npmax + 2]
    float *g = vec + 2 * (npmax + 2);                            // [buffer][stay, move][npmax]
    int *col = reinterpret_cast<int *>(g);                       // [stay, move][npmax], until the chains stand
    unsigned short *nxt = reinterpret_cast<unsigned short *>(g + 4 * npmax);      // [stay, move][npmax]
    unsigned char *nothead = reinterpret_cast<unsigned char *>(nxt + 2 * npmax);  // [stay, move][npmax]
    const int len = p.tlen[b];
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    if (ctc_bad_row(lab, len, p.Lt, nb, sl)) {                  // the fill kernel zeroes this chunk's gradient
        if (tid == 0) atomicOr(p.error, 4u);
        return;
    }
    const int n = len + 1 - sl;                                  // this chunk's positions, 1 .. npmax <= PMAX * BS
    const float c = p.logz_crf[b] / (float)T;
    const float stay_nb = p.blank - c;
    const float *srow = p.scores + (size_t)b * p.ld;
    const size_t tstride = (size_t)p.N * p.ld;
    float *stash = q.stash + (size_t)blockIdx.x * q.slot;        // alpha_t[l] at t * n + l, t = 0 .. T
    const int vs = n + 2;
    // this thread's positions: the stay column, the move columns into and out of the position, the move column into it in P
    int cs[PMAX], cin[PMAX], cout[PMAX], cpm[PMAX];
#pragma unroll
    for (int k = 0; k < PMAX; ++k) {
        const int l = tid + k * BS;
        cs[k] = cin[k] = cout[k] = cpm[k] = 0;
        if (l < n) {
            xb::ctc_columns<HB>(lab, l, nb, sl, cs[k], cin[k], cpm[k]);
            if (l + 1 < n) {
                int s1, p1;
                xb::ctc_columns<HB>(lab, l + 1, nb, sl, s1, cout[k], p1);
            }
            col[l] = cs[k];
            col[npmax + l] = cin[k];
            nxt[l] = nxt[npmax + l] = CTCG_NONE;
            nothead[l] = nothead[npmax + l] = 0;
        }
    }
    __syncthreads();
    // ---- the chains: the next position with the same column; a position some earlier one points at is no head
    unsigned heads = 0;                                          // bit k: stay head, bit 16 + k: move head
#pragma unroll
    for (int k = 0; k < PMAX; ++k) {
        const int l = tid + k * BS;
        if (l < n) {
            if (HB) {
                for (int j = l + 1; j < n; ++j)
                    if (col[j] == cs[k]) { nxt[l] = (unsigned short)j; nothead[j] = 1; break; }
            }
            if (l > 0) {
                for (int j = l + 1; j < n; ++j)
                    if (col[npmax + j] == cin[k]) { nxt[npmax + l] = (unsigned short)j; nothead[npmax + j] = 1; break; }
            }
        }
    }
    __syncthreads();
    int nxs[PMAX], nxm[PMAX];                                    // a head's second position: most chains end at their head
#pragma unroll
    for (int k = 0; k < PMAX; ++k) {
        const int l = tid + k * BS;
        nxs[k] = nxm[k] = CTCG_NONE;
        if (l < n) {
            if (HB && !nothead[l]) { heads |= 1u << k; nxs[k] = nxt[l]; }
            if (l > 0 && !nothead[npmax + l]) { heads |= 1u << (16 + k); nxm[k] = nxt[npmax + l]; }
        }
    }
    __syncthreads();                                             // the columns are read: g may be written
    for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTC_ZERO;
    __syncthreads();
    if (tid == 0) vec[1] = 0.0f;                                 // alpha_0: `one` at position 0
#pragma unroll
    for (int k = 0; k < PMAX; ++k) {
        const int l = tid + k * BS;
        if (l < n) stash[l] = l == 0 ? 0.0f : CTC_ZERO;
    }
    __syncthreads();

    // ---- forward, CtcSweep::forward's with the stash: alpha_{t+1}[l] = sum2(alpha_t[l] + stay[t][l], alpha_t[l-1] + move[t][l-1])
    float rs[CTC_RD][PMAX], rm[CTC_RD][PMAX], ra[CTC_RD][PMAX];
    // The ring holds RAW scores and `- c` happens where they are used: a load with arithmetic behind it, or one under a
    // per-position predicate, makes the compiler wait for it on the spot (vmcnt(0) every step).  So every load of the sweeps is
    // unconditional -- a slot without a position reads column 0 of the row -- and nothing touches its value before its step.
    auto fetch = [&](int t, float (&s_)[PMAX], float (&m_)[PMAX], const int (&cmv)[PMAX]) {
        const float *row = srow + (size_t)(t < 0 ? 0 : (t >= T ? T - 1 : t)) * tstride;
#pragma unroll
        for (int k = 0; k < PMAX; ++k) {
            if (HB) s_[k] = row[cs[k]];
            m_[k] = row[cmv[k]];
        }
    };
#pragma unroll
    for (int d = 0; d < CTC_RD; ++d) fetch(d, rs[d], rm[d], cin);
    int cur = 0;
    for (int t0 = 0; t0 < T; t0 += CTC_RD) {
#pragma unroll
        for (int d = 0; d < CTC_RD; ++d) {
            const int t = t0 + d;
            if (t < T) {                                   // uniform
                const float *vc = vec + cur * vs;
                float *vn = vec + (cur ^ 1) * vs;
#pragma unroll
                for (int k = 0; k < PMAX; ++k) {
                    const int l = tid + k * BS;
                    if (l < n) {
                        const float x0 = vc[l + 1] + (HB ? rs[d][k] - c : stay_nb);
                        const float x1 = l > 0 ? vc[l] + (rm[d][k] - c) : CTC_ZERO;
                        const float v = ctc_sum2<false>(x0, x1);
                        vn[l + 1] = v;
                        stash[(size_t)(t + 1) * n + l] = v;
                    }
                }
                fetch(t + CTC_RD, rs[d], rm[d], cin);
                __syncthreads();
                cur ^= 1;
            }
        }
    }
    const float lz = vec[cur * vs + n];                    // alpha_T[len - sl]
    const float raw = -(lz / (float)len);
    float w = -(1.0f / (float)len);
    if (q.mean) w = w / (float)p.N;
    float loss = raw;
    if (q.loss_clip > 0.0f) {
        if (!(raw >= 0.0f && raw <= q.loss_clip)) w = 0.0f;
        loss = raw < 0.0f ? 0.0f : (raw > q.loss_clip ? q.loss_clip : raw);
    }
    if (tid == 0) {
        p.loss[b] = loss;
        q.w[b] = w;
    }
    __syncthreads();

    // ---- backward, CtcSweep::backward's: beta_t[l] = sum2(stay[t][l] + beta_{t+1}[l], move[t][l] + beta_{t+1}[l+1]), the
    //      restricted posteriors of step t into g, the heads' sums into the gradient
    for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTC_ZERO;
    __syncthreads();
    if (tid == 0) vec[n] = 0.0f;                           // beta_T: `one` at the last position
    __syncthreads();
    auto fetch_back = [&](int t, float (&s_)[PMAX], float (&m_)[PMAX], float (&a_)[PMAX]) {
        fetch(t, s_, m_, cout);
        const float *arow = stash + (size_t)(t < 0 ? 0 : t) * n;
#pragma unroll
        for (int k = 0; k < PMAX; ++k) a_[k] = arow[tid + k * BS < n ? tid + k * BS : 0];
    };
    // the heads' CRF posteriors, one step ahead
    const float *post = q.post + (size_t)b * q.ldq;
    const size_t pstride = (size_t)p.N * q.ldq;
    float ps[PMAX] = {}, pm[PMAX] = {};
    auto fetch_post = [&](int t) {
        const float *row = post + (size_t)(t < 0 ? 0 : t) * pstride;
#pragma unroll
        for (int k = 0; k < PMAX; ++k) {
            if (HB) ps[k] = row[cs[k]];
            pm[k] = row[cpm[k]];
        }
    };
    float *grow = q.grad + (size_t)b * p.ld;
    cur = 0;
#pragma unroll
    for (int d = 0; d < CTC_RD; ++d) fetch_back(T - 1 - d, rs[d], rm[d], ra[d]);
    fetch_post(T - 1);
    for (int t0 = T - 1; t0 >= 0; t0 -= CTC_RD) {
#pragma unroll
        for (int d = 0; d < CTC_RD; ++d) {
            const int t = t0 - d;
            if (t >= 0) {                                  // uniform
                const float *vc = vec + cur * vs;
                float *vn = vec + (cur ^ 1) * vs;
                float *gs = g + (size_t)(t & 1) * 2 * npmax, *gm = gs + npmax;
#pragma unroll
                for (int k = 0; k < PMAX; ++k) {
                    const int l = tid + k * BS;
                    if (l < n) {
                        const float a = ra[d][k], st = HB ? rs[d][k] - c : stay_nb, mv = rm[d][k] - c;
                        const float bn = vc[l + 1];
                        const float bx = l + 1 < n ? vc[l + 2] : CTC_ZERO;
                        if (HB) gs[l] = xb_expf(((a + st) + bn) - lz);
                        if (l + 1 < n) gm[l + 1] = xb_expf(((a + mv) + bx) - lz);
                        const float x0 = st + bn;
                        const float x1 = l + 1 < n ? mv + bx : CTC_ZERO;
                        vn[l + 1] = ctc_sum2<false>(x0, x1);
                    }
                }
                fetch_back(t - CTC_RD, rs[d], rm[d], ra[d]);
                __syncthreads();
                cur ^= 1;
                float *out = grow + (size_t)t * tstride;
                // the heads' own terms, read together; this step's posteriors step aside and the next step's loads go out
                // BEFORE the stores: a wait for a load is a wait for every older store too
                float hs[PMAX], hm[PMAX], pcs[PMAX], pcm[PMAX];
#pragma unroll
                for (int k = 0; k < PMAX; ++k) {
                    if (HB && (heads >> k & 1u)) hs[k] = gs[tid + k * BS];
                    if (heads >> (16 + k) & 1u) hm[k] = gm[tid + k * BS];
                    pcs[k] = ps[k];
                    pcm[k] = pm[k];
                }
                fetch_post(t - 1);
#pragma unroll
                for (int k = 0; k < PMAX; ++k) {
                    if (HB && (heads >> k & 1u)) {
                        float sum = 0.0f + hs[k];
                        for (int j = nxs[k]; j != CTCG_NONE; j = nxt[j]) sum += gs[j];
                        out[cs[k]] = (sum - pcs[k]) * w;
                    }
                    if (heads >> (16 + k) & 1u) {
                        float sum = 0.0f + hm[k];
                        for (int j = nxm[k]; j != CTCG_NONE; j = nxt[npmax + j]) sum += gm[j];
                        out[cin[k]] = (sum - pcm[k]) * w;
                    }
                }
            }
        }
    }
}

// Every column of a chunk's gradient that none of its positions maps to: (0.0f - P) * w; a refused chunk: zeros throughout.
// blockIdx.x = chunk, blockIdx.y = a slab of CTCG_FILL_STEPS time steps; the chunk's columns as a bit set in LDS.
constexpr int CTCG_FILL_THREADS = 256, CTCG_FILL_STEPS = 16;

template <bool HB>
__global__ __launch_bounds__(CTCG_FILL_THREADS) void ctc_grad_fill_kernel(xb::CtcGradParams q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctc_smem[];
    unsigned *hit = reinterpret_cast<unsigned *>(ctc_smem);
    const xb::CtcLossParams &p = q.l;
    const int tid = threadIdx.x, b = blockIdx.x, T = p.T, nb = p.nb, sl = p.sl, E = nb + 1;
    const int C = p.ld;
    const int t_lo = blockIdx.y * CTCG_FILL_STEPS, t_hi = min(T, t_lo + CTCG_FILL_STEPS);
    const size_t tstride = (size_t)p.N * p.ld;
    float *grow = q.grad + (size_t)b * p.ld;
    const int len = p.tlen[b];
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    if (ctc_bad_row(lab, len, p.Lt, nb, sl)) {
        for (int t = t_lo; t < t_hi; ++t)
            for (int cidx = tid; cidx < C; cidx += CTCG_FILL_THREADS) grow[(size_t)t * tstride + cidx] = 0.0f;
        return;
    }
    const int n = len + 1 - sl;
    for (int i = tid; i < (C + 31) / 32; i += CTCG_FILL_THREADS) hit[i] = 0u;
    __syncthreads();
    for (int l = tid; l < n; l += CTCG_FILL_THREADS) {
        int cs, cm, cp;
        xb::ctc_columns<HB>(lab, l, nb, sl, cs, cm, cp);
        if (HB) atomicOr(&hit[cs >> 5], 1u << (cs & 31));
        if (l > 0) atomicOr(&hit[cm >> 5], 1u << (cm & 31));
    }
    __syncthreads();
    const float w = q.w[b];
    const float *post = q.post + (size_t)b * q.ldq;
    const size_t pstride = (size_t)p.N * q.ldq;
    for (int cidx = tid; cidx < C; cidx += CTCG_FILL_THREADS) {
        if (hit[cidx >> 5] >> (cidx & 31) & 1u) continue;
        const int pc = HB ? cidx : (cidx / nb) * E + cidx % nb + 1;
        for (int t = t_lo; t < t_hi; ++t) grow[(size_t)t * tstride + cidx] = (0.0f - post[(size_t)t * pstride + pc]) * w;
    }
}

// ---- one launcher shape ------------------------------------------------------------------------------------------------------
// what the three lattice launchers check alike: the sizes, the pointers, and that every gather column lies inside a row
bool ctc_args_ok(const float *scores, int T, int N, int ld, int has_blank, int nb, int sl, const uint8_t *targets, int Lt,
                 const int32_t *tlen, const unsigned *error)
{
    const int np = Lt - (sl - 1);
    if (T < 1 || N < 1 || sl < 1 || nb < 1 || np < 1 || np > xb::ctc_max_positions() || !scores || !targets || !tlen || !error)
        return false;
    int64_t S = 1;
    for (int i = 0; i < sl; ++i) S *= nb;
    return ld >= S * (has_blank ? nb + 1 : nb);
}
bool ctc_args_ok(const xb::CtcLossParams &p)
{
    return ctc_args_ok(p.scores, p.T, p.N, p.ld, p.has_blank, p.nb, p.sl, p.targets, p.Lt, p.tlen, p.error) && p.logz_crf && p.loss;
}

// launch(P, L): the caller's kernel in its PMAX = P() instantiation under the launch L of a row of np positions
template <typename Launch>
hipError_t ctc_launch_lattice(int np, int threads, bool chains, Launch &&launch)
{
    const xb::CtcLaunch L = xb::ctc_launch(np, threads, chains);
    switch (L.pmax) {
    case 1: launch(std::integral_constant<int, 1>{}, L); break;
    case 2: launch(std::integral_constant<int, 2>{}, L); break;
    case 4: launch(std::integral_constant<int, 4>{}, L); break;
    case CTC_PMAX: launch(std::integral_constant<int, CTC_PMAX>{}, L); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

namespace xb {

hipError_t launch_ctc_scan(const CtcParams &p, hipStream_t stream)
{
    if (!ctc_args_ok(p.scores, p.T, p.N, p.C, 1, p.nb, p.sl, p.targets, p.Lt, p.tlen, p.error)) return hipErrorInvalidValue;
    if ((p.gstay || p.gmove) && !p.alpha) return hipErrorInvalidValue;
    return ctc_launch_lattice(p.Lt - (p.sl - 1), 0, false, [&](auto P, const CtcLaunch &L) {
        constexpr int PM = decltype(P)::value;
        const dim3 g(p.N), bdim(L.threads);
        if (p.semiring && p.alpha) hipLaunchKernelGGL((ctc_scan_kernel<PM, true, true>), g, bdim, L.lds, stream, p);
        else if (p.semiring) hipLaunchKernelGGL((ctc_scan_kernel<PM, true, false>), g, bdim, L.lds, stream, p);
        else if (p.alpha) hipLaunchKernelGGL((ctc_scan_kernel<PM, false, true>), g, bdim, L.lds, stream, p);
        else hipLaunchKernelGGL((ctc_scan_kernel<PM, false, false>), g, bdim, L.lds, stream, p);
    });
}

hipError_t launch_ctc_loss(const CtcLossParams &p, hipStream_t stream)
{
    if (!ctc_args_ok(p)) return hipErrorInvalidValue;
    return ctc_launch_lattice(p.Lt - (p.sl - 1), p.threads, false, [&](auto P, const CtcLaunch &L) {
        constexpr int PM = decltype(P)::value;
        const dim3 g(p.N), bdim(L.threads);
        if (p.has_blank) hipLaunchKernelGGL((ctc_loss_kernel<PM, true>), g, bdim, L.lds, stream, p);
        else hipLaunchKernelGGL((ctc_loss_kernel<PM, false>), g, bdim, L.lds, stream, p);
    });
}

static bool ctc_grad_args_ok(const CtcGradParams &q)
{
    const CtcLossParams &p = q.l;
    if (!ctc_args_ok(p) || !q.post || !q.w || !q.grad) return false;
    int64_t S = 1;
    for (int i = 0; i < p.sl; ++i) S *= p.nb;
    // dense rows: the gradient has the scores' layout, and the fill kernel walks every column of a row
    return p.ld == S * (p.has_blank ? p.nb + 1 : p.nb) && q.ldq >= S * (p.nb + 1);
}

hipError_t launch_ctc_grad(const CtcGradParams &q, hipStream_t stream)
{
    const CtcLossParams &p = q.l;
    const int np = p.Lt - (p.sl - 1);
    if (!ctc_grad_args_ok(q) || !q.stash || q.slot < ctc_grad_slot_floats(p.T, np) || q.first < 0 || q.count < 1 ||
        q.first + q.count > p.N)
        return hipErrorInvalidValue;
    return ctc_launch_lattice(np, p.threads, true, [&](auto P, const CtcLaunch &L) {
        constexpr int PM = decltype(P)::value;
        const dim3 g(q.count), bdim(L.threads);
        if (p.has_blank) hipLaunchKernelGGL((ctc_grad_kernel<PM, true>), g, bdim, L.lds, stream, q);
        else hipLaunchKernelGGL((ctc_grad_kernel<PM, false>), g, bdim, L.lds, stream, q);
    });
}

hipError_t launch_ctc_grad_fill(const CtcGradParams &q, hipStream_t stream)
{
    if (!ctc_grad_args_ok(q)) return hipErrorInvalidValue;
    const CtcLossParams &p = q.l;
    const dim3 g(p.N, (p.T + CTCG_FILL_STEPS - 1) / CTCG_FILL_STEPS), bdim(CTCG_FILL_THREADS);
    const size_t lds = sizeof(unsigned) * (size_t)((p.ld + 31) / 32);
    if (p.has_blank) hipLaunchKernelGGL(ctc_grad_fill_kernel<true>, g, bdim, lds, stream, q);
    else hipLaunchKernelGGL(ctc_grad_fill_kernel<false>, g, bdim, lds, stream, q);
    return hipGetLastError();
}

}  // namespace xb
