// xb_ctc.hip -- the CTC-CRF validation loss on the encoder's own scores (the contract is in the public header: xb_ctc_loss;
// xb_internal.h CtcLossParams).
//
// The forward Log-semiring scan of ctc_scan_kernel (xb_decode.hip) over the stay / move lattice of a label row, in a form
// that reads what the encoder wrote and nothing the host prepared:
//   - the gather columns of prepare_ctc_scores (ub-bonito/bonito/crf/model.py:102-116) come from the uint8 labels in the
//     kernel: position l is the k-mer state st_l = sum_i base[l + i] nb^(sl - 1 - i); with the blank column the stay edge reads
//     column st_l (nb + 1) and the move edge into l column st_l (nb + 1) + base[l - 1] + 1; without it the stay edge is the
//     constant blank score and the move edge into l reads column st_l nb + base[l - 1] (the decode's and the beam's mapping);
//   - every score is normalised as it is fetched, s - logz_crf / T: one correctly rounded division per chunk, one
//     subtraction per score, as Model.normalise does on the host.  Folding T * c into the result would save the subtractions
//     and round differently;
//   - only the positions of the chunk's own length are computed: a position feeds itself and its right neighbour alone, so the
//     ones beyond tlen - sl never reach the end cell.
// One workgroup per chunk, position l on thread l % threads (CTCL_PMAX positions per thread at most); the position vector is
// double buffered in LDS with one barrier per time step, the two scores of a position come through a CTCL_RD-deep register
// ring.  The arithmetic is ctc_scan_kernel's: sum2 = max, exp, exp, add, log, the stay term before the move term.  Built
// without contraction; bit-equal to oracle.ctc_logz on the normalised, blank-expanded scores.
#include "xb_internal.h"
#include "xb_math.h"

namespace {

constexpr int CTCL_MAX_THREADS = 256, CTCL_PMAX = 8, CTCL_RD = 4;
constexpr float CTCL_ZERO = -1e38f;              // seqdist's Log.zero

__device__ __forceinline__ float ctcl_sum2(float x0, float x1)
{
    const float m = x0 > x1 ? x0 : x1;
    return m + xb_logf(xb_expf(x0 - m) + xb_expf(x1 - m));
}

template <int PMAX, bool HB>
__global__ __launch_bounds__(CTCL_MAX_THREADS) void ctc_loss_kernel(xb::CtcLossParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcl_smem[];
    float *vec = reinterpret_cast<float *>(ctcl_smem);           // [2][n + 2]: slot l + 1 = position l, slots 0 and n + 1 = `zero`
    const int tid = threadIdx.x, BS = blockDim.x, b = blockIdx.x, T = p.T, nb = p.nb, sl = p.sl;
    const int len = p.tlen[b];
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    int bad = len < sl || len > p.Lt;                            // uniform
    if (!bad)
        for (int j = tid; j < len; j += BS) bad |= lab[j] > nb;
    if (__syncthreads_or(bad)) {
        if (tid == 0) atomicOr(p.error, 4u);
        return;
    }
    const int n = len + 1 - sl;                                  // this chunk's positions, 1 .. Lt - sl + 1 <= PMAX * BS
    const float c = p.logz_crf[b] / (float)T;
    const float stay_nb = p.blank - c;                           // the stay score of the blank-less layout
    const float *srow = p.scores + (size_t)b * p.ld;
    const size_t tstride = (size_t)p.N * p.ld;
    const int vs = n + 2, E = nb + 1;
    // this thread's positions and their gather columns: stay (own), move into the position (l - 1 -> l)
    int cs[PMAX], cm[PMAX];
#pragma unroll
    for (int k = 0; k < PMAX; ++k) {
        const int l = tid + k * BS;
        cs[k] = cm[k] = 0;
        if (l < n) {
            int st = 0;
            for (int i = 0; i < sl; ++i) st = st * nb + max((int)lab[l + i] - 1, 0);         // torch.clamp(targets - 1, 0)
            const int base = l > 0 ? max((int)lab[l - 1] - 1, 0) : 0;
            cs[k] = HB ? st * E : 0;
            cm[k] = l > 0 ? (HB ? st * E + base + 1 : st * nb + base) : 0;
        }
    }
    for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTCL_ZERO;
    __syncthreads();
    if (tid == 0) vec[1] = 0.0f;                                 // alpha_0: `one` at position 0
    __syncthreads();

    // ---- alpha_{t+1}[l] = sum2(alpha_t[l] + stay[t][l], alpha_t[l-1] + move[t][l-1])
    float rs[CTCL_RD][PMAX], rm[CTCL_RD][PMAX];
    auto fetch = [&](int t, float (&s_)[PMAX], float (&m_)[PMAX]) {
        const float *row = srow + (size_t)(t >= T ? T - 1 : t) * tstride;
#pragma unroll
        for (int k = 0; k < PMAX; ++k)
            if (tid + k * BS < n) {
                s_[k] = HB ? row[cs[k]] - c : stay_nb;
                m_[k] = row[cm[k]] - c;
            }
    };
#pragma unroll
    for (int d = 0; d < CTCL_RD; ++d) fetch(d, rs[d], rm[d]);
    int cur = 0;
    for (int t0 = 0; t0 < T; t0 += CTCL_RD) {
#pragma unroll
        for (int d = 0; d < CTCL_RD; ++d) {
            const int t = t0 + d;
            if (t < T) {                                   // uniform
                const float *vc = vec + cur * vs;
                float *vn = vec + (cur ^ 1) * vs;
#pragma unroll
                for (int k = 0; k < PMAX; ++k) {
                    const int l = tid + k * BS;
                    if (l < n) {
                        const float x0 = vc[l + 1] + rs[d][k];
                        const float x1 = l > 0 ? vc[l] + rm[d][k] : CTCL_ZERO;
                        vn[l + 1] = ctcl_sum2(x0, x1);
                    }
                }
                fetch(t + CTCL_RD, rs[d], rm[d]);
                __syncthreads();
                cur ^= 1;
            }
        }
    }
    if (tid == 0) {
        const float lz = vec[cur * vs + n];                // alpha_T[len - sl]
        if (p.logz) p.logz[b] = lz;
        p.loss[b] = -(lz / (float)len);
    }
}

// ---- the loss with its gradient (xb_ctc_loss_grad; xb_internal.h CtcGradParams) -------------------------------------------
// ctc_grad_kernel: ctc_loss_kernel's forward sweep with alpha stashed, then ctc_scan_kernel's backward sweep with the
// restricted posteriors scattered over their score columns.  Positions that share a column (a repeated k-mer: a homopolymer
// run, a recurring k-mer) are linked once per chunk into chains of ascending position; per time step the posteriors go to
// LDS and the chain's first position adds its chain serially from 0.0f -- the order np.add.at gives, the same on every run,
// no floating-point atomic anywhere.  It writes (sum - P) * w for the columns the chunk's positions map to;
// ctc_grad_fill_kernel writes (0.0f - P) * w into all the others, at memory speed and off the lattice's latency chain.
// LDS: vec [2][np + 2] | g [2][2][np] (during the chain build: the positions' columns) | next [2][np] u16 | not-head [2][np] u8.
constexpr int CTCG_NONE = 0xffff;

// the columns of position l of a label row: stay (own), move into it (l - 1 -> l); cp = the move column in the posteriors'
// (blank) layout
template <bool HB>
__device__ __forceinline__ void ctcg_columns(const uint8_t *lab, int l, int nb, int sl, int &cs, int &cm, int &cp)
{
    const int E = nb + 1;
    int st = 0;
    for (int i = 0; i < sl; ++i) st = st * nb + max((int)lab[l + i] - 1, 0);         // torch.clamp(targets - 1, 0)
    const int base = l > 0 ? max((int)lab[l - 1] - 1, 0) : 0;
    cs = st * E;                                                  // HB only: the blank-less layout has no stay column
    cp = l > 0 ? st * E + base + 1 : 0;
    cm = l > 0 ? (HB ? cp : st * nb + base) : 0;
}

// uniform: a length outside [sl, Lt] or a label above nb inside it
__device__ __forceinline__ int ctcg_bad_row(const uint8_t *lab, int len, int Lt, int nb, int sl)
{
    int bad = len < sl || len > Lt;
    if (!bad)
        for (int j = threadIdx.x; j < len; j += blockDim.x) bad |= lab[j] > nb;
    return __syncthreads_or(bad);
}

template <int PMAX, bool HB>
__global__ __launch_bounds__(CTCL_MAX_THREADS) void ctc_grad_kernel(xb::CtcGradParams q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcl_smem[];
    const xb::CtcLossParams &p = q.l;
    const int tid = threadIdx.x, BS = blockDim.x, b = q.first + blockIdx.x, T = p.T, nb = p.nb, sl = p.sl;
    const int npmax = p.Lt - (sl - 1);
    float *vec = reinterpret_cast<float *>(ctcl_smem);           // [2][npmax + 2]
    float *g = vec + 2 * (npmax + 2);                            // [buffer][stay, move][npmax]
    int *col = reinterpret_cast<int *>(g);                       // [stay, move][npmax], until the chains stand
    unsigned short *nxt = reinterpret_cast<unsigned short *>(g + 4 * npmax);      // [stay, move][npmax]
    unsigned char *nothead = reinterpret_cast<unsigned char *>(nxt + 2 * npmax);  // [stay, move][npmax]
    const int len = p.tlen[b];
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    if (ctcg_bad_row(lab, len, p.Lt, nb, sl)) {                  // the fill kernel zeroes this chunk's gradient
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
            ctcg_columns<HB>(lab, l, nb, sl, cs[k], cin[k], cpm[k]);
            if (l + 1 < n) {
                int s1, p1;
                ctcg_columns<HB>(lab, l + 1, nb, sl, s1, cout[k], p1);
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
    for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTCL_ZERO;
    __syncthreads();
    if (tid == 0) vec[1] = 0.0f;                                 // alpha_0: `one` at position 0
#pragma unroll
    for (int k = 0; k < PMAX; ++k) {
        const int l = tid + k * BS;
        if (l < n) stash[l] = l == 0 ? 0.0f : CTCL_ZERO;
    }
    __syncthreads();

    // ---- forward, ctc_loss_kernel's: alpha_{t+1}[l] = sum2(alpha_t[l] + stay[t][l], alpha_t[l-1] + move[t][l-1])
    float rs[CTCL_RD][PMAX], rm[CTCL_RD][PMAX], ra[CTCL_RD][PMAX];
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
    for (int d = 0; d < CTCL_RD; ++d) fetch(d, rs[d], rm[d], cin);
    int cur = 0;
    for (int t0 = 0; t0 < T; t0 += CTCL_RD) {
#pragma unroll
        for (int d = 0; d < CTCL_RD; ++d) {
            const int t = t0 + d;
            if (t < T) {                                   // uniform
                const float *vc = vec + cur * vs;
                float *vn = vec + (cur ^ 1) * vs;
#pragma unroll
                for (int k = 0; k < PMAX; ++k) {
                    const int l = tid + k * BS;
                    if (l < n) {
                        const float x0 = vc[l + 1] + (HB ? rs[d][k] - c : stay_nb);
                        const float x1 = l > 0 ? vc[l] + (rm[d][k] - c) : CTCL_ZERO;
                        const float v = ctcl_sum2(x0, x1);
                        vn[l + 1] = v;
                        stash[(size_t)(t + 1) * n + l] = v;
                    }
                }
                fetch(t + CTCL_RD, rs[d], rm[d], cin);
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

    // ---- backward, ctc_scan_kernel's: beta_t[l] = sum2(stay[t][l] + beta_{t+1}[l], move[t][l] + beta_{t+1}[l+1]), the
    //      restricted posteriors of step t into g, the heads' sums into the gradient
    for (int i = tid; i < 2 * vs; i += BS) vec[i] = CTCL_ZERO;
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
    for (int d = 0; d < CTCL_RD; ++d) fetch_back(T - 1 - d, rs[d], rm[d], ra[d]);
    fetch_post(T - 1);
    for (int t0 = T - 1; t0 >= 0; t0 -= CTCL_RD) {
#pragma unroll
        for (int d = 0; d < CTCL_RD; ++d) {
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
                        const float bx = l + 1 < n ? vc[l + 2] : CTCL_ZERO;
                        if (HB) gs[l] = xb_expf(((a + st) + bn) - lz);
                        if (l + 1 < n) gm[l + 1] = xb_expf(((a + mv) + bx) - lz);
                        const float x0 = st + bn;
                        const float x1 = l + 1 < n ? mv + bx : CTCL_ZERO;
                        vn[l + 1] = ctcl_sum2(x0, x1);
                    }
                }
                fetch_back(t - CTCL_RD, rs[d], rm[d], ra[d]);
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
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcl_smem[];
    unsigned *hit = reinterpret_cast<unsigned *>(ctcl_smem);
    const xb::CtcLossParams &p = q.l;
    const int tid = threadIdx.x, b = blockIdx.x, T = p.T, nb = p.nb, sl = p.sl, E = nb + 1;
    const int C = p.ld;
    const int t_lo = blockIdx.y * CTCG_FILL_STEPS, t_hi = min(T, t_lo + CTCG_FILL_STEPS);
    const size_t tstride = (size_t)p.N * p.ld;
    float *grow = q.grad + (size_t)b * p.ld;
    const int len = p.tlen[b];
    const uint8_t *lab = p.targets + (size_t)b * p.Lt;
    if (ctcg_bad_row(lab, len, p.Lt, nb, sl)) {
        for (int t = t_lo; t < t_hi; ++t)
            for (int cidx = tid; cidx < C; cidx += CTCG_FILL_THREADS) grow[(size_t)t * tstride + cidx] = 0.0f;
        return;
    }
    const int n = len + 1 - sl;
    for (int i = tid; i < (C + 31) / 32; i += CTCG_FILL_THREADS) hit[i] = 0u;
    __syncthreads();
    for (int l = tid; l < n; l += CTCG_FILL_THREADS) {
        int cs, cm, cp;
        ctcg_columns<HB>(lab, l, nb, sl, cs, cm, cp);
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

template <bool HB>
void launch_grad_hb(const xb::CtcGradParams &q, int threads, int per, size_t lds, hipStream_t stream)
{
    const dim3 g(q.count), bdim(threads);
    if (per <= 1) hipLaunchKernelGGL((ctc_grad_kernel<1, HB>), g, bdim, lds, stream, q);
    else if (per <= 2) hipLaunchKernelGGL((ctc_grad_kernel<2, HB>), g, bdim, lds, stream, q);
    else if (per <= 4) hipLaunchKernelGGL((ctc_grad_kernel<4, HB>), g, bdim, lds, stream, q);
    else hipLaunchKernelGGL((ctc_grad_kernel<CTCL_PMAX, HB>), g, bdim, lds, stream, q);
}

template <bool HB>
void launch_hb(const xb::CtcLossParams &p, int threads, int per, size_t lds, hipStream_t stream)
{
    const dim3 g(p.N), bdim(threads);
    if (per <= 1) hipLaunchKernelGGL((ctc_loss_kernel<1, HB>), g, bdim, lds, stream, p);
    else if (per <= 2) hipLaunchKernelGGL((ctc_loss_kernel<2, HB>), g, bdim, lds, stream, p);
    else if (per <= 4) hipLaunchKernelGGL((ctc_loss_kernel<4, HB>), g, bdim, lds, stream, p);
    else hipLaunchKernelGGL((ctc_loss_kernel<CTCL_PMAX, HB>), g, bdim, lds, stream, p);
}

}  // namespace

namespace xb {

// One wave while the positions fit it one per lane (the barrier then costs nothing), else as many waves as give every lane
// a position, four at most: a time step is a chain of dependent instructions, and its length grows with the positions per lane.
int ctc_loss_threads(int positions) { return positions <= 64 ? 64 : (positions <= 128 ? 128 : CTCL_MAX_THREADS); }

hipError_t launch_ctc_loss(const CtcLossParams &p, hipStream_t stream)
{
    const int np = p.Lt - (p.sl - 1);
    if (p.T < 1 || p.N < 1 || p.sl < 1 || p.nb < 1 || np < 1 || np > ctc_max_positions() || !p.scores || !p.targets || !p.tlen ||
        !p.logz_crf || !p.loss || !p.error)
        return hipErrorInvalidValue;
    int64_t S = 1;
    for (int i = 0; i < p.sl; ++i) S *= p.nb;
    if (p.ld < S * (p.has_blank ? p.nb + 1 : p.nb)) return hipErrorInvalidValue;      // every gather column lies inside a row
    int threads = ctc_loss_threads(np);
    if ((p.threads == 64 || p.threads == 128 || p.threads == 256) && p.threads * CTCL_PMAX >= np) threads = p.threads;
    const int per = (np + threads - 1) / threads;
    if (per > CTCL_PMAX) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * 2 * (size_t)(np + 2);
    if (p.has_blank) launch_hb<true>(p, threads, per, lds, stream);
    else launch_hb<false>(p, threads, per, lds, stream);
    return hipGetLastError();
}

static bool ctc_grad_args_ok(const CtcGradParams &q)
{
    const CtcLossParams &p = q.l;
    const int np = p.Lt - (p.sl - 1);
    if (p.T < 1 || p.N < 1 || p.sl < 1 || p.nb < 1 || np < 1 || np > ctc_max_positions() || !p.scores || !p.targets || !p.tlen ||
        !p.logz_crf || !p.loss || !p.error || !q.post || !q.w || !q.grad)
        return false;
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
    int threads = ctc_loss_threads(np);
    if ((p.threads == 64 || p.threads == 128 || p.threads == 256) && p.threads * CTCL_PMAX >= np) threads = p.threads;
    const int per = (np + threads - 1) / threads;
    if (per > CTCL_PMAX) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * (2 * (size_t)(np + 2) + 4 * (size_t)np) + 4 * (size_t)np + 2 * (size_t)np;
    if (p.has_blank) launch_grad_hb<true>(q, threads, per, lds, stream);
    else launch_grad_hb<false>(q, threads, per, lds, stream);
    return hipGetLastError();
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
