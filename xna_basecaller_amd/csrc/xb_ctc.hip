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

}  // namespace xb
