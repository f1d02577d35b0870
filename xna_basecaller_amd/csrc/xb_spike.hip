// xb_spike.hip -- xb_spike_chunks and xb_synth_chunks: the reference's synthetic XNA spiking and its fully synthetic chunks
// (ub-bonito/bonito/spike_chunks.py; contract: the public header).  Built with -ffp-contract=off: every float64 operation is
// the contract's, in its order, bit-equal to the CPU restatements (tests/spike_ref.py, tests/synth_ref.py).
//
// spike_kernel
// One wave per chunk, one launch per call.  The wave copies its signal and label rows, then:
//   k-mers      the chunk's own k-mers (one per base, over the labels and their ATATA / TATAT tail) are looked up first: a
//               missing one ends the chunk with status 2 before anything is drawn.
//   positions   the chooser shared with xb_splice.hip (xb_positions.h), on stream 0; the X / Y list is a bit per entry in
//               LDS, shuffled by lane 0 on the same stream.  The six k-mers of every window are looked up before any paste.
//   med, mad    exact order statistics of the 100 * length squiggle values WITHOUT storing them: a value is a pure function
//               of (chunk, sample index), so every pass of a radix selection over order-preserving 64-bit keys regenerates
//               them -- a lane takes a base and walks its 100 samples, the model row loaded once.  A pass counts one 4-bit
//               digit in 16 registers per lane (no atomics, no LDS, nothing to overflow: int32), a wave sum per digit picks
//               the bucket of the rank: 16 passes find the lower middle value and how many equal it; the upper middle one is
//               the same value (ties) or the smallest key above it (one more pass).  34 passes for med and mad.
//   pastes      a lane per window sample: its k-mer from the window's cumulative repetitions, the level noise (uniform, or
//               the truncated normal through PPND16), the added noise, ((mean + level + noise) - med) / mad rounded once.
// Control flow is wave-uniform but for the per-sample branches of PPND16; positions are separated by a barrier, so a later
// paste may overlap an earlier one (pad < 5) and wins, as in the reference's sequential loop.
//
// The kernel reads lengths, labels and breakpoints it did not validate (the _dev form): lengths are clamped to the row,
// labels to 6, breakpoints to the chunk and to non-decreasing order, so that no access leaves the rows whatever they hold.
//
// synth_kernel
// The same wave per chunk, the same positions, shuffle, selection and draws; what differs is what they are applied to:
//   labels      the unnatural bases are written into the output row FIRST, and every k-mer after that -- the check, the
//               squiggle of med / mad, the synthesis -- is read from that row (a barrier between).  A missing k-mer puts the
//               input's letters back.  The k-mers of the input row are never looked up.
//   samples     lanes stride over the chunk's samples 0 .. total - 1 (total = the last breakpoint); a sample finds its base by
//               an upper-bound search over the clamped breakpoints, which skips bases without a sample by itself.  One shift
//               row and one noise std serve the whole chunk (stream 2), the draw index is the sample index.  Samples past
//               total keep the input's value.
// A breakpoint row that is not non-decreasing (the _dev form only) makes the search end at some base of the row: the values
// are unspecified, every access stays inside the rows.
#include <hip/hip_runtime.h>

#include "xb_internal.h"
#include "xb_positions.h"

namespace {

using xb::SpikeParams;
using namespace xb_pos;

constexpr int KM = 6;
constexpr int REPS = xb::SPIKE_KMER_REPS;
constexpr int MASK_WORDS = (xb::SPLICE_MAX_LABELS + 32) / 32;
constexpr u64 SIGN = 0x8000000000000000ULL;

// ---- the library's own logarithm: IEEE + - * / and bit operations only, in this order (x positive, finite, normal)
__device__ inline double xb_log(double x)
{
    const u64 bits = (u64)__double_as_longlong(x);
    int e = (int)(bits >> 52) - 1023;
    double m = __longlong_as_double((long long)((bits & 0x000FFFFFFFFFFFFFULL) | 0x3FF0000000000000ULL));   // [1, 2)
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e = e + 1;
    }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double q = 1.0 / 21.0;
    q = q * z + 1.0 / 19.0;
    q = q * z + 1.0 / 17.0;
    q = q * z + 1.0 / 15.0;
    q = q * z + 1.0 / 13.0;
    q = q * z + 1.0 / 11.0;
    q = q * z + 1.0 / 9.0;
    q = q * z + 1.0 / 7.0;
    q = q * z + 1.0 / 5.0;
    q = q * z + 1.0 / 3.0;
    const double t = (s * z) * q;
    const double logm = 2.0 * (s + t);
    const double de = (double)e;
    return de * 6.93147180369123816490e-01 + (logm + de * 1.90821492927058770002e-10);
}

// ---- Wichura's AS241 PPND16, the algorithm and coefficients of CPython's statistics._normal_dist_inv_cdf (0 < p < 1)
__device__ inline double ppnd16(double p)
{
    const double q = p - 0.5;
    double num, den;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                  4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                  2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-xb_log(r));
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                  1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                  1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                  2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                  7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                5.99832206555888793690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// an order-preserving key of a finite float64 (-0 counts as +0) and its inverse
__device__ inline u64 order_key(double x)
{
    const u64 b = (u64)__double_as_longlong(x + 0.0);
    return (b & SIGN) ? ~b : (b | SIGN);
}
__device__ inline double key_value(u64 k) { return __longlong_as_double((long long)((k & SIGN) ? (k & ~SIGN) : ~k)); }

__device__ inline u64 wave_min64(u64 v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

// the labels of one chunk with their tail: letter i of target[:length] + ATATA (TATAT when the last letter is A)
struct Letters {
    const unsigned char *tgt;
    int length, tail0;
    __device__ int operator()(int i) const
    {
        if (i < length) {
            const int v = tgt[i];
            return v > 6 ? 6 : v;
        }
        return ((i - length) & 1) ? 5 - tail0 : tail0;
    }
    __device__ int kmer(int i) const         // the k-mer that starts at base i, as a table index
    {
        int t = 0;
#pragma unroll
        for (int q = 0; q < KM; ++q) t = t * 7 + (*this)(i + q);
        return t;
    }
};

// the squiggle of one chunk: f(x) for every value x of the lane's bases
struct Squiggle {
    Letters letters;
    const double *model;
    u64 base;                                // of stream 1
    int lane;
    template <class F> __device__ void each(F f) const
    {
        for (int i = lane; i < letters.length; i += 64) {
            const int t = letters.kmer(i);
            const double mean = model[2 * t], s = model[2 * t + 1];
            const double lo = -s, w = s - lo;
            const u64 k0 = (u64)i * REPS;
            for (int r = 0; r < REPS; ++r) f(mean + (lo + w * unit(mix(base + GAMMA * (k0 + (u64)r + 1)))));
        }
    }
};

// the median of the squiggle (dev false) or of |x - med| (dev true): the two middle order statistics of an even count
__device__ double median(const Squiggle &sq, bool dev, double med)
{
    long long rank = (long long)sq.letters.length * REPS / 2 - 1;
    u64 prefix = 0, himask = 0;
    int eq = 0;
    for (int shift = 60; shift >= 0; shift -= 4) {
        int cnt[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) cnt[t] = 0;
        sq.each([&](double x) {
            if (dev) x = fabs(x - med);
            const u64 key = order_key(x);
            const int d = (key & himask) == prefix ? (int)((key >> shift) & 15) : -1;
#pragma unroll
            for (int t = 0; t < 16; ++t) cnt[t] += d == t;
        });
        int digit = 15;
        bool placed = false;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int total = wave_sum(cnt[t]);
            if (!placed) {
                if (rank < total) {
                    digit = t;
                    eq = total;
                    placed = true;
                } else {
                    rank -= total;
                }
            }
        }
        prefix |= (u64)digit << shift;
        himask |= (u64)15 << shift;
    }
    const double a = key_value(prefix);
    double b = a;
    if (rank + 1 >= eq) {                    // the next order statistic is the smallest key above
        u64 least = ~(u64)0;
        sq.each([&](double x) {
            if (dev) x = fabs(x - med);
            const u64 key = order_key(x);
            if (key > prefix && key < least) least = key;
        });
        b = key_value(wave_min64(least));
    }
    return (a + b) / 2.0;
}

// the X / Y list of n_pos > 0 positions (ubs_mask 3): X, Y, X, Y, .. of n_pos + n_pos % 2 entries, a bit per entry in LDS (set:
// Y), shuffled from its end by lane 0 with the chunk's next sequential draws.  Ends with a barrier.
template <class Next> __device__ inline void shuffle_ubs(unsigned *yset, int n_pos, Next &next, int lane)
{
    const int m = n_pos + (n_pos & 1);
    for (int w = lane; w <= (m - 1) >> 5; w += 64) yset[w] = 0xAAAAAAAAu;
    __syncthreads();
    if (lane == 0) {
        for (int i = m - 1; i >= 1; --i) {
            const int j = (int)bounded(next(), (unsigned)i + 1u);
            const unsigned bi = yset[i >> 5] >> (i & 31) & 1u, bj = yset[j >> 5] >> (j & 31) & 1u;
            if (bi != bj) {
                yset[i >> 5] ^= 1u << (i & 31);
                yset[j >> 5] ^= 1u << (j & 31);
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void spike_kernel(const SpikeParams p)
{
    __shared__ unsigned valid[MASK_WORDS], chosen[MASK_WORDS], yset[MASK_WORDS];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;
    const int N = p.N, Lt = p.Lt;
    const float *sig = p.signal + (size_t)c * N;
    float *out = p.out_signal + (size_t)c * N;
    const unsigned char *tgt = p.targets + (size_t)c * Lt;
    unsigned char *out_t = p.out_targets + (size_t)c * Lt;
    const uint16_t *bk = p.bkps + (size_t)c * Lt;

    copy_row(out, sig, N, p.signal, p.out_signal, lane);
    copy_row(out_t, tgt, Lt, p.targets, p.out_targets, lane);

    int length = p.lengths[c];
    length = length < 0 ? 0 : (length > Lt ? Lt : length);
    const int W = (length + 31) >> 5;
    auto finish = [&](int spiked, double med, double mad, int status) {
        if (lane == 0) {
            p.spiked[c] = spiked;
            p.med[c] = med;
            p.mad[c] = mad;
            p.status[c] = (int8_t)status;
        }
    };
    if (length == 0) {
        finish(0, 0.0, 0.0, 0);
        return;
    }
    const Letters letters{tgt, length, tgt[length - 1] == 1 ? 4 : 1};
    const double quiet_nan = __longlong_as_double(0x7FF8000000000000LL);

    // ---- the chunk's own k-mers: the first missing one ends it
    int missing = 0x7fffffff;
    for (int i = lane; i < length; i += 64) {
        const double mean = p.model[2 * letters.kmer(i)];
        if (mean != mean && i < missing) missing = i;
    }
    missing = wave_min(missing);
    if (missing != 0x7fffffff) {
        finish(0, (double)letters.kmer(missing), quiet_nan, 2);
        return;
    }

    // ---- stream 0: proportion, positions, the shuffle of the X / Y list
    const u64 chunk_base = mix(p.seed + GAMMA * (p.first_index + (u64)c + 1));
    const u64 base0 = mix(chunk_base + GAMMA * 1);
    u64 kdraw = 0;
    auto next = [&]() { return mix(base0 + GAMMA * ++kdraw); };
    const int n_pos = choose_positions(valid, chosen, tgt, length, p.pad, p.prop, p.var_prop, next, lane);
    if (p.ubs_mask == 3 && n_pos > 0) shuffle_ubs(yset, n_pos, next, lane);
    // the unnatural base of the ordinal-th position: 0 = none (ubs_mask 0: the DNA k-mers are re-synthesised)
    auto ub_of = [&](int ordinal) {
        if (p.ubs_mask == 3) return 5 + (int)(yset[ordinal >> 5] >> (ordinal & 31) & 1u);
        return p.ubs_mask == 0 ? 0 : 4 + p.ubs_mask;
    };
    // the six k-mers of the window at pos: letters i .. i + 5 of target[pos - 5 .. pos + 5], the middle one replaced
    auto window_kmers = [&](int pos, int ub, int idx[KM]) {
        int st[2 * KM - 1];
#pragma unroll
        for (int j = 0; j < 2 * KM - 1; ++j) st[j] = letters(pos - KM + 1 + j);
        if (ub) st[KM - 1] = ub;
#pragma unroll
        for (int i = 0; i < KM; ++i) {
            int t = 0;
#pragma unroll
            for (int q = 0; q < KM; ++q) t = t * 7 + st[i + q];
            idx[i] = t;
        }
    };

    // ---- every window's k-mers before any paste: the first missing one ends the chunk
    for (int w = 0, ordinal = 0; w < W; ++w) {
        unsigned cw = (unsigned)__builtin_amdgcn_readfirstlane((int)chosen[w]);
        while (cw) {
            const int pos = (w << 5) + __ffs((int)cw) - 1;
            cw &= cw - 1;
            int idx[KM];
            window_kmers(pos, ub_of(ordinal++), idx);
#pragma unroll
            for (int i = 0; i < KM; ++i) {
                const double mean = p.model[2 * idx[i]];
                if (mean != mean) {
                    finish(0, (double)idx[i], quiet_nan, 2);
                    return;
                }
            }
        }
    }

    // ---- med, mad of the squiggle (stream 1)
    const Squiggle sq{letters, p.model, mix(chunk_base + GAMMA * 2), lane};
    const double med = median(sq, false, 0.0);
    const double mad = median(sq, true, med) * 1.4826 + 0x1p-23;

    // ---- per position, ascending (stream 2 + ordinal)
    const int rows = p.dist_rows;
    const double noise_pa = p.phi[rows][0], noise_pw = p.phi[rows][1];
    int ordinal = 0;
    for (int w = 0; w < W; ++w) {
        unsigned cw = (unsigned)__builtin_amdgcn_readfirstlane((int)chosen[w]);
        while (cw) {
            const int pos = (w << 5) + __ffs((int)cw) - 1;
            cw &= cw - 1;
            const int ub = ub_of(ordinal);
            const u64 base = mix(chunk_base + GAMMA * ((u64)ordinal + 3));
            ++ordinal;
            auto draw = [&](u64 k) { return mix(base + GAMMA * (k + 1)); };
            int idx[KM], cum[KM + 1];
            window_kmers(pos, ub, idx);
            double mean[KM], stdv[KM];
#pragma unroll
            for (int i = 0; i < KM; ++i) {
                mean[i] = p.model[2 * idx[i]];
                stdv[i] = p.model[2 * idx[i] + 1];
            }
            int first = 0;
#pragma unroll
            for (int j = 0; j <= KM; ++j) {
                int v = bk[pos - KM + j];
                v = v > N ? N : v;
                if (j > 0) v = v < cum[j - 1] + first ? cum[j - 1] + first : v;
                if (j == 0) first = v;
                cum[j] = v - first;
            }
            const int len = cum[KM];
            double level_pa = 0.0, level_pw = 0.0;
            if (rows > 0) {
                const int r = (int)bounded(draw(0), (unsigned)rows);
                level_pa = p.phi[r][0];
                level_pw = p.phi[r][1];
            }
            double sigma = p.noise_std;
            if (p.noise_std > 0.0 && p.variable_noise) sigma = 0.0 + (p.noise_std - 0.0) * unit(draw(1));
            float *dst = out + first;
            for (int i = lane; i < len; i += 64) {
                double m = mean[0], s = stdv[0];
#pragma unroll
                for (int q = 1; q < KM; ++q) {
                    m = i >= cum[q] ? mean[q] : m;
                    s = i >= cum[q] ? stdv[q] : s;
                }
                const double u = unit(draw(2 + (u64)i));
                double level;
                if (rows == 0) {
                    const double lo = -s;
                    level = lo + (s - lo) * u;
                } else {
                    level = ppnd16(level_pa + u * level_pw) * s;
                }
                double v = m + level;
                if (p.noise_std > 0.0) v = v + ppnd16(noise_pa + unit(draw(2 + (u64)len + (u64)i)) * noise_pw) * sigma;
                dst[i] = (float)((v - med) / mad);
            }
            if (ub && lane == 0) out_t[pos] = (unsigned char)ub;
            __syncthreads();                                        // the paste is in place before the next one
        }
    }
    finish(ordinal, med, mad, 0);
}

__global__ __launch_bounds__(64) void synth_kernel(const SpikeParams p)
{
    __shared__ unsigned valid[MASK_WORDS], chosen[MASK_WORDS], yset[MASK_WORDS];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;
    const int N = p.N, Lt = p.Lt;
    const float *sig = p.signal + (size_t)c * N;
    float *out = p.out_signal + (size_t)c * N;
    const unsigned char *tgt = p.targets + (size_t)c * Lt;
    unsigned char *out_t = p.out_targets + (size_t)c * Lt;
    const uint16_t *bk = p.bkps + (size_t)c * Lt;

    copy_row(out, sig, N, p.signal, p.out_signal, lane);
    copy_row(out_t, tgt, Lt, p.targets, p.out_targets, lane);

    int length = p.lengths[c];
    length = length < 0 ? 0 : (length > Lt ? Lt : length);
    const int W = (length + 31) >> 5;
    auto finish = [&](int spiked, double med, double mad, int status) {
        if (lane == 0) {
            p.spiked[c] = spiked;
            p.med[c] = med;
            p.mad[c] = mad;
            p.status[c] = (int8_t)status;
        }
    };
    if (length == 0) {
        finish(0, 0.0, 0.0, 0);
        return;
    }

    // ---- stream 0: proportion, positions, the shuffle of the X / Y list (as spike_kernel)
    const u64 chunk_base = mix(p.seed + GAMMA * (p.first_index + (u64)c + 1));
    const u64 base0 = mix(chunk_base + GAMMA * 1);
    u64 kdraw = 0;
    auto next = [&]() { return mix(base0 + GAMMA * ++kdraw); };
    const int n_pos = choose_positions(valid, chosen, tgt, length, p.pad, p.prop, p.var_prop, next, lane);
    if (p.ubs_mask == 3 && n_pos > 0) shuffle_ubs(yset, n_pos, next, lane);

    // ---- the spiked row: the copy is in place (barrier), then the unnatural bases, then every reader (barrier)
    __syncthreads();
    if (p.ubs_mask != 0 && lane == 0) {
        for (int w = 0, ordinal = 0; w < W; ++w) {
            unsigned cw = chosen[w];
            while (cw) {
                const int pos = (w << 5) + __ffs((int)cw) - 1;
                cw &= cw - 1;
                out_t[pos] = (unsigned char)(p.ubs_mask == 3 ? 5 + (int)(yset[ordinal >> 5] >> (ordinal & 31) & 1u) : 4 + p.ubs_mask);
                ++ordinal;
            }
        }
    }
    __syncthreads();
    const Letters letters{out_t, length, out_t[length - 1] == 1 ? 4 : 1};
    const double quiet_nan = __longlong_as_double(0x7FF8000000000000LL);

    // ---- the spiked row's k-mers: the first missing one, in base order, ends the chunk with the input's letters back
    int missing = 0x7fffffff;
    for (int i = lane; i < length; i += 64) {
        const double mean = p.model[2 * letters.kmer(i)];
        if (mean != mean && i < missing) missing = i;
    }
    missing = wave_min(missing);
    if (missing != 0x7fffffff) {
        const int t = letters.kmer(missing);
        __syncthreads();                                                // every lane has read the row it is about to lose
        for (int i = lane; i < length; i += 64)
            if (chosen[i >> 5] >> (i & 31) & 1u) out_t[i] = tgt[i];
        finish(0, (double)t, quiet_nan, 2);
        return;
    }

    // ---- med, mad of the spiked row's squiggle (stream 1)
    const Squiggle sq{letters, p.model, mix(chunk_base + GAMMA * 2), lane};
    const double med = median(sq, false, 0.0);
    const double mad = median(sq, true, med) * 1.4826 + 0x1p-23;

    // ---- the chunk's samples (stream 2): one shift row, one noise std
    int total = bk[length - 1];
    total = total > N ? N : total;
    const u64 base = mix(chunk_base + GAMMA * 3);
    auto draw = [&](u64 k) { return mix(base + GAMMA * (k + 1)); };
    const int rows = p.dist_rows;
    const double noise_pa = p.phi[rows][0], noise_pw = p.phi[rows][1];
    double level_pa = 0.0, level_pw = 0.0;
    if (rows > 0) {
        const int r = (int)bounded(draw(0), (unsigned)rows);
        level_pa = p.phi[r][0];
        level_pw = p.phi[r][1];
    }
    double sigma = p.noise_std;
    if (p.noise_std > 0.0 && p.variable_noise) sigma = 0.0 + (p.noise_std - 0.0) * unit(draw(1));
    for (int i = lane; i < total; i += 64) {
        int lo_b = 0, hi_b = length - 1;                                // the first base whose breakpoint is past sample i
        while (lo_b < hi_b) {
            const int mid = (lo_b + hi_b) >> 1;
            int v = bk[mid];
            v = v > N ? N : v;
            if (v > i) hi_b = mid;
            else lo_b = mid + 1;
        }
        const int t = letters.kmer(lo_b);
        const double m = p.model[2 * t], s = p.model[2 * t + 1];
        const double u = unit(draw(2 + (u64)i));
        double level;
        if (rows == 0) {
            const double lo = -s;
            level = lo + (s - lo) * u;
        } else {
            level = ppnd16(level_pa + u * level_pw) * s;
        }
        double v = m + level;
        if (p.noise_std > 0.0) v = v + ppnd16(noise_pa + unit(draw(2 + (u64)total + (u64)i)) * noise_pw) * sigma;
        out[i] = (float)((v - med) / mad);
    }
    finish(n_pos, med, mad, 0);
}

}  // namespace

namespace xb {

hipError_t launch_synth(const SpikeParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(synth_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_spike(const SpikeParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(spike_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace xb
