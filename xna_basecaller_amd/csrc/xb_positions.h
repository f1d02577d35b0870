// xb_positions.h -- what the two ctc-data augmentations (xb_splice.hip, xb_spike.hip) share on the device: the counter-based
// draws and the reference's position chooser (stitch_chunks.py:104-125 = spike_chunks.py:194-215).  Everything here runs in a
// workgroup of ONE wave (64 lanes): the barriers are workgroup barriers, the reductions wave reductions.
#pragma once
#include <hip/hip_runtime.h>

namespace xb_pos {

typedef unsigned long long u64;

constexpr u64 GAMMA = 0x9E3779B97F4A7C15ULL;

__device__ inline u64 mix(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ inline unsigned bounded(u64 z, unsigned m) { return (unsigned)(((z >> 32) * (u64)m) >> 32); }

__device__ inline double unit(u64 z) { return (double)(z >> 11) * 0x1p-53; }

__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ inline int wave_min(int v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

// clears bits lo .. hi - 1 (clipped to 0 .. length); returns how many were set.  Ends with a barrier.
__device__ inline int clear_range(unsigned *bits, long long lo, long long hi, int length, int lane)
{
    if (lo < 0) lo = 0;
    if (hi > length) hi = length;
    int cleared = 0;
    if (lo < hi) {
        const int w0 = (int)(lo >> 5), w1 = (int)((hi - 1) >> 5);
        for (int w = w0 + lane; w <= w1; w += 64) {
            unsigned m = 0xffffffffu;
            if (w == w0) m &= 0xffffffffu << (int)(lo & 31);
            if (w == w1) {
                const int e = (int)(hi - ((long long)w1 << 5));          // 1 .. 32 bits of the last word
                if (e < 32) m &= (1u << e) - 1u;
            }
            const unsigned old = bits[w];
            cleared += __popc(old & m);
            bits[w] = old & ~m;
        }
    }
    __syncthreads();
    return wave_sum(cleared);
}

// out[0 .. n) = in[0 .. n) for rows of `T`, 16 bytes per lane when the rows allow it (whole: the arrays the rows lie in)
template <class T>
__device__ inline void copy_row(T *out, const T *in, int n, const void *whole_in, const void *whole_out, int lane)
{
    constexpr int PER = 16 / (int)sizeof(T);
    if ((n & (PER - 1)) == 0 && (((uintptr_t)whole_in | (uintptr_t)whole_out) & 15) == 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(in);
        uint4 *o4 = reinterpret_cast<uint4 *>(out);
        for (int i = lane; i < n / PER; i += 64) o4[i] = s4[i];
    } else {
        for (int i = lane; i < n; i += 64) out[i] = in[i];
    }
}

// The positions of one chunk: `valid` and `chosen` are bit sets in LDS of (length + 31) / 32 words; on return the set bits of
// `chosen` are the positions (walking its words in order handles them in ascending order without a sort).  tgt: the chunk's
// labels; next(): the chunk's next sequential draw.  The draws are spent as the reference spends them: the proportion when
// var_prop > 0, then one per round.  Returns the number of positions.
template <class Next>
__device__ inline int choose_positions(unsigned *valid, unsigned *chosen, const unsigned char *tgt, int length, long long pad,
                                       double prop_in, double var_prop, Next &next, int lane)
{
    const int W = (length + 31) >> 5;
    for (int w = lane; w < W; w += 64) {
        valid[w] = 0xffffffffu;
        chosen[w] = 0;
    }
    __syncthreads();
    clear_range(valid, 0, 10, length, lane);
    clear_range(valid, (long long)length - 10, (long long)W << 5, W << 5, lane);

    // ---- existing UBs: counted, and nothing is inserted within 2 pad of one
    int n_exist = 0;
    for (int b0 = 0; b0 < length; b0 += 64) {
        const int i = b0 + lane;
        u64 m = __ballot(i < length && tgt[i] > 4);
        n_exist += __popcll(m);
        while (m) {
            const int pos = b0 + __ffsll((long long)m) - 1;
            m &= m - 1;
            clear_range(valid, pos - 2 * pad, pos + 2 * pad + 1, length, lane);
        }
    }
    int nvalid = 0;
    for (int w = lane; w < W; w += 64) nvalid += __popc(valid[w]);
    nvalid = wave_sum(nvalid);

    double prop = prop_in;
    if (var_prop > 0.0) {
        const double lo = prop_in - var_prop, hi = prop_in + var_prop;
        prop = lo + (hi - lo) * unit(next());
    }
    long long n_pos = (long long)rint((double)length * prop) - n_exist;
    if (n_pos < 1) n_pos = 1;

    int found = 0;
    for (long long round = 0; round < n_pos && nvalid > 0; ++round) {
        unsigned k = bounded(next(), (unsigned)nvalid);
        int pos = -1;
        for (int blk = 0; blk < W; blk += 64) {
            const int w = blk + lane;
            const unsigned bits = w < W ? valid[w] : 0u;
            const int cnt = __popc(bits);
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            const unsigned tot = (unsigned)__shfl(incl, 63);
            if (k < tot) {
                const u64 m = __ballot(incl > (int)k);
                const int L = __ffsll((long long)m) - 1;
                unsigned wb = (unsigned)__shfl((int)bits, L);
                int r = (int)k - __shfl(incl - cnt, L);
                while (r-- > 0) wb &= wb - 1;
                pos = ((blk + L) << 5) + __ffs((int)wb) - 1;
                break;
            }
            k -= tot;
        }
        if (pos < 0) break;                              // cannot happen while nvalid counts the set bits
        pos = __builtin_amdgcn_readfirstlane(pos);
        if (lane == 0) chosen[pos >> 5] |= 1u << (pos & 31);
        nvalid -= clear_range(valid, pos - pad, pos + pad + 1, length, lane);
        ++found;
    }
    return found;
}

}  // namespace xb_pos
