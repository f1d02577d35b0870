// xb_splice.hip -- xb_splice_chunks: the reference's per_kmer XNA augmentation (ub-bonito/bonito/stitch_chunks.py; contract:
// the public header).  Built with -ffp-contract=off: the resampling is numpy's float64 arithmetic operation by operation,
// bit-equal to the CPU restatement (tests/splice_ref.py).
//
// One wave per chunk, one launch per call.  The wave copies its signal and label rows (16-byte accesses when the rows allow
// it), then works on the copy:
//   positions   (xb_positions.h, shared with xb_spike.hip) the validity mask of the chunk's bases is a bit set in LDS (a word
//               per lane and pass); a round finds the k-th valid base from the words' popcounts (a wave scan), marks it in a
//               second bit set and clears its surroundings.  Walking the second set in word order handles the positions in
//               ascending order without a sort.
//   draws       draw k is a pure function of (seed, global chunk index, k): every lane computes the wave-uniform ones
//               itself; the up to 32 draws of a candidate sample are taken one per lane and the partial Fisher-Yates
//               permutation is then resolved in wave-uniform steps (ballot for "who wrote this slot last").
//   candidates  lane j reads the length of sampled row j; a wave minimum over (|len - kmer_rep|, j) keeps the first best.
//   resampling  stretch: the <= 600 xp of the six k-mers go to LDS (a lane per point), then a lane per output sample
//               searches its interval and interpolates in float64.  Shrink: a flag per dropped source sample in LDS, then
//               the kept samples are compacted by ballot / popcount.  Values leave as float32, rounded once.
// Control flow is wave-uniform throughout; positions are separated by a barrier, so a later paste may overlap an earlier one
// (pad < 5) and wins, as in the reference's sequential loop.
//
// The kernel reads lengths, labels and breakpoints it did not validate (the _dev form): lengths are clamped to the row,
// labels to 6, breakpoints to the chunk and to non-decreasing order, so that no access leaves the rows whatever they hold.
#include <hip/hip_runtime.h>

#include "xb_internal.h"
#include "xb_positions.h"

namespace {

using xb::SpliceParams;
using namespace xb_pos;       // the draws and the position chooser, shared with xb_spike.hip

constexpr int KM = xb::SPLICE_KMERS;
constexpr int MAX_SLICE = KM * xb::SPLICE_MAX_KMER;       // samples of the six library rows of one paste
constexpr int MASK_WORDS = (xb::SPLICE_MAX_LABELS + 32) / 32;

// numpy.linspace(0, stop, num, dtype=int)[i]: floor(i * (stop / (num - 1))), the last value stop itself
__device__ inline int linspace_floor(int i, int stop, int num)
{
    if (num <= 1) return 0;
    if (i == num - 1) return stop;
    return (int)floor((double)i * ((double)stop / (double)(num - 1)));
}

__global__ __launch_bounds__(64) void splice_kernel(const SpliceParams p)
{
    __shared__ unsigned valid[MASK_WORDS], chosen[MASK_WORDS];
    __shared__ int xp[MAX_SLICE];
    __shared__ unsigned char drop[MAX_SLICE];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;
    const int N = p.N, Lt = p.Lt;
    const float *sig = p.signal + (size_t)c * N;
    float *out = p.out_signal + (size_t)c * N;
    const unsigned char *tgt = p.targets + (size_t)c * Lt;
    unsigned char *out_t = p.out_targets + (size_t)c * Lt;
    const uint16_t *bk = p.bkps + (size_t)c * Lt;

    // ---- the rows' copy
    copy_row(out, sig, N, p.signal, p.out_signal, lane);
    copy_row(out_t, tgt, Lt, p.targets, p.out_targets, lane);

    int length = p.lengths[c];
    length = length < 0 ? 0 : (length > Lt ? Lt : length);
    const int W = (length + 31) >> 5;

    // ---- draws
    const u64 base = mix(p.seed + GAMMA * (p.first_index + (u64)c + 1));
    u64 kdraw = 0;
    auto next = [&]() { return mix(base + GAMMA * ++kdraw); };

    // ---- positions (its first barrier also: the copy has landed before a paste overwrites it)
    choose_positions(valid, chosen, tgt, length, p.pad, p.prop, p.var_prop, next, lane);

    // ---- per position, ascending
    int inserted = 0;
    for (int w = 0; w < W; ++w) {
        unsigned cw = (unsigned)__builtin_amdgcn_readfirstlane((int)chosen[w]);
        while (cw) {
            const int pos = (w << 5) + __ffs((int)cw) - 1;
            cw &= cw - 1;
            if (pos < KM || pos + KM > length) continue;            // never: positions keep 10 bases from either end
            const int ub = p.ubs[bounded(next(), (unsigned)p.n_ubs)];
            int st[2 * KM - 1], bb[KM + 1];
#pragma unroll
            for (int j = 0; j < 2 * KM - 1; ++j) {
                const int v = tgt[pos - KM + 1 + j];
                st[j] = v > 6 ? 6 : v;
            }
#pragma unroll
            for (int j = 0; j <= KM; ++j) {
                int v = bk[pos - KM + j];
                v = v > N ? N : v;
                if (j > 0) v = v < bb[j - 1] ? bb[j - 1] : v;
                bb[j] = v;
            }
            const int ins_st = bb[0], ins_len = bb[KM] - bb[0];
            int off[KM], cnt[KM];
            bool found = true;
#pragma unroll
            for (int i = 0; i < KM; ++i) {
                if (!found) continue;
                int t = 0;
#pragma unroll
                for (int q = 0; q < KM - 1; ++q) t = t * 7 + (q < i ? st[KM + q] : st[q]);
                // (the five labels: the i behind the UB, st[6 .. 5 + i], then the 5 - i in front of it, st[i .. 4])
                const int g = ((ub - 5) * xb::SPLICE_TEMPLATES + t) * KM + (KM - 1 - i);
                const int first = p.table[2 * g], count = p.table[2 * g + 1];
                if (count <= 0) {
                    found = false;
                    continue;
                }
                const int rep = bb[i + 1] - bb[i];
                int row;
                if (p.cand > 1) {
                    const int m = count < p.cand ? count : p.cand;
                    int r_l = -1;
                    if (lane < m) r_l = lane + (int)bounded(mix(base + GAMMA * (kdraw + 1 + (u64)lane)), (unsigned)(count - lane));
                    kdraw += (u64)m;
                    int v_l = 0, o_l = 0;                           // lane j: the value at slot j before its swap, its pick
                    for (int j = 0; j < m; ++j) {
                        const int rj = __shfl(r_l, j);
                        const u64 earlier = ((u64)1 << j) - 1;
                        const u64 mj = __ballot(r_l == j) & earlier;
                        const int vj = mj ? __shfl(v_l, 63 - __clzll((long long)mj)) : j;
                        int oj = vj;
                        if (rj != j) {
                            const u64 mr = __ballot(r_l == rj) & earlier;
                            oj = mr ? __shfl(v_l, 63 - __clzll((long long)mr)) : rj;
                        }
                        if (lane == j) {
                            v_l = vj;
                            o_l = oj;
                        }
                    }
                    int key = 0x7fffffff;
                    if (lane < m) {
                        const int len = p.rows[2 * (first + o_l) + 1];
                        const int d = len > rep ? len - rep : rep - len;
                        key = (d << 6) | lane;
                    }
                    key = wave_min(key);
                    row = first + __shfl(o_l, key & 63);
                } else {
                    row = first + (int)bounded(next(), (unsigned)count);
                }
                row = __builtin_amdgcn_readfirstlane(row);
                off[i] = p.rows[2 * row];
                cnt[i] = p.rows[2 * row + 1];
            }
            if (!found) continue;                                   // abandoned: the draws stay spent

            int cum[KM + 1];
            cum[0] = 0;
#pragma unroll
            for (int i = 0; i < KM; ++i) cum[i + 1] = cum[i] + cnt[i];
            const int slice_len = cum[KM];
            auto fp = [&](int i) {
                int o = off[0] + i;
#pragma unroll
                for (int q = 1; q < KM; ++q) o = i >= cum[q] ? off[q] + (i - cum[q]) : o;
                return (double)(float)p.pool[o];
            };
            float *dst = out + ins_st;

            if (slice_len == ins_len) {
                for (int x = lane; x < ins_len; x += 64) dst[x] = (float)fp(x);
            } else if (slice_len > ins_len) {                       // drop linspace(0, slice_len - 1, n_rmv, dtype=int)
                const int n_rmv = slice_len - ins_len;
                for (int i = lane; i < slice_len; i += 64) drop[i] = 0;
                __syncthreads();
                for (int i = lane; i < n_rmv; i += 64) drop[linspace_floor(i, slice_len - 1, n_rmv)] = 1;
                __syncthreads();
                int kept = 0;
                for (int b0 = 0; b0 < slice_len; b0 += 64) {
                    const int i = b0 + lane;
                    const bool keep = i < slice_len && !drop[i];
                    const u64 m = __ballot(keep);
                    const int at = kept + __popcll(m & (((u64)1 << lane) - 1));
                    if (keep && at < ins_len) dst[at] = (float)fp(i);
                    kept += __popcll(m);
                }
            } else {                                                // stretch: numpy.interp over per-k-mer sample positions
                int left = 0, o = 0;
#pragma unroll
                for (int q = 0; q < KM; ++q) {
                    const int n = cnt[q];
                    const int right = q < KM - 1 ? (linspace_floor(o + n - 1, ins_len - 1, slice_len) +
                                                    linspace_floor(o + n, ins_len - 1, slice_len)) >> 1
                                                 : ins_len - 1;
                    for (int i = lane; i < n; i += 64) {
                        int v = left;
                        if (n > 1) v = i == n - 1 ? right : (int)rint((double)i * ((double)(right - left) / (double)(n - 1)) + (double)left);
                        xp[o + i] = v;
                    }
                    left = right + 1;
                    o += n;
                }
                __syncthreads();
                for (int x = lane; x < ins_len; x += 64) {
                    int lo = 0, hi = slice_len - 1;                 // the largest j with xp[j] <= x; xp[0] = 0
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (xp[mid] <= x) lo = mid; else hi = mid - 1;
                    }
                    const int j = lo;
                    double y = fp(j);
                    if (j != slice_len - 1 && xp[j] != x) {
                        const double f1 = fp(j + 1);
                        const double slope = (f1 - y) / ((double)xp[j + 1] - (double)xp[j]);
                        y = slope * ((double)x - (double)xp[j]) + y;
                    }
                    dst[x] = (float)y;
                }
            }
            if (lane == 0) out_t[pos] = (unsigned char)ub;
            ++inserted;
            __syncthreads();                                        // xp / drop are free again; the paste is in place
        }
    }
    if (lane == 0) {
        p.success[c] = inserted > 0 ? 1 : 0;
        p.inserted[c] = inserted;
    }
}

}  // namespace

namespace xb {

hipError_t launch_splice(const SpliceParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(splice_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace xb
