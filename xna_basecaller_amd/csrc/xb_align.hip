// xb_align.hip -- alignment of called sequences: the host-side accuracy of a call against its reference (xb_align_accuracy,
// below), and the device mapper of calls to a template library (xb_map_templates: the two kernels at the end of this file).
//
// `bonito evaluate` scores every call with util.accuracy (ub-bonito/bonito/util.py:402-424):
//     parasail.sw_trace_striped_32(seq, ref, 8, 4, parasail.dnafull) -> CIGAR -> '=' / ('=' + 'I' + 'X' + 'D') * 100,
//     0 when the alignment (its columns, insertions included: util.py:410) is shorter than min_coverage of the reference.
// parasail is a third-party CPU library that no image here has; this is a restatement of what that call computes -- a
// Smith-Waterman local alignment with affine gaps (a gap of length k costs 8 + 4 (k - 1)), match + 5 / mismatch - 4 (the
// A, C, G, T block of NUC.4.4 = parasail.dnafull) -- with two stated choices where the restatement cannot be pinned:
//   * the extended letters X and Y score as ordinary letters (+ 5 / - 4).  parasail's dnafull would read 'Y' as the IUPAC
//     pyrimidine code and has no 'X'; the reference's own XNA accuracies come from analyze_paf.py, not from this function;
//   * among equal-score predecessors the trace-back prefers the diagonal, then a deletion (gap in the query), then an
//     insertion; the end cell is the first maximum in row-major order.
// It is post-processing on the host, like the reference's: nothing of the basecalling path runs here.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xna_basecaller.h"
#include "xb_internal.h"

extern "C" XB_API int xb_align_accuracy(const char *ref, int ref_len, const char *seq, int seq_len, double min_coverage,
                                        int balanced, double *accuracy, int32_t counts[4])
{
    if (!ref || !seq || !accuracy || ref_len < 0 || seq_len < 0) return XB_ERR_INVALID;
    int32_t c4[4] = {0, 0, 0, 0};                       // '=', 'X', 'I' (in the query only), 'D' (in the reference only)
    *accuracy = 0.0;
    if (counts) memcpy(counts, c4, sizeof c4);
    if (ref_len == 0 || seq_len == 0) return XB_OK;
    const int OPEN = 8, EXT = 4, MATCH = 5, MIS = -4;
    const int n = seq_len, m = ref_len;                 // rows: query (seq), columns: reference
    const size_t W = (size_t)m + 1;
    // three full (n + 1) x (m + 1) int32 matrices (the trace-back needs them): bounded -- `bonito evaluate` aligns chunk-level
    // calls of a few thousand bases; 2^26 cells = 768 MiB is far beyond that and far below what would exhaust the host
    if ((size_t)(n + 1) * W > ((size_t)1 << 26)) return XB_ERR_NOMEM;
    const int NEG = -(1 << 28);
    // H: best score ending at (i, j); E: ... with a gap in the query (deletion, consumes ref); F: ... gap in the ref (insertion)
    std::vector<int32_t> H((size_t)(n + 1) * W, 0), E((size_t)(n + 1) * W, NEG), F((size_t)(n + 1) * W, NEG);
    int best = 0, bi = 0, bj = 0;
    for (int i = 1; i <= n; ++i) {
        for (int j = 1; j <= m; ++j) {
            const size_t k = (size_t)i * W + j;
            E[k] = std::max(E[k - 1] - EXT, H[k - 1] - OPEN);
            F[k] = std::max(F[k - W] - EXT, H[k - W] - OPEN);
            const int d = H[k - W - 1] + (seq[i - 1] == ref[j - 1] ? MATCH : MIS);
            int h = std::max(0, d);
            h = std::max(h, std::max(E[k], F[k]));
            H[k] = h;
            if (h > best) { best = h; bi = i; bj = j; }
        }
    }
    if (best == 0) return XB_OK;
    // trace back from (bi, bj) until a cell of score 0
    int i = bi, j = bj, state = 0;                       // 0: in H, 1: in E, 2: in F
    while (i > 0 && j > 0) {
        const size_t k = (size_t)i * W + j;
        if (state == 0) {
            if (H[k] == 0) break;
            const int d = H[k - W - 1] + (seq[i - 1] == ref[j - 1] ? MATCH : MIS);
            if (H[k] == d) { c4[seq[i - 1] == ref[j - 1] ? 0 : 1] += 1; --i; --j; }
            else if (H[k] == E[k]) state = 1;
            else state = 2;
        } else if (state == 1) {
            c4[3] += 1;
            state = (E[k] == H[k - 1] - OPEN) ? 0 : 1;
            --j;
        } else {
            c4[2] += 1;
            state = (F[k] == H[k - W] - OPEN) ? 0 : 2;
            --i;
        }
    }
    if (counts) memcpy(counts, c4, sizeof c4);
    // util.py:410: r_coverage = len(alignment.traceback.ref) / len(ref) -- the traceback string carries a '-' for every column
    // the reference does not take part in, so its length is the number of alignment COLUMNS ('=', X, D and I), not of
    // reference bases
    const int columns = c4[0] + c4[1] + c4[2] + c4[3];
    if ((double)columns / (double)m < min_coverage) return XB_OK;
    const double den = balanced ? (double)(c4[0] + c4[1] + c4[3]) : (double)(c4[0] + c4[1] + c4[2] + c4[3]);
    const double num = balanced ? (double)(c4[0] - c4[2]) : (double)c4[0];
    *accuracy = den > 0 ? 100.0 * num / den : 0.0;
    return XB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// xb_map_templates: exhaustive local alignment of every called row against every template, both strands (contract: the
// public header).  Two kernels.  xb_ctc_targets, the ctc-data verdict and label row of a mapped row, follows them, and
// xb_ub_tally, the per-position UB accuracy tallies of a mapped row, follows that, and xb_barcode_dist, its barcode distance.
//
// Score pass: grid (read, template chunk), a workgroup stages its chunk's template codes and the read's codes in LDS once,
// its waves take the (template, strand) pairs of the chunk in turn.  One wave runs one pair as a systolic array: the
// template lies across the lanes, K consecutive columns per lane (a stripe of 64 K columns; longer templates take several
// stripes, the last column of a stripe handed to the next through a per-wave LDS column of (H, E)), lane l works on query
// row s - l at step s, and takes H and E of its left neighbour's last column with one __shfl_up per value and step; the
// diagonal is the value it took one step earlier.  Only the previous row's H and F of a lane's own K columns live in
// registers.  Per pair the result is (score, first end cell); per workgroup one record of MAP_PARTIAL_INTS ints goes to
// memory -- nothing per cell, nothing per pair.
//
// Trace pass: one wave per read merges the read's records (winner and `second`), runs the winner's pair once more through the
// same cell update, this time storing a direction byte per cell (LDS when the pair fits, else the context's scratch), and
// lane 0 walks back from the end cell.
namespace {

using xb::MapParams;

constexpr int MAP_NEG = -(1 << 28);

struct MapScoring { int match, mis, go, ge, amb; };

struct MapBest { int score, t, s, i, j, sec; };

__device__ inline bool map_better(const MapBest &x, const MapBest &a)
{
    if (x.score != a.score) return x.score > a.score;
    if (x.t != a.t) return x.t < a.t;
    if (x.s != a.s) return x.s < a.s;
    if (x.i != a.i) return x.i < a.i;
    return x.j < a.j;
}

// a <- the summary of the union of what a and x summarise: the winner by the tie order, and the best score among the
// templates other than the winner's
__device__ inline void map_merge(MapBest &a, const MapBest &x)
{
    // field by field: selecting whole structs sends them through private memory
    const bool take = x.score > 0 && (a.score <= 0 || map_better(x, a));      // x wins
    const bool both = x.score > 0 && a.score > 0;
    const int l_score = take ? a.score : x.score, l_t = take ? a.t : x.t, l_sec = take ? a.sec : x.sec;   // the loser
    int sec = take ? x.sec : a.sec;
    a.score = take ? x.score : a.score;
    a.t = take ? x.t : a.t;
    a.s = take ? x.s : a.s;
    a.i = take ? x.i : a.i;
    a.j = take ? x.j : a.j;
    if (both) {
        sec = sec > l_sec ? sec : l_sec;
        if (l_t != a.t && l_score > sec) sec = l_score;
    }
    a.sec = sec;
}

__device__ inline int map_code(int8_t c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

// One (read, template, strand) pair on one wave.  q: the read's codes (forward), n of them; strand 1 aligns their reverse
// complement.  t: the template's codes, L of them.  bnd: 2 (n + 1) ints of this wave (needed when L > 64 K).  TRACE: a
// direction byte per cell to dir[(i - 1) * L + (j - 1)]: bits 0-1 where H came from (0 nowhere: H = 0, 1 diagonal, 2 E, 3 F),
// bit 2 E was opened from H, bit 3 F was opened from H.  Returns, on every lane, score << 32 | (65535 - i) << 16 | (65535 - j)
// of the first maximal cell in row-major order (i, j 1-based), or 0.
template <int K, bool TRACE>
__device__ inline unsigned long long map_pair(const uint8_t *q, int n, int strand, const uint8_t *t, int L, const MapScoring sc,
                                              int *bnd, uint8_t *dir, int lane)
{
    unsigned long long best = 0;
    int *bH = bnd, *bE = bnd + (n + 1);
    const int open = sc.go + sc.ge;
    for (int j0 = 0; j0 < L; j0 += 64 * K) {
        const bool more = j0 + 64 * K < L;             // another stripe follows: every column of this one is real
        const int jc = j0 + lane * K;                  // 0-based first column of this lane
        int tc[K], Hp[K], Fp[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            tc[c] = jc + c < L ? (int)t[jc + c] : 4;
            Hp[c] = 0;
            Fp[c] = MAP_NEG;
        }
        int hdiag = 0, last_h = 0, last_e = MAP_NEG;
        const int steps = n + 63;
        for (int s = 0; s < steps; ++s) {
            int in_h = __shfl_up(last_h, 1), in_e = __shfl_up(last_e, 1);
            const int i = s - lane + 1;                // 1-based query row
            const bool active = i >= 1 && i <= n;
            if (lane == 0) {
                in_h = 0;
                in_e = MAP_NEG;
                if (j0 > 0 && active) { in_h = bH[i]; in_e = bE[i]; }
            }
            if (active) {
                int qc = strand ? (int)q[n - i] : (int)q[i - 1];
                if (strand && qc < 4) qc = 3 - qc;
                int hl = in_h, el = in_e, hd = hdiag;
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const int e0 = el - sc.ge, e1 = hl - open;
                    const int e = e0 > e1 ? e0 : e1;
                    const int f0 = Fp[c] - sc.ge, f1 = Hp[c] - open;
                    const int f = f0 > f1 ? f0 : f1;
                    const int sub = ((qc | tc[c]) & 4) ? -sc.amb : (qc == tc[c] ? sc.match : -sc.mis);
                    const int d = hd + sub;
                    int h = d > 0 ? d : 0;
                    const int g = e > f ? e : f;
                    h = h > g ? h : g;
                    const bool real = more || jc + c < L;
                    if (TRACE) {
                        if (real) {
                            const int from = h == 0 ? 0 : (h == d ? 1 : (h == e ? 2 : 3));
                            dir[(size_t)(i - 1) * L + (jc + c)] = (uint8_t)(from | (e == e1 ? 4 : 0) | (f == f1 ? 8 : 0));
                        }
                    }
                    if (real) {
                        const unsigned long long key = ((unsigned long long)(unsigned)h << 32) |
                                                       ((unsigned long long)(65535 - i) << 16) | (unsigned long long)(65535 - (jc + c + 1));
                        if (h > 0 && key > best) best = key;
                    }
                    hd = Hp[c];
                    Hp[c] = h;
                    Fp[c] = f;
                    hl = h;
                    el = e;
                }
                hdiag = in_h;
                last_h = hl;
                last_e = el;
                if (more && lane == 63) { bH[i] = hl; bE[i] = el; }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        if (o > best) best = o;
    }
    return best;
}

// waves of a score workgroup: four, fewer when every wave needs a stripe hand-off column in LDS and the rows are wide
inline int map_score_waves(int W, int Lmax)
{
    if (Lmax <= 64 * xb::map_cols_per_lane(Lmax)) return 4;
    const int fit = 32768 / (8 * (W + 1));
    return fit < 1 ? 1 : (fit > 4 ? 4 : fit);
}
inline size_t map_bnd_ints(int W, int Lmax) { return Lmax <= 64 * xb::map_cols_per_lane(Lmax) ? 0 : 2 * (size_t)(W + 1); }
inline size_t map_row_bytes(int W) { return ((size_t)W + 15) & ~(size_t)15; }

template <int K>
__global__ __launch_bounds__(256) void map_score_kernel(const MapParams p, const int bnd_ints)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t map_smem[];
    uint8_t *tl = map_smem;                                             // MAP_CHUNK_BYTES template codes
    uint8_t *q = tl + xb::MAP_CHUNK_BYTES;                              // the read's codes
    int *part = reinterpret_cast<int *>(q + (((size_t)p.W + 15) & ~(size_t)15));   // a record per wave
    int *bnd = part + 4 * xb::MAP_PARTIAL_INTS;
    const int r = blockIdx.x, chunk = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int t0 = p.chunk_first[chunk], t1 = p.chunk_first[chunk + 1];
    const int base = p.toff[t0], bytes = p.toff[t1] - base;
    for (int k = tid; k < bytes; k += blockDim.x) tl[k] = p.tcodes[base + k];
    int n = p.seq_len[r];
    n = n < 0 ? 0 : (n > p.W ? p.W : n);
    for (int k = tid; k < n; k += blockDim.x) q[k] = (uint8_t)map_code(p.seq[(size_t)r * p.W + k]);
    __syncthreads();
    const MapScoring sc = {p.match, p.mismatch, p.gap_open, p.gap_extend, p.ambiguous};
    MapBest mine = {0, -1, 0, 0, 0, 0};
    if (n > 0) {
        for (int item = wave; item < 2 * (t1 - t0); item += waves) {
            const int t = t0 + (item >> 1), s = item & 1;
            const int off = p.toff[t] - base, L = p.toff[t + 1] - p.toff[t];
            if (L < 1) continue;
            const unsigned long long key = map_pair<K, false>(q, n, s, tl + off, L, sc, bnd + (size_t)wave * bnd_ints, nullptr, lane);
            const MapBest x = {(int)(key >> 32), t, s, 65535 - (int)((key >> 16) & 0xffff), 65535 - (int)(key & 0xffff), 0};
            map_merge(mine, x);
        }
    }
    if (lane == 0) {
        int *o = part + wave * xb::MAP_PARTIAL_INTS;
        o[0] = mine.score; o[1] = mine.t; o[2] = mine.s; o[3] = mine.i; o[4] = mine.j; o[5] = mine.sec;
    }
    __syncthreads();
    if (tid == 0) {
        MapBest all = {0, -1, 0, 0, 0, 0};
        for (int w = 0; w < waves; ++w) {
            const int *o = part + w * xb::MAP_PARTIAL_INTS;
            const MapBest x = {o[0], o[1], o[2], o[3], o[4], o[5]};
            map_merge(all, x);
        }
        int32_t *g = p.partial + ((size_t)r * p.nchunks + chunk) * xb::MAP_PARTIAL_INTS;
        g[0] = all.score; g[1] = all.t; g[2] = all.s; g[3] = all.i; g[4] = all.j; g[5] = all.sec;
    }
}

// LDS of a trace workgroup: the read's codes, the template's codes, the ops written backwards, the stripe hand-off column,
// and the direction bytes when they fit
constexpr size_t MAP_TRACE_LDS = 64 * 1024;
inline size_t map_trace_fixed_bytes(int W, int Lmax)
{
    return map_row_bytes(W) + map_row_bytes(Lmax) + map_row_bytes(W + Lmax) + 4 * map_bnd_ints(W, Lmax);
}

template <int K>
__global__ __launch_bounds__(64) void map_trace_kernel(const MapParams p, const int dir_in_lds)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t map_smem[];
    const size_t wq = ((size_t)p.W + 15) & ~(size_t)15, wt = ((size_t)p.Lmax + 15) & ~(size_t)15;
    const int cap = p.W + p.Lmax;
    const size_t wo = ((size_t)cap + 15) & ~(size_t)15;
    uint8_t *q = map_smem, *tl = q + wq, *rev = tl + wt;
    int *bnd = reinterpret_cast<int *>(rev + wo);
    const size_t bnd_ints = p.Lmax <= 64 * K ? 0 : 2 * (size_t)(p.W + 1);
    uint8_t *dir = dir_in_lds ? reinterpret_cast<uint8_t *>(bnd + bnd_ints)
                              : p.scratch + (size_t)blockIdx.x * (size_t)p.W * (size_t)p.Lmax;
    const int lane = threadIdx.x;
    const MapScoring sc = {p.match, p.mismatch, p.gap_open, p.gap_extend, p.ambiguous};
    for (int r = blockIdx.x; r < p.n; r += gridDim.x) {
        MapBest win = {0, -1, 0, 0, 0, 0};
        for (int c = 0; c < p.nchunks; ++c) {
            const int32_t *g = p.partial + ((size_t)r * p.nchunks + c) * xb::MAP_PARTIAL_INTS;
            const MapBest x = {g[0], g[1], g[2], g[3], g[4], g[5]};
            map_merge(win, x);
        }
        uint8_t *ops = p.ops + (size_t)r * cap;
        if (win.score <= 0) {
            if (lane == 0) {
                p.tmpl[r] = -1; p.strand[r] = 0; p.score[r] = 0; p.second[r] = 0;
                p.q_st[r] = 0; p.q_en[r] = 0; p.r_st[r] = 0; p.r_en[r] = 0; p.n_ops[r] = 0;
            }
            for (int k = lane; k < cap; k += 64) ops[k] = 0;
            continue;
        }
        int n = p.seq_len[r];
        n = n > p.W ? p.W : n;
        const int tb = p.toff[win.t], L = p.toff[win.t + 1] - tb;
        __syncthreads();                               // the previous read's walk is over
        for (int k = lane; k < n; k += 64) q[k] = (uint8_t)map_code(p.seq[(size_t)r * p.W + k]);
        for (int k = lane; k < L; k += 64) tl[k] = p.tcodes[tb + k];
        __syncthreads();
        (void)map_pair<K, true>(q, n, win.s, tl, L, sc, bnd, dir, lane);
        __syncthreads();
        int n_ops = 0;
        if (lane == 0) {
            int i = win.i, j = win.j, state = 0, at = cap;
            while (i > 0 && j > 0) {
                const int d = dir[(size_t)(i - 1) * L + (j - 1)];
                if (state == 0) {
                    const int from = d & 3;
                    if (from == 0) break;
                    if (from == 1) {
                        int qc = win.s ? (int)q[n - i] : (int)q[i - 1];
                        if (win.s && qc < 4) qc = 3 - qc;
                        rev[--at] = (qc < 4 && qc == (int)tl[j - 1]) ? '=' : 'X';
                        --i;
                        --j;
                    } else {
                        state = from == 2 ? 1 : 2;
                    }
                } else if (state == 1) {
                    rev[--at] = 'D';
                    state = (d & 4) ? 0 : 1;
                    --j;
                } else {
                    rev[--at] = 'I';
                    state = (d & 8) ? 0 : 2;
                    --i;
                }
            }
            n_ops = cap - at;
            p.tmpl[r] = win.t; p.strand[r] = win.s ? -1 : 1; p.score[r] = win.score; p.second[r] = win.sec;
            p.q_st[r] = i; p.q_en[r] = win.i; p.r_st[r] = j; p.r_en[r] = win.j; p.n_ops[r] = n_ops;
        }
        n_ops = __shfl(n_ops, 0);
        __syncthreads();
        for (int k = lane; k < cap; k += 64) ops[k] = k < n_ops ? rev[cap - n_ops + k] : (uint8_t)0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// xb_ctc_targets: what `basecaller --save-ctc` decides per chunk (the reference's CTCWriter.run, io.py:495-540) from the
// mapper's outputs: mlen, blen, the verdict byte and, for a kept row, the label row cut from the library image.  One
// workgroup of one wave per row; every branch below depends on the row's scalars alone, so the wave never diverges.
//   mlen      the '=' bytes among the row's n_ops alignment columns: 16 bytes per lane and load, a masked popcount per lane, one wave sum
//   slice     template codes [r_st, r_en) staged in LDS through aligned 16-byte loads (the image is padded to 16 bytes, and an
//             aligned block that holds one byte of a buffer lies in that byte's page), a code 4 anywhere in it noted on the way
//   labels    16 per lane from the staged codes, reversed and complemented on strand -1, one 16-byte store each; the same loop
//             zero-fills the row behind target_len (the whole row when the verdict is not 0)
constexpr int CTC_LDS_BYTES = xb::MAP_MAX_TEMPLATE + 32;

__device__ inline unsigned ctc_byte(const uint4 &v, int j)
{
    const unsigned w = j < 4 ? v.x : (j < 8 ? v.y : (j < 12 ? v.z : v.w));
    return (w >> (8 * (j & 3))) & 0xffu;
}

// bit 7 of every byte of `w` that is '=' and whose bit in the low four of `in` is set
__device__ inline unsigned ctc_eq_mask(unsigned w, unsigned in)
{
    const unsigned x = w ^ 0x3d3d3d3du;                                                  // '=' bytes become 0
    const unsigned zero = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;        // exact per byte: no carry crosses
    return zero & (((in & 1u) << 7) | ((in & 2u) << 14) | ((in & 4u) << 21) | ((in & 8u) << 28));
}

__global__ __launch_bounds__(64) void ctc_targets_kernel(const xb::CtcTargetParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t codes[CTC_LDS_BYTES];
    const int r = blockIdx.x, lane = threadIdx.x;
    int sl = p.seq_len[r];
    sl = sl < 0 ? 0 : (sl > p.W ? p.W : sl);
    int nops = p.n_ops[r];
    nops = nops < 0 ? 0 : (nops > p.cap ? p.cap : nops);
    const int t = p.tmpl[r];

    // mlen: bytes [mis, end) of the row's aligned 16-byte blocks are its columns; a count per lane, then one wave sum
    int mlen = 0;
    {
        const uint8_t *rowp = p.ops + (size_t)r * p.cap;
        const int mis = (int)(reinterpret_cast<uintptr_t>(rowp) & 15), end = mis + nops;
        const uint4 *blk = reinterpret_cast<const uint4 *>(rowp - mis);
        for (int k = lane * 16; k < end; k += 1024) {
            const uint4 v = blk[k >> 4];
            const int lo = mis > k ? mis - k : 0, hi = end - k < 16 ? end - k : 16;      // the block's bytes [lo, hi) count
            const unsigned in = lo < hi ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
            mlen += __popc(ctc_eq_mask(v.x, in) | ctc_eq_mask(v.y, in >> 4) >> 1 | ctc_eq_mask(v.z, in >> 8) >> 2 |
                           ctc_eq_mask(v.w, in >> 12) >> 3);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mlen += __shfl_xor(mlen, d);
    }

    int verdict = (sl == 0 ? xb::CTC_FAILED_SEQ : 0) | ((t < 0 || t >= p.R) ? xb::CTC_FAILED_MAP : 0);
    int tl = 0, shift = 0, st = 0;
    if (verdict == 0) {
        const int tb = p.toff[t], L = p.toff[t + 1] - tb;
        int r0 = p.r_st[r], r1 = p.r_en[r];
        r0 = r0 < 0 ? 0 : (r0 > L ? L : r0);
        r1 = r1 < r0 ? r0 : (r1 > L ? L : r1);
        tl = r1 - r0;
        st = p.strand[r];
        const uint8_t *g0 = p.tcodes + tb + r0;
        shift = (int)(reinterpret_cast<uintptr_t>(g0) & 15);
        const uint4 *gblk = reinterpret_cast<const uint4 *>(g0 - shift);
        bool ub = false;
        for (int k = lane * 16; k < shift + tl; k += 1024) {
            const uint4 v = gblk[k >> 4];
            *reinterpret_cast<uint4 *>(codes + k) = v;
#pragma unroll
            for (int j = 0; j < 16; ++j) ub = ub || (k + j >= shift && k + j < shift + tl && ctc_byte(v, j) >= 4u);
        }
        const bool has_ub = __ballot(ub) != 0ull;
        if (p.ub_only && !has_ub) {
            verdict = xb::CTC_SKIPPED_NON_UB;
        } else {
            // one correctly rounded float64 division each (this translation unit is built without contraction or fast-math)
            const double acc = (double)mlen / (double)nops;
            const double cov = (double)(p.q_en[r] - p.q_st[r]) / (double)sl;
            if (nops == 0 || acc < p.min_accuracy) verdict |= xb::CTC_FAILED_ACC;
            if (cov < p.min_coverage) verdict |= xb::CTC_FAILED_COV;
        }
    }
    __syncthreads();                                   // the staged codes are visible to every lane
    if (verdict != 0) tl = 0;
    const unsigned ubl = (unsigned)(st < 0 ? p.ub_minus : p.ub_plus) & 0xffu;
    uint8_t *row = p.target + (size_t)r * p.TW;
    for (int k0 = lane * 16; k0 < p.TW; k0 += 1024) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (k0 < tl) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + j;
                if (k < tl) {
                    unsigned c = codes[shift + (st < 0 ? tl - 1 - k : k)];
                    if (st < 0 && c < 4u) c = 3u - c;
                    w[j >> 2] |= (c < 4u ? c + 1u : ubl) << (8 * (j & 3));
                }
            }
        }
        *reinterpret_cast<uint4 *>(row + k0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (lane == 0) {
        p.mlen[r] = mlen;
        p.blen[r] = nops;
        p.verdict[r] = (uint8_t)verdict;
        p.target_len[r] = tl;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// xb_ub_tally: the per-read half of the reference's analyze_paf.py -p (compute_read_matches, polish_target_matches,
// compute_errors_paf and the UB-area metrics of utils.py, the confusion matrix of analyze_paf.py:520-536) over the mapper's
// outputs.  One workgroup of one wave per row; the template's letters T, the called letters C and their polished copy P
// live in LDS, a byte per template position each.
//   walk      64 alignment columns per step, one per lane: the row and template positions of a column are the counts of
//             row-consuming / template-consuming columns before it (two ballots and a masked popcount), so every '=' / 'X'
//             column stores its called letter at once; the first column that leaves a range ends the walk for the lanes
//             behind it
//   polish    the UB sites in ascending order, found by a ballot per 64 positions; the conditions read C, which no longer
//             changes, so every lane evaluates them (the '-' run around a deleted site is scanned 64 positions a step);
//             lane 0 alone reads and writes P, in order
//   tallies   per lane over its positions, one wave sum per count; an atomic per wrong position into err, the confusion
//             cells summed in LDS first, then one atomic per non-zero cell
constexpr int UB_LDS_BYTES = xb::MAP_MAX_TEMPLATE;
constexpr int UB_CM_CELLS = xb::UB_CM_ROWS * xb::UB_CM_COLS;

// index of a called byte in the confusion matrix's column order A T C G X Y '-', -1 for any other byte; the complement on
// the reverse strand (A <-> T, C <-> G, X <-> Y, '-' stays) is index ^ 1 below 6
__device__ inline int ub_letter_index(unsigned c)
{
    switch (c) {
    case 'A': return 0;
    case 'T': return 1;
    case 'C': return 2;
    case 'G': return 3;
    case 'X': return 4;
    case 'Y': return 5;
    case '-': return 6;
    default: return -1;
    }
}

// the row's letter at position i of the aligned strand: upper case, on strand -1 read from the far end and complemented
// with the X <-> Y table
__device__ inline unsigned ub_query_letter(const int8_t *row, int sl, int i, bool minus)
{
    unsigned c = (unsigned)(uint8_t)row[minus ? sl - 1 - i : i];
    if (c >= 'a' && c <= 'z') c -= 32u;
    if (minus) {
        switch (c) {
        case 'A': c = 'T'; break;
        case 'T': c = 'A'; break;
        case 'C': c = 'G'; break;
        case 'G': c = 'C'; break;
        case 'X': c = 'Y'; break;
        case 'Y': c = 'X'; break;
        default: break;
        }
    }
    return c;
}

// ones of m from bit 0 up to the first zero
__device__ inline int ub_low_ones(unsigned long long m) { return ~m == 0ull ? 64 : __ffsll((unsigned long long)~m) - 1; }

// the run of '-' in c[0, L) that contains u (c[u] == '-'): every lane calls, every lane gets [*lo, *hi]
__device__ inline void ub_gap_run(const uint8_t *c, int u, int L, int lane, int *lo, int *hi)
{
    int l = u, h = u;
    for (int b = u - 1; b >= 0; b -= 64) {
        const int j = b - lane;
        const int ones = ub_low_ones(__ballot(j >= 0 && c[j >= 0 ? j : 0] == '-'));
        l = b - ones + 1;
        if (ones < 64) break;
    }
    for (int b = u + 1; b < L; b += 64) {
        const int j = b + lane;
        const int ones = ub_low_ones(__ballot(j < L && c[j < L ? j : L - 1] == '-'));
        h = b + ones - 1;
        if (ones < 64) break;
    }
    *lo = l;
    *hi = h;
}

__global__ __launch_bounds__(64) void ub_tally_kernel(const xb::UbTallyParams p)
{
    __shared__ uint8_t T[UB_LDS_BYTES], Cc[UB_LDS_BYTES], P[UB_LDS_BYTES];
    __shared__ unsigned cells[UB_CM_CELLS];
    const int r = blockIdx.x, lane = threadIdx.x;
    int32_t *cnt = p.counts + (size_t)r * xb::UB_COUNTS;
    const int t = p.tmpl[r];
    if (t < 0 || t >= p.R) {                           // unmapped: zeros, nothing accumulated (the whole wave leaves)
        if (lane < xb::UB_COUNTS) cnt[lane] = 0;
        return;
    }
    int sl = p.seq_len[r];
    sl = sl < 0 ? 0 : (sl > p.W ? p.W : sl);
    int nops = p.n_ops[r];
    nops = nops < 0 ? 0 : (nops > p.cap ? p.cap : nops);
    const int tb = p.toff[t], L = p.toff[t + 1] - tb;
    int r0 = p.r_st[r], r1 = p.r_en[r], q0 = p.q_st[r];
    r0 = r0 < 0 ? 0 : (r0 > L ? L : r0);
    r1 = r1 < r0 ? r0 : (r1 > L ? L : r1);
    q0 = q0 < 0 ? 0 : (q0 > sl ? sl : q0);
    const bool minus = p.strand[r] < 0;

    for (int j = lane; j < L; j += 64) {
        const unsigned c = p.tcodes[tb + j];
        T[j] = c < 4u ? (uint8_t)"ACGT"[c] : (uint8_t)'X';
        Cc[j] = '-';
    }
    if (lane < UB_CM_CELLS) cells[lane] = 0u;
    __syncthreads();

    // the walk
    {
        const uint8_t *ops = p.ops + (size_t)r * p.cap;
        const int8_t *row = p.seq + (size_t)r * p.W;
        const unsigned long long below = (1ull << lane) - 1ull;
        int qb = q0, rb = r0;
        for (int k0 = 0; k0 < nops; k0 += 64) {
            const int k = k0 + lane;
            const bool in = k < nops;
            const unsigned op = in ? ops[k] : 0u;
            const bool both = op == '=' || op == 'X';
            const bool isq = both || op == 'I', isr = both || op == 'D';
            const unsigned long long mq = __ballot(isq), mr = __ballot(isr);
            const int qi = qb + __popcll(mq & below), ri = rb + __popcll(mr & below);
            const bool stop = in && ((!isq && !isr) || (isq && qi >= sl) || (isr && ri >= r1));
            const unsigned long long ms = __ballot(stop);
            const int first = ms ? __ffsll(ms) - 1 : 64;
            if (both && lane < first) Cc[ri] = (uint8_t)ub_query_letter(row, sl, qi, minus);
            if (ms) break;
            qb += __popcll(mq);
            rb += __popcll(mr);
        }
    }
    __syncthreads();
    for (int j = lane; j < L; j += 64) P[j] = Cc[j];
    __syncthreads();

    // the polish
    for (int j0 = 0; j0 < L; j0 += 64) {
        const int j = j0 + lane;
        unsigned long long sites = __ballot(j < L && T[j < L ? j : 0] == 'X');
        while (sites) {
            const int u = j0 + __ffsll(sites) - 1;
            sites &= sites - 1ull;
            const unsigned cu = Cc[u];
            if (cu == 'X') continue;
            if (cu == '-') {
                int lo, hi;
                ub_gap_run(Cc, u, L, lane, &lo, &hi);
                if (lane == 0) {
                    if (lo > 0 && Cc[lo - 1] == 'X') { P[lo - 1] = '-'; P[u] = 'X'; }
                    else if (hi < L - 1 && Cc[hi + 1] == 'X') { P[hi + 1] = '-'; P[u] = 'X'; }
                }
            } else if (u >= 1 && u < L - 1 && lane == 0) {
                if (Cc[u - 1] == '-' && Cc[u + 1] == 'X') { P[u - 1] = P[u]; P[u] = 'X'; P[u + 1] = '-'; }
                else if (Cc[u + 1] == '-' && Cc[u - 1] == 'X') { P[u + 1] = P[u]; P[u] = 'X'; P[u - 1] = '-'; }
            }
        }
    }
    __syncthreads();

    // the tallies
    int n_err = 0, ub_len = 0, ub_match = 0, area_len = 0, area_match = 0, detected = 0;
    int32_t *err = p.err + (size_t)(minus ? p.total : 0) + tb;
    for (int j = lane; j < L; j += 64) {
        const unsigned tj = T[j], pj = P[j];
        const bool e = pj != tj, ub = tj == 'X';
        bool area = false;
        if (!ub) {
#pragma unroll
            for (int d = 1; d <= xb::UB_AREA; ++d)
                area = area || (j - d >= 0 && T[j - d >= 0 ? j - d : 0] == 'X') || (j + d < L && T[j + d < L ? j + d : 0] == 'X');
        }
        n_err += e;
        ub_len += ub;
        ub_match += ub && !e;
        area_len += area;
        area_match += area && !e;
        detected += pj == 'X' || pj == 'Y';
        if (e) atomicAdd(err + (minus ? L - 1 - j : j), 1);
        int row = tj == 'A' ? 0 : (tj == 'T' ? 1 : (tj == 'C' ? 2 : (tj == 'G' ? 3 : 4)));
        int col = ub_letter_index(pj);
        if (col >= 0) {
            if (minus) { row ^= 1; col = col < 6 ? col ^ 1 : col; }
            atomicAdd(&cells[row * xb::UB_CM_COLS + col], 1u);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n_err += __shfl_xor(n_err, d);
        ub_len += __shfl_xor(ub_len, d);
        ub_match += __shfl_xor(ub_match, d);
        area_len += __shfl_xor(area_len, d);
        area_match += __shfl_xor(area_match, d);
        detected += __shfl_xor(detected, d);
    }
    __syncthreads();                                   // the cells are complete
    if (lane < UB_CM_CELLS && cells[lane]) atomicAdd(p.cm + lane, (unsigned long long)cells[lane]);
    if (lane == 0) {
        const int n_match = L - n_err;
        cnt[0] = n_match;
        cnt[1] = ub_match;
        cnt[2] = ub_len;
        cnt[3] = area_match;
        cnt[4] = area_len;
        cnt[5] = n_match - ub_match - area_match;
        cnt[6] = L - ub_len - area_len;
        cnt[7] = detected;
        atomicAdd(p.reads + 2 * t + (minus ? 1 : 0), 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// xb_barcode_dist: the reference's get_barcode_match_score (utils.py:1387-1434) over the mapper's outputs.  One workgroup
// of one wave per row.  The barcode B (at most 64 letters) and the stretch of the query the windows can touch (at most
// bc_len + 2 relax = 80 letters from the first window's start) live in LDS, a byte per letter.
//   masks     lane j keeps B[j] in a register; for every letter of the stretch one ballot of (B[j] == letter) is the bit
//             mask of the barcode positions that letter matches: 80 ballots at most, a 64-bit word each, kept in LDS
//   windows   lane w owns window lo + w and runs Myers' bit-vector recurrence (in Hyyro's form) for the GLOBAL distance
//             over its letters: B is the pattern of one word, the vertical deltas start at +1 everywhere (D[j][0] = j) and a
//             +1 is shifted into the horizontal deltas at every letter (D[0][k] = k); the score follows bit len(B) - 1.
//             The 2 relax + 1 <= 17 windows run side by side, each step one letter of every window; a clipped window
//             stops early under a predicate.
//   winner    min over the lanes of (distance, window) packed in one int: the smallest distance, the lowest window.
// No global scratch, no atomics; lane 0 writes the four integers.
constexpr int BC_STRETCH = xb::BC_MAX_LEN + 2 * xb::BC_MAX_RELAX;

__global__ __launch_bounds__(64) void barcode_dist_kernel(const xb::BarcodeDistParams p)
{
    __shared__ uint8_t Qs[BC_STRETCH];
    __shared__ unsigned long long Eq[BC_STRETCH];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int t = p.tmpl[r];
    if (t < 0 || t >= p.R) {                           // unmapped (the whole wave leaves)
        if (lane == 0) { p.dist[r] = -1; p.start[r] = 0; p.end[r] = 0; p.obs_len[r] = 0; }
        return;
    }
    int sl = p.seq_len[r];
    sl = sl < 0 ? 0 : (sl > p.W ? p.W : sl);
    const int tb = p.toff[t], L = p.toff[t + 1] - tb;
    int r0 = p.r_st[r], q0 = p.q_st[r];
    r0 = r0 < 0 ? 0 : (r0 > L ? L : r0);
    q0 = q0 < 0 ? 0 : (q0 > sl ? sl : q0);
    const bool minus = p.strand[r] < 0;
    int start = q0 + p.bc_pos - r0;                     // q0 <= 4096, bc_pos <= 2^30: no overflow
    start = start < 0 ? 0 : start;
    const int lo = start - p.relax < 0 ? 0 : start - p.relax;
    const int nwin = start + p.relax - lo + 1;          // 1 .. 2 relax + 1
    // the barcode: lane j holds B[j], m letters in all
    int m = L - p.bc_pos;
    m = m < 0 ? 0 : (m > p.bc_len ? p.bc_len : m);
    unsigned bj = 0x100u;                               // no byte
    if (lane < m) {
        bj = p.tletters[tb + p.bc_pos + lane];
        if (bj >= 'a' && bj <= 'z') bj -= 32u;
    }
    // the stretch Q[lo, lo + ns): what window lo .. lo + nwin - 1 of bc_len letters can touch, clipped to the row
    int ns = sl - lo;
    ns = ns < 0 ? 0 : (ns > nwin - 1 + p.bc_len ? nwin - 1 + p.bc_len : ns);
    const int8_t *row = p.seq + (size_t)r * p.W;
    for (int k = lane; k < ns; k += 64) Qs[k] = (uint8_t)ub_query_letter(row, sl, lo + k, minus);
    __syncthreads();
    for (int k = 0; k < ns; ++k) {
        const unsigned long long eq = __ballot(bj == (unsigned)Qs[k]);
        if (lane == (k & 63)) Eq[k] = eq;
    }
    __syncthreads();
    // lane w: window i = lo + w, obs = Q[i, i + len)
    const bool mine = lane < nwin;
    int len = sl - (lo + lane);
    len = !mine || len < 0 ? 0 : (len > p.bc_len ? p.bc_len : len);
    int len0 = sl - lo;                                // the first window is the longest
    len0 = len0 < 0 ? 0 : (len0 > p.bc_len ? p.bc_len : len0);
    int score = m;
    if (m == 0) {
        score = len;                                   // an empty barcode: every letter is an insertion
    } else {
        unsigned long long pv = ~0ull, mv = 0ull;
        const unsigned long long top = 1ull << (m - 1);
        for (int s = 0; s < len0; ++s) {
            if (s < len) {
                const unsigned long long eq = Eq[lane + s];     // lane + s < nwin - 1 + bc_len <= BC_STRETCH
                const unsigned long long xv = eq | mv;
                const unsigned long long xh = (((eq & pv) + pv) ^ pv) | eq;
                unsigned long long ph = mv | ~(xh | pv);
                unsigned long long mh = pv & xh;
                score += (ph & top) ? 1 : ((mh & top) ? -1 : 0);
                ph = (ph << 1) | 1ull;
                mh <<= 1;
                pv = mh | ~(xv | ph);
                mv = ph & xv;
            }
        }
    }
    int key = mine ? score * 32 + lane : 0x7fffffff;   // score <= 64, lane <= 16
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int other = __shfl_xor(key, d);
        key = other < key ? other : key;
    }
    if (lane == 0) {
        const int w = key & 31, i = lo + w;
        int ol = sl - i;
        ol = ol < 0 ? 0 : (ol > p.bc_len ? p.bc_len : ol);
        p.dist[r] = key >> 5;
        p.start[r] = i;
        p.end[r] = i + p.bc_len;
        p.obs_len[r] = ol;
    }
}

}  // namespace

namespace xb {

bool map_trace_in_lds(int W, int Lmax)
{
    return map_trace_fixed_bytes(W, Lmax) + (size_t)W * (size_t)Lmax <= MAP_TRACE_LDS;
}

hipError_t launch_map_score(const MapParams &p, hipStream_t stream)
{
    const int waves = map_score_waves(p.W, p.Lmax);
    const int bnd_ints = (int)map_bnd_ints(p.W, p.Lmax);
    const size_t lds = MAP_CHUNK_BYTES + map_row_bytes(p.W) + 4 * MAP_PARTIAL_INTS * sizeof(int) + (size_t)waves * bnd_ints * sizeof(int);
    const dim3 grid(p.n, p.nchunks), block(64 * waves);
    switch (map_cols_per_lane(p.Lmax)) {
    case 1: hipLaunchKernelGGL(map_score_kernel<1>, grid, block, lds, stream, p, bnd_ints); break;
    case 2: hipLaunchKernelGGL(map_score_kernel<2>, grid, block, lds, stream, p, bnd_ints); break;
    default: hipLaunchKernelGGL(map_score_kernel<4>, grid, block, lds, stream, p, bnd_ints); break;
    }
    return hipGetLastError();
}

hipError_t launch_map_trace(const MapParams &p, hipStream_t stream)
{
    const int in_lds = map_trace_in_lds(p.W, p.Lmax) ? 1 : 0;
    const size_t lds = map_trace_fixed_bytes(p.W, p.Lmax) + (in_lds ? (size_t)p.W * (size_t)p.Lmax : 0);
    const dim3 grid(p.trace_wgs), block(64);
    switch (map_cols_per_lane(p.Lmax)) {
    case 1: hipLaunchKernelGGL(map_trace_kernel<1>, grid, block, lds, stream, p, in_lds); break;
    case 2: hipLaunchKernelGGL(map_trace_kernel<2>, grid, block, lds, stream, p, in_lds); break;
    default: hipLaunchKernelGGL(map_trace_kernel<4>, grid, block, lds, stream, p, in_lds); break;
    }
    return hipGetLastError();
}

hipError_t launch_ctc_targets(const CtcTargetParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(ctc_targets_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_ub_tally(const UbTallyParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(ub_tally_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_barcode_dist(const BarcodeDistParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(barcode_dist_kernel, dim3(p.n), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace xb
