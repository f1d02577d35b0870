// xb_internal.h -- declarations shared by the translation units of libxnacall.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xb_ctc_lattice.h"
#include "xb_ctc_split.h"

namespace xb {

typedef _Float16 half_t;

// ---------------------------------------------------------------- CRF decode (xb_decode.hip)
struct DecodeParams {
    const float *scores;   // (T, N, ld) fp32, first `cin` columns of each row are used
    int T, N, S, hi, nb;   // hi = nb^(state_len-1)
    int cin, ld, has_blank;
    float blank;
    float *alpha, *beta, *bmax;   // (T+1, N, S) fp32 stashes
    float *qbuf;                  // (T, N, ldq) fp32 log-posteriors written by sweep 2, read by sweep 3
    int ldq;                      // >= S*(nb+1), multiple of 4
    float *logz;                  // (N) or nullptr
    int stop_after;               // 0: full decode; 1: return after the Log forward sweep (alpha, logZ); 2: after the Log
                                  // backward sweep (xb_crf_scans)
    float *beta_out;              // (T+1, N, S) or nullptr: the Log backward scores, written by sweep 2
    int post_mode;                // 1: sweep 2 writes the posteriors P instead of Q = log(P + 1e-8) into qbuf
    int8_t *labels;               // (N, T) or nullptr
    int8_t *seq;                  // (N, T) or nullptr
    int32_t *seq_len;             // (N) or nullptr
    char alphabet[8];
    int debug_stop;               // diagnostic builds only (XB_LSTM_STAMPS): return after sweep 1 / 2
    int debug_lds;                // diagnostic builds only: sweep 2 with lane-linear (conflict-free) LDS addresses, WRONG results
    // qualities (xb_decode_q): set qstr to run the quality variant -- it needs seq and beta_out ((T+1, N, S) workspace) too
    int8_t *qstr;                 // (N, T) or nullptr: quality characters, left-packed in parallel with seq, zero-padded
    uint8_t *moves;               // (N, T) or nullptr (quality variant only): 1 where the step emits a base
    float qscale, qoffset;        // q = -10 log10(error) * qscale + qoffset, before the clamp to [1, 50]
    // letter probabilities (xb_decode_ub): set probs to run the UB variant -- the quality variant plus the per-step letter
    // mass of the move edges, stored by sweep 2 into ubuf, and per base the windowed probability bytes of every letter
    float *ubuf;                  // (N, T, nb) fp32 workspace: e_t[b] per chunk and step
    uint8_t *probs;               // (N, nb, T) or nullptr: plane b = letter alphabet[1 + b], left-packed beside seq, zero-padded
};
hipError_t launch_crf_decode(const DecodeParams &p, hipStream_t stream);
int decode_lanes_per_state(int S, int N);   // 1, 2 or 4 lanes serve one CRF state (env XB_DECODE_LPS overrides for tests)

// ---------------------------------------------------------------- the CTC lattice (xb_ctc.hip; its pure rules: xb_ctc_lattice.h)
// CTC-CRF loss scans: seqdist.ctc_simple logZ over the stay / move lattice of the targets (crf/model.py:102-135) on scores as
// they are given.  Position l of Lt - sl + 1 reads the columns ctc_columns<true> derives from the labels.
struct CtcParams {
    const float *scores;         // (T, N, C) fp32 with the blank column
    int T, N, C;
    const uint8_t *targets;      // (N, Lt) CTC labels 1 .. nb (0 reads as base 0), checked by the caller
    int Lt, nb, sl;
    const int32_t *tlen;         // (N) target lengths (in bases); positions in use = tlen + 1 - sl
    int semiring;                // 0 Log, 1 Max
    float *alpha;                // N slots of (T + 1) (Lt - sl + 1) floats, workspace, required for gstay / gmove
    float *logz;                 // (N) or nullptr
    float *gstay;                // (T, N, n) or nullptr, n = Lt - sl + 1: Log: d logZ / d stay; Max: the one-hot alignment (zeroed by the caller)
    float *gmove;                // (T, N, n - 1) or nullptr (Log only)
    unsigned *error;             // the context's data word: xb::DATA_SCAN_LENGTH (xb_status.h) ORed in when a target length is out of range
};
hipError_t launch_ctc_scan(const CtcParams &p, hipStream_t stream);

// CTC-CRF validation loss: the forward Log sweep of the same lattice on the encoder's own scores.  RAW scores in either layout,
// the labels as references.npy holds them; the normalisation (s - logz_crf / T) is the kernel's (the contract is in the public
// header: xb_ctc_loss).
struct CtcLossParams {
    const float *scores;         // (T, N, ld) fp32 RAW scores
    int T, N, ld, has_blank;
    float blank;                 // the stay score when the scores come without the blank column
    int nb, sl;
    const uint8_t *targets;      // (N, Lt) CTC labels 1 .. nb (0 reads as base 0)
    int Lt;
    const int32_t *tlen;         // (N) target lengths (in bases); positions in use = tlen + 1 - sl
    const float *logz_crf;       // (N) the CRF's log partition function of the same scores
    float *loss;                 // (N) -logz_ctc / tlen
    float *logz;                 // (N) or nullptr: logz_ctc
    unsigned *error;             // the context's data word: xb::DATA_LOSS_LABEL (xb_status.h) ORed in when a target length or a label inside it is out of range
    int threads;                 // 0 = the rule ctc_loss_threads; 64, 128, 256 (experiments: XB_CTC_LOSS_THREADS): ctc_launch's override
};
hipError_t launch_ctc_loss(const CtcLossParams &p, hipStream_t stream);

// The loss with d loss / d scores (the contract is in the public header: xb_ctc_loss_grad).  launch_ctc_grad runs the lattice
// of chunks [first, first + count) -- forward with alpha stashed, backward with the restricted posteriors summed per score
// column in ascending position -- and writes loss, w and the gradient's columns that the chunk's positions map to;
// launch_ctc_grad_fill, after all of them, writes the remaining columns of all N chunks and zeroes the refused chunks.
struct CtcGradParams {
    CtcLossParams l;             // l.ld = the columns of the layout (dense rows); l.loss (N): clamped to [0, loss_clip] when clipping
    int first, count;            // launch_ctc_grad: workgroup i serves chunk first + i with stash slot i
    const float *post;           // (T, N, ldq) the CRF's edge posteriors of the same scores, blank layout (xb_crf_scans)
    int ldq;
    float *stash;                // count slots of `slot` floats, slot >= ctc_grad_slot_floats(T, Lt - sl + 1) (xb_ctc_split.h)
    size_t slot;
    float loss_clip;             // > 0: chunks whose loss lies outside [0, loss_clip] get a zero gradient
    int mean;                    // 1: w = -(1 / length) / N, else -(1 / length)
    float *w;                    // (N) workspace: the lattice kernel leaves a chunk's weight here for the fill kernel
    float *grad;                 // (T, N, l.ld)
};
hipError_t launch_ctc_grad(const CtcGradParams &q, hipStream_t stream);
hipError_t launch_ctc_grad_fill(const CtcGradParams &q, hipStream_t stream);

// ---------------------------------------------------------------- beam search (xb_beam.hip)
// koi.decode.beam_search as compute_scores calls it (crf/basecall.py:43-46): back-guided beam over the CRF with sequence
// hashes, stay / step merging, qualities from k-mer posteriors, moves.  One wave per chunk.
constexpr int BEAM_MAX_WIDTH = 32;
constexpr int BEAM_MAX_STATES = 1024;      // = the CRF scans' limit (launch_crf_decode)
struct BeamParams {
    const float *scores;         // (T, N, ld) fp32
    int ld, has_blank;
    float blank;                 // the stay score when the scores come without the blank column
    const float *alpha, *beta;   // (T + 1, N, S) Log-semiring scans of the same scores (xb_crf_scans)
    const float *logz;           // (N)
    int T, N, S, nb, hi;         // hi = nb^(state_len - 1)
    int W;                       // beam width, 1..BEAM_MAX_WIDTH
    float log_cut;               // log(beam_cut), FLT_MAX = no cut
    float qscale, qoffset;
    char base_chars[8];          // alphabet[1 + base]
    uint32_t *hist;              // (N, T + 1, BEAM_MAX_WIDTH) workspace: state | prev << 16 | stay << 24
    int32_t *path;               // (N, T) workspace: the state of the traced path per block
    float *prob;                 // (N, T) workspace: per-block probability of the path k-mer
    int8_t *seq, *qstr;          // (N, T): ASCII at the emitting blocks, 0 elsewhere
    uint8_t *moves;              // (N, T)
    float *score;                // (N) or nullptr
    // filled in by launch_beam_search: the LDS images of a block's score row and back-guide row
    int row_floats, beta_off, pre_stride, row_vec16, beta_vec16;
};
hipError_t launch_beam_search(const BeamParams &p, hipStream_t stream);

// ---------------------------------------------------------------- encoder (xb_encoder.hip)

// conv1(1->4,k5,p2)+SiLU, conv2(4->16,k5,p2)+SiLU, then the im2col rows of conv3
// (row (t*N+n), col c*winlen+k = a2[c][t*stride - winlen/2 + k]) as split fp16, K padded to kp.
struct ConvFrontParams {
    const float *signal;   // (N, L); with signal2 set: chunks [0, split) come from signal, chunks [split, N) from signal2
    const float *signal2;  // (N - split, L) or nullptr: the second of two batches that share one pass through the encoder
    int split;
    int N, L, T, winlen, stride, kp;
    const float *w1, *b1;  // (4,1,5), (4)
    const float *w2, *b2;  // (16,4,5), (16)
    half_t *a_hi, *a_lo;   // (T*N, kp); a_lo holds the q8 image instead when q8 != 0
    int q8;                // 1: second part = fp8 image (see "q8 image" below), activation exponent 0
};
hipError_t launch_conv_front(const ConvFrontParams &p, hipStream_t stream);

enum GemmEpilogue { EPI_BIAS_F32 = 0, EPI_SILU_SPLIT = 1, EPI_TANH_SCALE = 2 };

// q8 image (precision XB_PREC_F16F8): the second part of every operand is not the fp16 residual but, byte for byte in
// its place, per row and per 32 columns a 64-byte block [h8: 32 x e4m3 of hi * 2^e | l8: 32 x e4m3 of lo * 2^(e+11)]
// (e = the tensor's exponent: 8 for LSTM outputs |h| < 1, 0 for the conv tensors, chosen per weight tensor from max|W|).
// One block-scaled MFMA (K = 64) then computes BOTH correction products of 32 columns: lanes 0-31 feed Ah8 x Bl8,
// lanes 32-63 feed Al8 x Bh8, both with the scale 2^-(ea + eb + 11).

// D[m][n] = sum_k A[m][k] * B[n][k]  (+ epilogue); A, B split fp16 (hi, lo / q8), K multiple of 32.
struct GemmParams {
    const half_t *a_hi, *a_lo;   // (M, lda)
    const half_t *b_hi, *b_lo;   // (Nn, ldb)
    int M, Nn, K, lda, ldb;
    const float *bias;           // (Nn) or nullptr
    float *out_f32;              // EPI_BIAS_F32 / EPI_TANH_SCALE : (M, ldc)
    half_t *out_hi, *out_lo;     // EPI_SILU_SPLIT : (M, ldc)
    int ldc;
    float scale;                 // EPI_TANH_SCALE
    int nb, expand;              // EPI_TANH_SCALE : insert blank column in front of every nb outputs
    float blank;
    int nsplit;                  // 3 = hi*hi + hi*lo + lo*hi ; 1 = hi*hi only ; 2 = hi*hi + fp8 corrections (q8 images)
    int a_exp, b_exp;            // nsplit == 2: exponents of the A and B q8 images
    int out_exp;                 // EPI_SILU_SPLIT, q8 output: exponent of the q8 image written to out_lo
    int out_fmt;                 // EPI_SILU_SPLIT: second part of the output -- 0: this GEMM's own form (q8 image when nsplit == 2,
                                 // else the fp16 residual), 1: fp16 residual, 2: q8 image (what the CONSUMING GEMM's arithmetic reads)
    int gin_n;                   // EPI_BIAS_F32: > 0 selects the member-major gin layout (below) with gin_n chunks per time step
    // gemm4p_kernel (two workgroups per CU, B straight from a fragment-major weight image, see xb_encoder.hip): used when b4
    // is set; otherwise gemm8r_kernel (one 256 x 256 workgroup per CU, both operands through LDS; kept as the A/B reference)
    const unsigned char *b4;     // [K / 32][rows4 / 32][pieces][64 lanes][16 B], rows4 = Nn rounded up to 256 (zero rows); the pieces:
                                 // xb_pack.h (gemm4_pieces), which builds the image
    size_t b4_kstride;           // bytes between consecutive k-tiles of b4 = rows4 / 32 * pieces * 1024
    int one_per_cu;              // gemm4p: 1 = at most one workgroup per CU (launches beside the recurrence)
    int sn;                      // gemm4p: N tiles per XCD super-tile (0 = the rule gemm_super_n; XB_GEMM_SN, experiments)
};
// The three-product arithmetic (nsplit 3) of both GEMM kernels runs on v_mfma_f32_16x16x32_f16 -- per accumulator and k-tile of 32:
// lo*hi, hi*lo, hi*hi (round 5; rounds 1-4 ran it on 32x32x16 per k-step of 16, which sums the same products in another order).
// The chip holds a 13 % higher clock on the 16x16x32 shape (profiles/r05_mfma_shape_ubench.txt).
// gin layout (input projection of an LSTM layer, written by the GEMM, read by lstm_kernel): row m = t * n + chunk, column
// c = unit * 4 + gate.  Stored member-major, [t][c / 128][chunk][c % 128]: the 64 chunks x 128 gate columns a recurrence
// workgroup (32 units) needs per step are ONE contiguous 32 KiB block instead of 64 segments 4F floats apart.
__host__ __device__ inline size_t gin_offset(size_t m, int c, int n, int cols)
{
    const size_t t = m / (size_t)n, chunk = m % (size_t)n;
    return ((t * (size_t)(cols / 128) + (size_t)(c >> 7)) * (size_t)n + chunk) * 128 + (size_t)(c & 127);
}
hipError_t launch_gemm(const GemmParams &p, int epilogue, hipStream_t stream);

// One LSTM layer's recurrence over a slab of chunks.  Gate pre-activations of the input
// projection (+ both biases) are in `gin` with gate-interleaved columns (col = unit*4 + gate,
// gates i,f,g,o); w_hh rows are in the same order.  y receives h_t as split fp16.
struct LstmParams {
    const float *gin;            // (T, N, 4F)
    const half_t *w_hi, *w_lo;   // (4F, F) gate-interleaved rows
    half_t *y_hi, *y_lo;         // (T, N, F)
    float *c_state;              // (N, F) fp32 cell state (in/out across launches)
    half_t *xh;                  // exchange buffer [groups][2 parity][2 parts][64][F] (h of the previous step)
    int T, N, F;
    int n0, nslab;               // chunks [n0, n0+nslab) are processed by this launch
    int grp0;                    // index of this launch's first group in the exchange buffer and the counters (n0 / 64 when the
                                 // whole batch fits the 64 group slots, so that h and the counters survive between the launches
                                 // of different chunk slabs and time slabs; else 0)
    int reverse;                 // time runs T-1..0
    int s_begin, s_end;          // recurrence steps [s_begin, s_end) of this launch (s = 0 is the first step)
    int persistent;              // 1: all steps in one launch with inter-workgroup sync
    unsigned *sync;              // per-group monotonic arrival counters, 64 words per 64-chunk group slot (zeroed once per layer and chunk slab)
    unsigned sync_base;          // arrivals per member already counted by earlier launches of this layer (time slabs)
    unsigned *error;             // the context's sync word: xb::SYNC_LOST (xb_status.h) stored when a sync wait timed out; polled by the waits
    int nsplit;                  // as GemmParams::nsplit (2: w_lo, y_lo and the exchange "lo" part are q8 images, h exponent 8);
                                 // 4: int8-limb recurrence (wq1, wq0, wscale below; y stays hi + q8 image for the next GEMM);
                                 // 5: the same without the d0 x d0 product
    const int8_t *wq1, *wq0;     // nsplit == 4: (4F, F) balanced signed digits of round(W_hh / row scale * 32512), gate-interleaved rows
    const float *wscale;         // nsplit == 4: (4F) row scale / 32512^2: the factor that turns the integer digit sums into W_hh h
    int w_exp;                   // nsplit == 2: exponent of the W_hh q8 image
    int y_alt;                   // 1 (nsplit 2 or 3): y_lo receives the OTHER second part than the exchange image -- the fp16
                                 // residual when nsplit == 2, the q8 image (exponent 8) when nsplit == 3 -- for a next GEMM that
                                 // runs in the other arithmetic
    int spread;                  // 1: spread each group's members over all XCDs (placement-independence test)
    int dual;                    // 1: a workgroup serves two groups alternately (a launch then holds twice the groups)
    int slab;                    // index of this launch among the layer's time slabs (selects the byte of the XCD mask below)
    int xcd_local;               // 1: members prove per launch that their group sits on one XCD (words 1..4 of the group's sync
                                 // slot, one byte per time slab, zeroed with the counters) and then exchange h with plain stores
    // One launch over all steps that reports its time slabs (sig_flag != nullptr): the layer output is stored write-through,
    // and when the last workgroup has finished slab i (steps [T i / sig_nts, T (i + 1) / sig_nts)) it stores sig_base + i + 1
    // to *sig_flag -- the word the GEMM stream waits on (hipStreamWaitValue32) before it consumes that slab.
    unsigned *sig_flag;          // device word, monotonic across layers and batches
    unsigned *sig_done;          // sig_nts arrival counters, zeroed with the group counters
    unsigned sig_base;
    int sig_nts;
};
hipError_t launch_lstm(const LstmParams &p, hipStream_t stream);
// (members -- workgroups per group -- and chunks per group of the LSTM kernel: xb_schedule.h, lstm_members / lstm_group_chunks)
// workgroups of the persistent kernel the occupancy calculator admits per CU for feature size F (0: the kernel cannot be
// resident at all, e.g. LDS or registers taken by another tenant's limits); the persistent mode needs >= 1
int lstm_resident_per_cu(int F, int nsplit, int dual);
bool lstm_supported_features(int F);
// ---------------------------------------------------------------- template mapper (xb_align.hip)
// xb_map_templates: every called row against every template of a small library on both strands (the contract is in the
// public header).  Letters travel as codes: A C G T = 0..3, everything else 4.
constexpr int MAP_MAX_TEMPLATE = 4096;      // longest template
constexpr int MAP_MAX_ROW = 4096;           // widest row of called sequences
constexpr int MAP_CHUNK_BYTES = 16384;      // template codes one score workgroup stages in LDS (whole templates only)
constexpr int MAP_PARTIAL_INTS = 6;         // score, template, strand (0 +, 1 -), end row i, end column j (1-based), second
struct MapParams {
    const int8_t *seq;           // (n, W) ASCII rows, left-packed
    const int32_t *seq_len;      // (n)
    int n, W;
    const uint8_t *tcodes;       // the templates' codes, concatenated
    const int32_t *toff;         // (R + 1) offsets into tcodes
    const int32_t *chunk_first;  // (nchunks + 1) first template of every chunk of at most MAP_CHUNK_BYTES codes
    int R, Lmax, nchunks;
    int match, mismatch, gap_open, gap_extend, ambiguous;
    int32_t *partial;            // (n, nchunks, MAP_PARTIAL_INTS): what the score pass leaves, all it writes
    int32_t *tmpl, *score, *second, *q_st, *q_en, *r_st, *r_en, *n_ops;   // (n)
    int8_t *strand;              // (n) +1 / -1, 0 unmapped
    uint8_t *ops;                // (n, W + Lmax)
    uint8_t *scratch;            // direction bytes of the trace pass when a pair does not fit LDS: trace_wgs x W x Lmax
    int trace_wgs;               // workgroups of the trace pass (each walks reads blockIdx.x, + trace_wgs, ..)
};
// columns per lane of a stripe (1, 2 or 4) for a library whose longest template is Lmax
inline int map_cols_per_lane(int Lmax) { return Lmax <= 64 ? 1 : (Lmax <= 128 ? 2 : 4); }
bool map_trace_in_lds(int W, int Lmax);     // the direction bytes of one pair fit the trace workgroup's LDS
hipError_t launch_map_score(const MapParams &p, hipStream_t stream);
hipError_t launch_map_trace(const MapParams &p, hipStream_t stream);

// xb_ctc_targets: per mapped row the ctc-data verdict and label row (the contract is in the public header).  One wave per row.
constexpr int CTC_FAILED_SEQ = 1, CTC_FAILED_MAP = 2, CTC_SKIPPED_NON_UB = 4, CTC_FAILED_ACC = 8, CTC_FAILED_COV = 16;
inline int ctc_target_width(int Lmax) { return (Lmax + 15) & ~15; }   // bytes per label row
struct CtcTargetParams {
    const int32_t *seq_len;      // (n) as the mapper read it: clamped to [0, W]
    int n, W, cap;               // cap = W + Lmax: bytes per row of ops
    const int32_t *tmpl, *q_st, *q_en, *r_st, *r_en, *n_ops;   // (n) the mapper's outputs
    const int8_t *strand;        // (n)
    const uint8_t *ops;          // (n, cap)
    const uint8_t *tcodes;       // the library image: codes and offsets
    const int32_t *toff;
    int R, TW;                   // TW = ctc_target_width(Lmax)
    double min_accuracy, min_coverage;
    int ub_only, ub_plus, ub_minus;
    int32_t *mlen, *blen, *target_len;   // (n)
    uint8_t *verdict;            // (n)
    uint8_t *target;             // (n, TW), 16-byte aligned
};
hipError_t launch_ctc_targets(const CtcTargetParams &p, hipStream_t stream);

// xb_ub_tally: per mapped row the called letter of every template position, the UB polish and the integer tallies of the
// UB report (the contract is in the public header).  One wave per row.
constexpr int UB_COUNTS = 8;                // int32 per row of counts
constexpr int UB_AREA = 5;                  // a position within this many letters of a UB site lies in the UB area
constexpr int UB_CM_ROWS = 6, UB_CM_COLS = 7;
struct UbTallyParams {
    const int8_t *seq;           // (n, W) ASCII rows, left-packed
    const int32_t *seq_len;      // (n)
    int n, W, cap;               // cap = W + Lmax: bytes per row of ops
    const int32_t *tmpl, *q_st, *r_st, *r_en, *n_ops;   // (n) the mapper's outputs
    const int8_t *strand;        // (n)
    const uint8_t *ops;          // (n, cap)
    const uint8_t *tcodes;       // the library image: codes and offsets
    const int32_t *toff;
    int R;
    int32_t *counts;             // (n, UB_COUNTS)
    int32_t *reads;              // (R, 2) accumulator
    int32_t *err;                // (2, total) accumulator
    int total;                   // letters of the library
    unsigned long long *cm;      // (UB_CM_ROWS, UB_CM_COLS) accumulator (int64 on the host)
};
hipError_t launch_ub_tally(const UbTallyParams &p, hipStream_t stream);

// xb_barcode_dist: per mapped row the edit distance of the template's barcode to the row's letters where the mapping puts
// them, over 2 relax + 1 windows (the contract is in the public header).  One wave per row, a lane per window.
constexpr int BC_MAX_LEN = 64;              // letters of a barcode: one bit each of a 64-bit word
constexpr int BC_MAX_RELAX = 8;             // windows to either side of the expected start
constexpr int BC_MAX_POS = 1 << 30;         // bc_pos: start + relax + bc_len stays an int32
struct BarcodeDistParams {
    const int8_t *seq;           // (n, W) ASCII rows, left-packed
    const int32_t *seq_len;      // (n)
    int n, W;
    const int32_t *tmpl, *q_st, *r_st;   // (n) the mapper's outputs
    const int8_t *strand;        // (n)
    const uint8_t *tletters;     // the library image: the letters as passed in, and the offsets
    const int32_t *toff;
    int R;
    int bc_pos, bc_len, relax;
    int32_t *dist, *start, *end, *obs_len;   // (n)
};
hipError_t launch_barcode_dist(const BarcodeDistParams &p, hipStream_t stream);

// ---------------------------------------------------------------- DTW signal segmentation (xb_dtw.hip)
// xb_dtw_segment: every signal chunk against the expected levels of its reference by dynamic time warping (the contract is
// in the public header).  One wave per chunk; the columns lie across the lanes, cols consecutive columns per lane, in
// stripes of 64 * cols columns.
constexpr int DTW_MAX_SAMPLES = 65535;      // samples per chunk (breakpoints.npy is uint16)
constexpr int DTW_MAX_COLUMNS = 65535;      // ref_rep * levels of one chunk
struct DtwParams {
    const float *signal;         // (n, N) fp32
    const double *levels;        // the chunks' levels, concatenated, before repetition
    const int32_t *off;          // (n + 1) offsets into levels
    const double *window;        // (n) half-width of the slanted band in columns, negative = none
    int N, rep, Kmax;
    int first, count;            // this launch serves chunks first .. first + count - 1, workgroup b chunk first + b
    unsigned long long *scratch; // count slots of slot_words 8-byte words: choice words, then two hand-off columns of N doubles
    size_t choice_words, slot_words;
    int32_t *bp;                 // (n, Kmax)
    int8_t *ok;                  // (n)
    double *cost;                // (n)
};
// columns per lane (1, 2 or 4) for a call whose widest chunk has Mmax columns
inline int dtw_cols_per_lane(int Mmax) { return Mmax <= 64 ? 1 : (Mmax <= 128 ? 2 : 4); }
// 8-byte choice words per stripe / per chunk of N samples and M <= N columns at `cols` columns per lane: a bit per cell of
// the rows a stripe can reach, in batches of 64 rows
constexpr size_t dtw_stripe_words(int N, int M, int cols) { return (size_t)((N - M + 64 * cols + 63) & ~63) * cols; }
constexpr size_t dtw_choice_words(int N, int M, int cols)
{
    return M > N ? 0 : (size_t)((M + 64 * cols - 1) / (64 * cols)) * dtw_stripe_words(N, M, cols);
}
hipError_t launch_dtw(const DtwParams &p, int cols, bool band, hipStream_t stream);

// ---------------------------------------------------------------- XNA spliced augmentation (xb_splice.hip)
// xb_splice_chunks: per DNA chunk the positions, the candidate k-mers of the XNA library, their resampled signal pasted over
// the chunk's own (the contract is in the public header).  One wave per chunk.
constexpr int SPLICE_MAX_SAMPLES = 65535;   // samples per chunk (breakpoints.npy is uint16)
constexpr int SPLICE_MAX_LABELS = 65535;    // entries per label row
constexpr int SPLICE_MAX_CAND = 32;         // cand_sample_size
constexpr int SPLICE_MAX_KMER = 100;        // samples of one library row (the reference's max_kmer_cnt)
constexpr int SPLICE_KMERS = 6;
constexpr int SPLICE_TEMPLATES = 16807;     // 7^5
constexpr int SPLICE_TABLE_LEN = 2 * SPLICE_TEMPLATES * SPLICE_KMERS;
struct SpliceParams {
    const float *signal;         // (n, N) fp32
    const uint8_t *targets;      // (n, Lt) labels 0 .. 6
    const int32_t *lengths;      // (n)
    const uint16_t *bkps;        // (n, Lt): the sample where every base's signal ends
    int n, N, Lt;
    unsigned long long first_index, seed;
    int n_ubs, ubs[2];           // the labels (5, 6) the choice runs over, in its order
    double prop, var_prop;
    int cand, pad;
    const half_t *pool;          // the library: signal pool, rows (n_rows, 2) pool offset and length, table (first row, count)
    const int32_t *rows;
    const int32_t *table;
    float *out_signal;           // (n, N)
    uint8_t *out_targets;        // (n, Lt)
    int8_t *success;             // (n)
    int32_t *inserted;           // (n)
};
hipError_t launch_splice(const SpliceParams &p, hipStream_t stream);

// ---------------------------------------------------------------- XNA synthetic spiking (xb_spike.hip)
// xb_spike_chunks: per DNA chunk the positions, med / mad of its synthetic squiggle by exact selection, the synthetic signal
// of the six k-mers around every position pasted over the chunk's own (the contract is in the public header).  One wave per
// chunk.  The limits of the rows are splice's.
constexpr int SPIKE_MODEL_KMERS = 117649;   // 7^6
constexpr int SPIKE_KMER_REPS = 100;        // squiggle samples per base (compute_med_mad_squiggly's kmer_rep)
constexpr int SPIKE_MAX_ROWS = 32;          // shift values of a truncated-normal level distribution
struct SpikeParams {
    const float *signal;         // (n, N) fp32
    const uint8_t *targets;      // (n, Lt) labels 0 .. 6
    const int32_t *lengths;      // (n)
    const uint16_t *bkps;        // (n, Lt): the sample where every base's signal ends
    int n, N, Lt;
    unsigned long long first_index, seed;
    int ubs_mask;                // 0: none (DNA re-synthesised), 1: X, 2: Y, 3: both
    double prop, var_prop;
    int pad;
    int dist_rows;               // 0: uniform level noise; else the shift values of the truncated normal
    double phi[SPIKE_MAX_ROWS + 1][2];   // per shift value Phi(a), Phi(b) - Phi(a); row dist_rows: the added noise's truncation
    double noise_std;
    int variable_noise;
    const double *model;         // (7^6, 2) level mean (NaN: no such k-mer) and stdv
    float *out_signal;           // (n, N)
    uint8_t *out_targets;        // (n, Lt)
    int32_t *spiked;             // (n)
    double *med, *mad;           // (n)
    int8_t *status;              // (n)
};
hipError_t launch_spike(const SpikeParams &p, hipStream_t stream);
// xb_synth_chunks: the same parameters, positions, selection and draws; the whole chunk is synthesised from the spiked labels
// and the breakpoints (med / mad from the spiked labels too), `spiked` may be 0 with the chunk still synthesised.
hipError_t launch_synth(const SpikeParams &p, hipStream_t stream);

#ifdef XB_LSTM_STAMPS
void lstm_read_stamps(unsigned long long out[10], bool reset);   // diagnostic build only
void gemm_read_stamps(unsigned long long out[8], bool reset);    // diagnostic build only (XB_GEMM_STAMPS)
#endif

}  // namespace xb
