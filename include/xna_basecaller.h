/*
 * xna_basecaller.h -- C ABI of libxnacall.so, the MI355X (gfx950) implementation of the
 * ub-bonito CRF basecalling hot path.
 *
 * The reference (CSB5/XNA_Basecaller) is 100 % Python; its device arithmetic lives in
 * un-vendored CUDA wheels (torch/cuDNN, ont-seqdist-cuda 0.0.4, koi 0.0.5).  There is therefore
 * no native reference interface to mirror: every entry point below replaces a *Python-level*
 * operator of the reference, cited as file:line under /root/reference/ub-bonito/bonito/.
 * The binding a maintainer adds on the reference side is a ctypes stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions across the ABI.
 *   - every function returns XB_OK (0) or a negative xb_status; xb_last_error(ctx) gives text.
 *   - one xb_ctx per GPU, and the GPU to itself: the persistent LSTM kernel keeps up to 192 workgroups (one per CU, all
 *     of the CU's registers) resident and exchanging data for a whole layer; a second tenant on the same device (another
 *     process, a CU mask) can keep part of them from becoming resident, in which case the waiting workgroups give up
 *     after a bounded spin and the next xb_synchronize / xb_collect_chunks reports XB_ERR_DEVICE.
 *   - the ctx owns its HIP streams (a main stream plus two low-priority side streams: the next
 *     layer's input GEMM runs beside the current layer's recurrence; the CRF decode of a batch runs on the MAIN stream
 *     behind its encoder -- round 4's schedule; XB_DECODE_ASYNC=1 restores the side-stream decode beside the next batch's
 *     encoder, the only case in which xb_result_stream is not the main stream) and every device buffer it allocates.  A ctx is
 *     used by one thread at a time (the reference calls compute_scores from ONE pipeline
 *     thread, crf/basecall.py:109-111); distinct ctxs are independent.
 *   - "host" entry points take host buffers owned by the caller and block until the result is
 *     in them.  "_dev" entry points take device pointers valid on the ctx's device (e.g.
 *     torch tensor data_ptr()), enqueue on the ctx's streams and return without waiting.  The ONLY completion
 *     point is xb_synchronize (it joins all of the ctx's streams): call it before reading results or reusing /
 *     freeing the buffers passed in.  Consecutive xb_basecall_chunks_dev calls queue up on the device back to back (no host
 *     synchronisation between them; what runs concurrently is the co-scheduled pair below and, inside a batch, the next layer's
 *     input GEMM beside the current recurrence): give each in-flight batch its own d_seq / d_seq_len -- and its own d_signal
 *     that stays untouched until xb_synchronize (or until work ordered behind xb_result_stream has run).
 *   - a caller that keeps two batches in flight can have them CO-SCHEDULED: after xb_reserve_pairing (an explicit opt-in;
 *     contexts of at most 640 chunks at features 768 -- a pair must fit ONE recurrence launch of two chunk groups per
 *     workgroup: 2 x 8 groups of 64 with a group's members on one XCD, 2 x 10 with the members dealt over all XCDs, which the
 *     library does for 513..640 chunks, XB_LSTM_WIDE=0 restores the 512 limit; XB_FUSE=0 refuses) an xb_basecall_chunks_dev / xb_submit_chunks that finds nothing
 *     held back is itself held back (NOTHING is enqueued yet -- a device-wide synchronise or an event recorded on a stream
 *     fetched earlier does not cover it; its launch status is reported by the call that launches it) until the next such call
 *     arrives; the two batches then go through the encoder and the decode as one -- the recurrence serves two chunk groups
 *     per workgroup and hides one group's hand-off behind the other's arithmetic -- and each call's results land in its own
 *     buffers.  A held-back call is launched on its own, with the weights and the profiling state it was called under, by
 *     every other entry point (xb_load_weights, xb_weights_ready and xb_set_profiling included), by xb_synchronize,
 *     xb_result_stream, xb_collect_chunks of its slot and xb_ctx_destroy; results are the same bytes either way.  Without the
 *     opt-in every asynchronous call is enqueued before it returns.
 *   - layouts are the reference's: signal (N, L) fp32 [= (N,1,L)], scores (T, N, C) fp32
 *     time-major, labels / seq (N, T) int8.
 */
#ifndef XNA_BASECALLER_H
#define XNA_BASECALLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define XB_API __attribute__((visibility("default")))
#else
#define XB_API
#endif

typedef struct xb_ctx xb_ctx;

typedef enum xb_status {
    XB_OK = 0,
    XB_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    XB_ERR_HIP = -2,          /* a HIP runtime call failed */
    XB_ERR_NOMEM = -3,        /* host or device allocation failed */
    XB_ERR_STATE = -4,        /* call out of order (e.g. weights not loaded) */
    XB_ERR_DEVICE = -5,       /* a kernel reported an internal failure (e.g. sync timeout) */
    XB_ERR_NO_GPU = -6        /* no usable gfx950 device */
} xb_status;

/* Arithmetic of the dense projections (Conv1d k19, LSTM, Linear). */
typedef enum xb_precision {
    XB_PREC_F16X3 = 0,        /* split-fp16 MFMA, 3 products, fp32 accumulate: |score err| ~3e-6 */
    XB_PREC_F16 = 1,          /* single fp16 MFMA, fp32 accumulate (the reference's model.half()): ~1e-3 */
    XB_PREC_F16F8 = 2,        /* fp16 main product + both correction products on the block-scaled FP8 MFMA: ~4e-5 */
    XB_PREC_F16F8_IN1 = 3,    /* as F16F8, but the LSTM input projections (45 % of the FLOPs, no feedback through time) keep
                                 only the fp16 main product: |score err| ~6e-4 max / 1e-4 rms, 1.19x the throughput */
    XB_PREC_MIXED = 4         /* the feed-forward projections (conv3, the five LSTM input projections, the CRF linear layer) in
                                 the three-product F16X3 arithmetic, the five recurrent projections (W_hh register-resident,
                                 the critical path) in F16F8.  Default of Model, the CLI and bench.py: |score err| 3.4e-4 max on
                                 trained-like (peaky) weights, where plain F16F8 sits on the 1e-3 tolerance (1.08e-3), at 0.87x
                                 its throughput (profiles/r04_x3_attribution.txt) */
} xb_precision;

/*
 * Model + geometry.  Mirrors config.toml [encoder]/[global_norm]/[labels]
 * (models/xna_r9.4.1_e8_sup@v3.3/config.toml:1-29) and rnn_encoder() (crf/model.py:142-160).
 */
typedef struct xb_config {
    int32_t n_base;           /* len(labels) - 1 : 4, 5 or 6                                   */
    int32_t state_len;        /* [global_norm] state_len (3)                                   */
    int32_t features;         /* [encoder] features (768); multiple of 32                      */
    int32_t winlen;           /* [encoder] winlen (19)                                         */
    int32_t stride;           /* [encoder] stride (5)                                          */
    float scale;              /* [encoder] scale (5.0)                                         */
    float blank_score;        /* [encoder] blank_score (2.0)                                   */
    int32_t chunk_len;        /* samples per chunk L (basecaller chunksize); T = L / stride    */
    int32_t max_batch;        /* largest N passed to any call                                  */
    int32_t precision;        /* xb_precision                                                  */
    int32_t lstm_mode;        /* 0 = auto, 1 = one launch per time step, 2 = persistent kernel */
} xb_config;

/* ---- lifetime ------------------------------------------------------------------------- */

/* Create a context on HIP device `device`.  Replaces Model(config).to(device), util.py:295,365. */
XB_API int xb_ctx_create(xb_ctx **out, int device, const xb_config *cfg);
XB_API void xb_ctx_destroy(xb_ctx *ctx);
/* Text of the last error on `ctx` (or of the last failed xb_ctx_create when ctx is NULL). */
XB_API const char *xb_last_error(const xb_ctx *ctx);
XB_API int xb_device_count(void);

/*
 * Load one tensor of the reference state dict (model.load_state_dict, util.py:354) in PyTorch
 * layout, fp32, from host memory.  `name` is the inference-encoder key:
 *   encoder.{0,1,2}.conv.{weight,bias}          Conv1d (out, in, k)
 *   encoder.{4..8}.rnn.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0}   (4H, H) / (4H), gates i,f,g,o
 *   encoder.9.linear.{weight,bias}              (n_base^(state_len+1), H)
 * `n` is the element count and must match the shape implied by the config.
 */
XB_API int xb_load_weights(xb_ctx *ctx, const char *name, const float *host, int64_t n);
/* Re-layout the loaded tensors for the kernels (model.eval()/.to(device)); requires all 28 tensors. */
XB_API int xb_weights_ready(xb_ctx *ctx);

/* ---- operators -------------------------------------------------------------------------- */

/*
 * Model.forward: scores = model(batch) (crf/basecall.py:53, crf/model.py:212-213, nn.py).
 * signal (n, L) fp32.  scores (T, n, C): C = S*(n_base+1) when expand_blanks != 0 (the
 * LinearCRFEncoder layout with the blank column, nn.py:123-130), else S*n_base.
 */
XB_API int xb_encode(xb_ctx *ctx, const float *signal, int n, int expand_blanks, float *scores);
XB_API int xb_encode_dev(xb_ctx *ctx, const float *d_signal, int n, int expand_blanks, float *d_scores);

/*
 * SeqdistModel.decode_batch + path_to_str + the left-pack of compute_scores
 * (crf/model.py:215-218, 92-100; crf/basecall.py:57-76).
 * scores (T, n, C) fp32, C = S*(n_base+1) if has_blank else S*n_base (blank = cfg.blank_score).
 * labels (n, T) int8 [optional]: per-step arg-max edge % (n_base+1).
 * seq    (n, T) int8 [optional]: ASCII of alphabet[label] for label != 0, left-packed, zero padded.
 * seq_len (n) int32 [optional].   alphabet: n_base+1 bytes, e.g. "NACGTXY".
 */
XB_API int xb_decode(xb_ctx *ctx, const float *scores, int T, int n, int has_blank,
                     const char *alphabet, int8_t *labels, int8_t *seq, int32_t *seq_len);
XB_API int xb_decode_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank,
                         const char *alphabet, int8_t *d_labels, int8_t *d_seq, int32_t *d_seq_len);

/*
 * The same Viterbi decode with per-base qualities and moves (an extension: the reference's Viterbi branch writes the
 * placeholder 'O' and all-zero moves, crf/basecall.py:60-76).  No reference vectors exist for it: PARITY UNPINNED.
 * Specification, with the decode's own quantities (scores M, S = nb^sl, E = nb + 1, hi = nb^(sl-1), the Log-semiring alpha,
 * beta (T+1, S) and logZ exactly as xb_crf_scans returns them, the decode's arithmetic contract):
 *   path      f_t = the arg-max flat edge j*E + k of step t (the decode's label is k = f_t % E); s_t = f_t / E, the
 *             destination state, i.e. the path's state at scan index t+1.
 *   moves     m_t = (k != 0).
 *   p_t       the k-mer posterior of the beam search, in its order of summation: P(x) = exp((alpha[t+1][x] + beta[t+1][x]) - logZ),
 *             p = P(s_t); for b = 0..nb-1: p += P(s_t / nb + hi*b); p += P((s_t % hi)*nb + b);  clamped to [0, 1],
 *             p_t = p > 0 ? exp(0.4 * log p) : 0.
 *   quality   per emitting step t, over its run t .. u-1 (u = the next emitting step, or T): bp = sum p_u,
 *             tot = sum (p_u + (nb-1) * ((1 - p_u) / (nb-1))) (the inner sum one term at a time), e = 1 - bp / tot,
 *             q = e > 0 ? log(e) * -4.3429448190325175 : FLT_MAX, q = q * qscale, q = q + qoffset, clamped to [1, 50],
 *             character (int)(33.5 + q).  Steps before the first move belong to no base.
 * Viterbi and beam-search qualities of one model therefore share one scale.
 *   seq, seq_len  byte-equal to xb_decode's;  qstring (n, T) int8: left-packed and zero-padded in parallel with seq (its i-th
 *             non-zero byte is the quality of the i-th base);  moves (n, T) uint8 [optional]: m_t per time step (not packed).
 */
XB_API int xb_decode_q(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, float qscale,
                       float qoffset, int8_t *seq, int8_t *qstring, uint8_t *moves, int32_t *seq_len);
XB_API int xb_decode_q_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet, float qscale,
                           float qoffset, int8_t *d_seq, int8_t *d_qstring, uint8_t *d_moves, int32_t *d_seq_len);

/*
 * xb_decode_q with per-base letter probabilities (an extension for calling unnatural bases: how sure the decode is of each
 * letter of the alphabet at every called base).  No reference vectors exist for it: PARITY UNPINNED.  Specification, with
 * the quantities of xb_decode_q (scores M, S, E, hi, idx(j, k) = (k - 1) * hi + j / nb for k >= 1, Log alpha / beta, logZ):
 *   P_t(j, k)   the edge posterior exp(((alpha[t][idx(j, k)] + M[t][j][k]) + beta[t+1][j]) - logZ), bit-equal to
 *               xb_crf_scans' post.
 *   m_t[i]      move mass of source state i: its nb move edges (j = (i % hi) * nb + e - 1, k = i / hi + 1, e = 1..nb)
 *               summed in edge order: ((0 + P_t(e = 1)) + P_t(e = 2)) + .. + P_t(e = nb).  Stays emit nothing.
 *   e_t[b]      letter mass of step t, b = 0..nb-1 (every move edge out of i emits letter i / hi + 1): over the hi sources
 *               i = b * hi + q, lane g = 0..15 first sums x_g = 0 + m_t[b*hi + g] + m_t[b*hi + g + 16] + .. (increasing q);
 *               then four rounds of x_g = x_{g-d} + x_g for g >= d, d = 1, 2, 4, 8 (all g of a round at once); e_t[b] = x_15.
 *   bases       the emitting steps t_1 < .. < t_L of the decode's own path (m_t = 1 of xb_decode_q): the packed sequence.
 *   window      of base i: W_i = t_{i-1} + 1 .. t_{i+1} - 1 with t_0 = -1, t_{L+1} = T (neighbouring windows overlap).
 *   mass_i[b] = 0 + e_u[b] summed over u in W_i in increasing u;  tot_i = mass_i[0] + mass_i[1] + .. (letter order).
 *   prob_i[b] = mass_i[b] / tot_i, or 0 for every letter when tot_i = 0 (everything underflowed: no information).
 *   byte        v = min(255, (int)(256 * prob_i[b])): SAM ML's 1/256 binning.
 *   probs (n, nb, T) uint8: plane b is letter alphabet[1 + b], left-packed and zero-padded in parallel with seq exactly as
 *             qstring is (the i-th byte of a chunk's row in plane b belongs to base i).  seq, seq_len, qstring and moves are
 *             byte-equal to xb_decode_q's (moves may be NULL).
 */
XB_API int xb_decode_ub(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, float qscale,
                        float qoffset, int8_t *seq, int8_t *qstring, uint8_t *moves, uint8_t *probs, int32_t *seq_len);
XB_API int xb_decode_ub_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet,
                            float qscale, float qoffset, int8_t *d_seq, int8_t *d_qstring, uint8_t *d_moves, uint8_t *d_probs,
                            int32_t *d_seq_len);

/*
 * The Log-semiring scans of the CRF on their own (seqdist `sparse` operators behind crf/model.py:41-61): any of
 *   alpha (T+1, n, S)  CTC_CRF.forward_scores  (crf/model.py:50-54): alpha_0 = 0, alpha_{t+1}[j] = LSE_k(M[t,j,k] + alpha_t[idx[j,k]])
 *   beta  (T+1, n, S)  CTC_CRF.backward_scores (crf/model.py:56-60): beta_T = 0, beta_t[i] = LSE over edges (j,k) leaving i of
 *                      (M[t,j,k] + beta_{t+1}[j])
 *   logz  (n)          CTC_CRF.logZ            (crf/model.py:41-46): LSE_j alpha_T[j]   (`normalise` = scores - logz / T)
 *   post  (T, n, S*(n_base+1))  the edge posteriors exp(alpha_t[src] + M + beta_{t+1}[dst] - logZ) = d logZ / d scores
 *                      (seqdist `posteriors`, Log semiring; the blank column is part of the layout also when the scores
 *                      come without it); the _dev variant writes rows of stride (S*(n_base+1) + 3) & ~3 floats.
 * NULL outputs are skipped (alpha/logz alone stop after the forward sweep).  Same arithmetic contract as the decode:
 * bit-equal to the oracle.  xb_crf_logz = xb_crf_scans with only logz.
 */
XB_API int xb_crf_scans(xb_ctx *ctx, const float *scores, int T, int n, int has_blank,
                        float *alpha, float *beta, float *logz, float *post);
XB_API int xb_crf_scans_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank,
                            float *d_alpha, float *d_beta, float *d_logz, float *d_post);
XB_API int xb_crf_logz(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, float *logz);
XB_API int xb_crf_logz_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, float *d_logz);

/*
 * Beam search with qualities and moves: the non-Viterbi branch of compute_scores (crf/basecall.py:33-46:
 * `sequence, qstring, moves = koi.decode.beam_search(scores, beam_width=32, beam_cut=100.0, scale=1.0, offset=0.0,
 * blank_score=2.0)`, selected when the model's last layer has expand_blanks = False).  koi 0.0.5 is not part of the
 * reference tree; the algorithm restated is the one ONT publishes for this decoder (back-guided beam with CRC-32C sequence
 * hashes, stay / step merging, beam cut by bisection, k-mer posterior qualities), generalised to n_base in 2..7 -- its
 * specification is the "CRF beam search" section of oracle/xna_oracle.c, against which the kernel is bit-exact.  PARITY UNPINNED.
 *   scores    (T, n, C) fp32; has_blank = 0: C = S * n_base and the stay score is the context's blank_score (what the
 *             reference passes); has_blank = 1: the stay score is column 0 of every state row.
 *   beam_width 1..32; beam_cut >= 1 (candidates below max - log(beam_cut) are dropped; <= 0: no cut; inside (0, 1) the
 *             logarithm is negative, no candidate can reach the threshold and the beam would be empty: XB_ERR_INVALID);
 *             qscale / qoffset = koi's scale / offset on the phred value.  States: at most 1024 (the limit of the scans).
 *             The scores must be finite: a NaN compares below every threshold and empties the beam in the same way, and
 *             that is NOT checked -- the results of such a call are undefined.
 *   sequence, qstring (n, T) int8: the base character alphabet[1 + base] / the quality character (33 + q, q in 1..50) at the
 *             blocks that emit a base, 0 elsewhere (koi.decode.to_str drops the zeros); moves (n, T) uint8 1 = a base is
 *             emitted in this block (moves[0] is always 1); score (n) [optional] the log-sum path score of the result.
 * xb_basecall_chunks_beam = encoder (no blank column) + beam search without the scores leaving the device.
 */
XB_API int xb_beam_search(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, int beam_width,
                          float beam_cut, float qscale, float qoffset, int8_t *sequence, int8_t *qstring, uint8_t *moves,
                          float *score);
XB_API int xb_beam_search_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet,
                              int beam_width, float beam_cut, float qscale, float qoffset, int8_t *d_sequence,
                              int8_t *d_qstring, uint8_t *d_moves, float *d_score);
XB_API int xb_basecall_chunks_beam(xb_ctx *ctx, const float *signal, int n, const char *alphabet, int beam_width,
                                   float beam_cut, float qscale, float qoffset, int8_t *sequence, int8_t *qstring,
                                   uint8_t *moves, float *score);

/*
 * The CTC-CRF loss scans (CTC_CRF.ctc_loss and ctc_viterbi_alignments, crf/model.py:102-135: prepare_ctc_scores +
 * seqdist.ctc_simple.logZ_cupy / viterbi_alignments), for `bonito evaluate` / fine-tuning on the same device:
 *   scores  (T, n, S*(n_base+1)) fp32 with the blank column -- ctc_loss passes the NORMALISED scores
 *           (scores - xb_crf_logz / T, crf/model.py:48-49,120-121); targets (n, Lt) int32 CTC labels (1..n_base, 0 = padding);
 *           target_lengths (n) in bases, state_len <= length <= Lt.  With np = Lt - state_len + 1 target positions the lattice
 *           has a stay edge per position (score column stay_idx) and a move edge between consecutive positions (move_idx).
 *   xb_ctc_logz:  logz (n) = log-sum over all monotone paths that end at position target_length - state_len at time T
 *           (loss = -logz / target_length);  gstay (T, n, np) / gmove (T, n, np-1) [optional] = d logz / d stay, d logz / d move,
 *           the restricted posteriors -- scatter-added over (stay_idx, move_idx) they are d logz / d scores.
 *   xb_ctc_alignments:  the Max-semiring path: alignments (T, n, np) one-hot over positions (where the best path sits before
 *           step t: seqdist's stay.grad + shifted move.grad; ties prefer the stay edge), max_score (n) [optional].
 * Same arithmetic contract as the decode (bit-equal to the oracle; seqdist itself is absent: "parity unpinned").
 */
XB_API int xb_ctc_logz(xb_ctx *ctx, const float *scores, int T, int n, const int32_t *targets, int Lt,
                       const int32_t *target_lengths, float *logz, float *gstay, float *gmove);
XB_API int xb_ctc_alignments(xb_ctx *ctx, const float *scores, int T, int n, const int32_t *targets, int Lt,
                             const int32_t *target_lengths, float *alignments, float *max_score);

/*
 * The validation loss from RAW scores where they lie (validate_one_step, training.py:159-173:
 * CTC_CRF.ctc_loss(scores, targets, lengths, normalise_scores=True, reduction='none', loss_clip=None), crf/model.py:118-131).
 *   scores  (T, n, C) fp32 RAW encoder scores, 1 <= T <= the context's T; has_blank = 1: C = S*(n_base+1); has_blank = 0:
 *           C = S*n_base, the fused path's layout: a stay edge scores the context's blank_score, the move edge into position
 *           l + 1 reads column state*n_base + base (the correspondence of xb_decode and xb_beam_search).
 *   targets (n, Lt) uint8 CTC labels as references.npy holds them (1..n_base, 0 = padding, read as clamp(label - 1, 0));
 *           target_lengths (n) int32 in bases, state_len <= length <= Lt; Lt - state_len + 1 <= 2048 positions.  The gather
 *           columns of prepare_ctc_scores (crf/model.py:102-116) are derived from the labels on the device.
 *   Arithmetic: logz_crf = xb_crf_logz of the scores; every score the lattice reads is s - (logz_crf / (float)T) in fp32 (one
 *           division per chunk, one subtraction per score, as CTC_CRF.normalise; not folded into the result); the forward
 *           recurrence of xb_ctc_logz (sum2 = max, exp, exp, add, log; the stay term before the move term; zero = -1e38);
 *           logz (n) [optional] = alpha_T[length - state_len]; loss (n) = -(logz / (float)length).
 *   A length outside [state_len, Lt] or a label above n_base inside a row's length: XB_ERR_INVALID -- from the host form before
 *           anything is staged, with the chunk's index; from the _dev form, which has nothing on the host to check and returns
 *           without waiting, by the next xb_synchronize (the chunk's loss is then not written).  The context stays usable.
 *   No allocation per call: logz_crf lies in the decode's workspace, the host form stages through the context's buffers.
 * xb_validate_chunks = validate_one_step's device half in one call: signal (n, chunk_len) -> encoder (blank-less scores) ->
 *   Viterbi decode (seq (n, T), seq_len (n): bit-identical to xb_basecall_chunks on the same signal) -> loss (n) from the same
 *   scores; only seq, seq_len and n floats come back.  Joins anything asynchronous first.
 * Parity unpinned: seqdist is absent; bit-equal to the oracle's restatement (oracle.ctc_logz on the normalised,
 * blank-expanded scores).
 */
XB_API int xb_ctc_loss(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const uint8_t *targets, int Lt,
                       const int32_t *target_lengths, float *loss, float *logz);
XB_API int xb_ctc_loss_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const uint8_t *d_targets, int Lt,
                           const int32_t *d_target_lengths, float *d_loss, float *d_logz);
XB_API int xb_validate_chunks(xb_ctx *ctx, const float *signal, int n, const char *alphabet, const uint8_t *targets, int Lt,
                              const int32_t *target_lengths, int8_t *seq, int32_t *seq_len, float *loss);

/*
 * The training criterion with its gradient, where the scores lie: the loss of
 * CTC_CRF.ctc_loss(scores, targets, lengths, loss_clip, reduction, normalise_scores=True) (crf/model.py:118-131) per chunk, and
 * d (reduced loss) / d RAW scores -- what the reference obtains by autograd through seqdist.
 *   scores, targets, target_lengths, has_blank, the limits and the lattice arithmetic: those of xb_ctc_loss (every fetched score
 *           is s - logz_crf / (float)T; forward recurrence with alpha_0 .. alpha_T kept; the backward recurrence of xb_ctc_logz:
 *           beta_t[l] = sum2(stay + beta_{t+1}[l], move + beta_{t+1}[l+1]), sum2 = max, exp, exp, add, log, zero = -1e38).
 *   loss_clip > 0 clips (<= 0: no clipping); mean != 0: reduction 'mean', else 'none'.
 *   R[t, col] = the sum, over the positions l of the chunk whose stay (move) column is col, in ASCENDING l and starting from
 *           0.0f, of the restricted posteriors of xb_ctc_logz (gstay / gmove):
 *           exp(((alpha_t[l] + stay) + beta_{t+1}[l]) - logz),  exp(((alpha_t[l] + move) + beta_{t+1}[l+1]) - logz).
 *           Positions that share a column (a repeated k-mer) are added in that order and no other: the result is the same
 *           bytes on every run (no floating-point atomics), and the bytes of np.add.at over the positions.
 *   P[t, col] = the CRF edge posterior of xb_crf_scans (post) of the same raw scores.
 *   w[b]    = -(1.0f / (float)length[b]), then / (float)n when mean; 0 where loss_clip > 0 and the unclipped loss lies outside
 *           [0, loss_clip].
 *   grad (T, n, C) fp32, dense, in the layout of scores: grad[t, b, col] = (R - P) * w[b], three fp32 operations, no
 *           contraction; columns no position maps to get (0.0f - P) * w.  has_blank = 0: the C = S*n_base columns are the
 *           with-blank gradient without the blank columns (the blank is a constant): the stay edges add nothing, the move
 *           column state*n_base + base takes P from column state*(n_base+1) + base + 1.
 *   loss (n) = xb_ctc_loss's, clamped to [0, loss_clip] when loss_clip > 0 (the mean over the chunks is the caller's).
 *   Validation as xb_ctc_loss: the host form refuses a bad length or label with the chunk's index before anything is staged; the
 *           _dev form reports it by the next xb_synchronize (XB_ERR_INVALID), the offending chunk's loss is not written and its
 *           gradient is all zero (either sign), the other chunks' results are right, and the context stays usable.
 *   Precondition: every row has a path, T >= length - state_len.  A row without one gives unspecified values.
 *   Workspace: the alpha stash ((T + 1) x (Lt - state_len + 1) floats per chunk) belongs to the context and grows with the calls;
 *           one launch owns at most XB_CTC_SCRATCH_MB megabytes of it (default 1024, read on every call), so a call runs as
 *           launches of as many chunks as fit, at least one; the result does not depend on the split.  P lies in the decode's
 *           workspace.  Not a stage of xb_get_stage_times.  The _dev form returns without waiting, its outputs are ordered on
 *           xb_result_stream.
 * Parity unpinned: seqdist is absent; bit-equal to the restatement tests/ctcgrad_ref.py (oracle.decode, oracle.ctc_logz, np.add.at).
 */
XB_API int xb_ctc_loss_grad(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const uint8_t *targets, int Lt,
                            const int32_t *target_lengths, float loss_clip, int mean, float *loss, float *grad);
XB_API int xb_ctc_loss_grad_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const uint8_t *d_targets, int Lt,
                                const int32_t *d_target_lengths, float loss_clip, int mean, float *d_loss, float *d_grad);

/*
 * Training the CRF head with everything below it frozen: `bonito train -F` at --num-unfreeze-top 1 (cli/train.py:134-158), where
 * the one trainable layer is LinearCRFEncoder, scores = scale * tanh(X W^T + b) (encoder.9.linear.{weight,bias}), and no
 * gradient with respect to X is needed.  C = S * n_base blank-less columns, F = features.
 *
 * xb_head_grad: the gradient of W and b from the gradient of the scores.
 *   y, dy   (rows, C) fp32, dense: the RAW blank-less scores as xb_encode(expand_blanks = 0) writes them, and d loss / d scores
 *           in that layout (xb_ctc_loss_grad with has_blank = 0).
 *   x_hi, x_lo  (rows, F) fp16 bit patterns, value = hi + lo, 16-byte aligned.  Both NULL: the last LSTM layer's output that
 *           the most recent encoder pass left in the context (what xb_debug_layer_output(which = 1) reads); rows must then be
 *           T * n of that pass (XB_ERR_STATE otherwise).  Once the workspaces were replaced (xb_reserve_pairing) nothing of an
 *           earlier pass lies in them: both NULL is XB_ERR_STATE, with dw and db untouched, until the next full encoder pass; so
 *           it is after xb_encode_bottom_dev below the top layer.  After xb_load_weights / xb_weights_ready without a new pass,
 *           both NULL still means the planes that lie there -- those the OLD weights computed.
 *   dw (C, F), db (C) fp32:  dZ = dy * (scale - y * y / scale);  dw[o, f] = sum_m dZ[m, o] X[m, f];  db[o] = sum_m dZ[m, o].
 *   Arithmetic: e = 14 - exponent(max |dy| * scale) (frexp's exponent; 0 for a gradient of zeros): dZ is formed in fp32 as
 *           (dy * 2^e) * (((scale - y) * (scale + y)) / scale) -- scale - y^2 / scale in the form that does not cancel where
 *           tanh saturates -- no contraction, and split into fp16 hi + lo where the operand is loaded
 *           -- it is never written to memory, and a mean loss's gradients of 1e-6 and less do not underflow fp16.  The
 *           products hi*hi + hi*lo + lo*hi run on the fp16 MFMA with fp32 accumulation, as the forward's head does; db sums the
 *           scaled fp32 dZ in float64.  The rows are cut into slabs of whole 32-row tiles, one workgroup per slab and output
 *           tile; a second kernel adds the slabs' partial sums in ascending slab order and multiplies by 2^-e.  No
 *           floating-point atomics: the same bytes on every run.  Measured error: DESIGN.md 4.2.5.
 *   Workspace: the partial sums belong to the context; one launch owns at most XB_HEAD_SCRATCH_MB megabytes of them (default
 *           256, read on every call).  A call that needs more is split over blocks of 64 output rows with the slabs unchanged
 *           -- the same bytes -- and only when one block's slabs alone exceed the bound are the slabs made fewer and longer
 *           (csrc/xb_head_split.h).
 *   Refused (XB_ERR_INVALID, with a message): a context whose head is not computed in three fp16 products (any precision but
 *           XB_PREC_MIXED and XB_PREC_F16X3); a scale that is not positive.  The activation is always tanh here; a model with
 *           another one is refused where its config is read (Model.head_trainer).
 *   The host form stages through the context and returns synchronised; the _dev form returns without waiting, its outputs
 *   are ordered on xb_result_stream.  No counterpart in the reference (autograd through torch.nn.Linear and Tanh).
 */
XB_API int xb_head_grad(xb_ctx *ctx, const float *y, const float *dy, const uint16_t *x_hi, const uint16_t *x_lo, int64_t rows, float *dw,
                        float *db);
XB_API int xb_head_grad_dev(xb_ctx *ctx, const float *d_y, const float *d_dy, const uint16_t *d_x_hi, const uint16_t *d_x_lo, int64_t rows,
                            float *d_dw, float *d_db);

/* *d_norm = (float)sqrt(sum dw^2 + sum db^2), summed in float64 in a fixed order (256 interleaved partial sums, each a tree,
 * then a tree over them): clip_grad_norm_'s total norm (training.py:113). */
XB_API int xb_grad_norm_dev(xb_ctx *ctx, const float *d_dw, int64_t len_w, const float *d_db, int64_t len_b, float *d_norm);

/*
 * torch.optim.AdamW's single-tensor update with torch's defaults (betas 0.9 / 0.999, eps 1e-8; the weight decay arrives in
 * `decay`), one pass over len elements of (p, g, m, v) fp32, every operation rounded to nearest on its own, in this order:
 *   g = g * clip;  p = p * decay;  m = 0.9f * m + (float)(1 - 0.9) * g;  v = 0.999f * v + ((float)(1 - 0.999) * g) * g;
 *   p = p - (step_size * m) / (sqrt(v) / bc2_sqrt + 1e-8f)
 * with, for step t = 1, 2, .. at learning rate lr, computed by the caller in double and rounded once:
 *   decay = 1 - lr * 0.01,  step_size = lr / (1 - 0.9^t),  bc2_sqrt = sqrt(1 - 0.999^t).
 * g keeps the clipped gradient.  Bit-equal to tests/adamw_ref.py; a few ulps from torch, which forms m by lerp.
 */
XB_API int xb_adamw_step_dev(xb_ctx *ctx, float *d_p, float *d_g, float *d_m, float *d_v, int64_t len, float clip, float decay,
                             float step_size, float bc2_sqrt);

/* Rebuild, from fp32 weights (C, F) and bias (C) on the device, what the forward's head reads: the split fp16 rows, the
 * fragment-major image and the bias, byte for byte what xb_weights_ready uploads for the same floats.  Three-product heads only. */
XB_API int xb_head_repack_dev(xb_ctx *ctx, const float *d_w, const float *d_b);

/*
 * The trainer.  xb_head_train_begin takes the head's fp32 master weights (C, F) and bias (C) from the host, zeroes AdamW's moments
 * and the step count on the device and repacks, so the forward reads exactly these floats.  While it is open xb_load_weights is
 * refused (XB_ERR_STATE).  xb_head_train_step runs one step on n chunks (signal (n, chunk_len), targets (n, Lt) uint8 labels,
 * lengths (n), validated as xb_ctc_loss's host form does), with nothing score-sized leaving the device:
 *   encoder, blank-less scores -> xb_ctc_loss_grad (reduction mean, no loss_clip) -> xb_head_grad on the encoder's own layer
 *   output -> xb_grad_norm -> clip = (float)min(1, 2.0 / ((double)norm + 1e-6)) (clip_grad_norm_(max_norm = 2.0)) ->
 *   xb_adamw_step on W, then on b, at step t = steps taken + 1 -> xb_head_repack.
 *   *loss = (float)(the chunks' losses summed in double in index order / n), before the step; *grad_norm before clipping.
 *   A gradient whose norm is not finite leaves the weights unchanged (XB_ERR_DEVICE).
 * xb_head_get_weights reads the master weights back; xb_head_train_end frees the trainer's state -- the context goes on
 * computing with the trained head until weights are loaded again.  Calls outside begin .. end: XB_ERR_STATE.
 */
XB_API int xb_head_train_begin(xb_ctx *ctx, const float *w, const float *b);
XB_API int xb_head_train_step(xb_ctx *ctx, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, float lr,
                              float *loss, float *grad_norm);
XB_API int xb_head_get_weights(xb_ctx *ctx, float *w, float *b);
XB_API int xb_head_train_end(xb_ctx *ctx);

/*
 * One LSTM layer's recurrence for training: the forward that keeps what the backward needs, and the backward through time --
 * the step that `bonito train -F` above --num-unfreeze-top 1 needs from the top LSTM layer on.  One unidirectional layer with
 * torch.nn.LSTM's semantics: gate order i, f, g, o, h_-1 = c_-1 = 0; reverse != 0 processes the time axis from T-1 down to 0
 * and stores every output at its own t (nn.py:189-193: flip, rnn, flip).  F is independent of the context's model: the context
 * gives the stream, the error message and the workspace.  All tensors fp32, dense, on the device, 16-byte aligned.
 *   gin     (T, n, 4F): gin[t] = x_t W_ih^T + b_ih + b_hh, an INPUT (a non-recurrent product: the caller's).
 *   w_hh    (4F, F) row-major: torch's weight_hh_l0.
 * xb_lstm_train_forward_dev, per step in processing order (p = the step processed before t):
 *   pre = gin[t] + y[p] W_hh^T (at the first step: gin[t]);  (i, f, o) = sigma(pre), g = tanh(pre);
 *   gates[t] (n, 4F) = i | f | g | o after the activation;  c[t] (n, F) = fma(f, c[p], i * g);  y[t] (n, F) = o * tanh(c[t]).
 * xb_lstm_train_backward_dev, per step in the opposite order (s = the step processed after t in the forward), from dy (T, n, F)
 * and the forward's gates and c:
 *   dh = dy[t] + dgin[s] W_hh (at the last processed step: dy[t]);  th = tanh(c[t]);  do = dh * th;
 *   dc = fma(dh * o, (1 - th)(1 + th), carry);  di = dc * g;  df = dc * c[p];  dg = dc * i;  carry = dc * f;
 *   dgin[t] (n, 4F) = di * (i (1 - i)) | df * (f (1 - f)) | dg * ((1 - g)(1 + g)) | do * (o (1 - o)),  zeros written as +0.
 *   dgin is d loss / d gin: d loss / d W_hh = sum_t dgin[t]^T y[p(t)] and the gradients of x, W_ih and the bias follow from it by
 *   products without a recurrence, which are the caller's (crf/lstm.py leaves them to torch).
 * Arithmetic: fp32 throughout.  The recurrent products run on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact f32 operands,
 *   one rounding per product, a fixed k order per output element -- gradients of 1e-9 need no scaling); the forward's sum runs
 *   over K = F, the backward's over K = 4F as four gate-wise partial sums added in gate order.  sigma(x) = 1 / (1 + exp(-x))
 *   and tanh (an odd polynomial below 0.625, 1 - 2 / (exp(2|x|) + 1) above) use the decode's exp, whose argument is clamped:
 *   finite and monotone for every finite x, saturated gates included.  One launch per time step; no workgroup waits for another
 *   inside a kernel; no floating-point atomics: a row's results do not depend on which other rows are in the call, and a call
 *   repeated gives the same bytes.  Measured error against float64: DESIGN.md 4.2.6.
 * The stash is the caller's: y, gates and c are T * n * 6F floats, of which the backward reads gates and c, T * n * 5F floats --
 *   0.71 GB at T = 720, n = 64, F = 768 and 4.2 GB at n = 384.  The workspace (the (n, F) carry and W_hh transposed) belongs to
 *   the context and grows with the calls.
 * Accepted: T >= 1, n >= 1, F a multiple of 16 in 16 .. 1024; anything else, a null pointer or one that is not 16-byte aligned
 *   is XB_ERR_INVALID with the figures.  No weights need to be loaded.  The calls return without waiting; the outputs are
 *   ordered on xb_result_stream.  No counterpart in the reference (autograd through torch.nn.LSTM, cuDNN).
 */
XB_API int xb_lstm_train_forward_dev(xb_ctx *ctx, const float *d_gin, const float *d_w_hh, int T, int n, int F, int reverse,
                                     float *d_y, float *d_gates, float *d_c);
XB_API int xb_lstm_train_backward_dev(xb_ctx *ctx, const float *d_dy, const float *d_w_hh, const float *d_gates, const float *d_c,
                                      int T, int n, int F, int reverse, float *d_dgin);

/*
 * The products of training that carry no recurrence, in fp32 (csrc/xb_train_gemm.hip).  All tensors fp32, dense, on the device;
 * no alignment is asked of them (16-byte aligned operands whose row length is a multiple of 4 are read 16 bytes at a time, others
 * float by float -- the sums are the same).  Products run on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact f32 operands, so a
 * gradient of 1e-9 needs no scaling).  No floating-point atomics; an output element is summed by one wave in an order that its
 * shape alone decides: a repeated call gives the same bytes.  No weights need to be loaded; the calls return without waiting,
 * outputs ordered on xb_result_stream.  No counterpart in the reference (torch autograd, cuBLAS).
 * xb_linear_f32_dev: out (M, N) = act(a (M, K) w (N, K)^T + bias (N) or NULL); act 0 the identity, 1 scale * tanh with the training
 *   recurrence's tanh.  Both operands k-contiguous; the sum of an element runs over k ascending in groups of four (one MFMA), an
 *   order that depends on K alone: a row's results do not depend on the rows beside it.  M, N, K >= 1, any value.  It serves
 *   gin = x W_ih^T + b, the head's scores, and -- given the transposed weight -- dx = dgin W_ih and the head's dX = dZ W.
 * xb_wgrad_f32_dev: dw (N, K)[o, f] = sum_m a (M, N)[m, o] b (M, K)[m, f], dcol (N)[o] = sum_m a[m, o] (NULL: not wanted).  Both
 *   operands arrive row-major over the summed dimension and are turned on their way through LDS.  One workgroup per 64 x 64 tile of
 *   dw walks all of M in ascending order: no partial sums between workgroups, no second kernel, no scratch.  THE BLOCKED FORM
 *   SHIPPED: an element's running fp32 sum (four rows per MFMA) is closed every 1024 rows and added to its total, blocks in
 *   ascending order (DESIGN.md 4.2.7 has the measurement that decided it).  dcol is summed in float64 (four interleaved row
 *   classes, each ascending, added in order) and rounded once.  Zeros are written as +0; M = 0 writes +0 everywhere.  M >= 0,
 *   N, K >= 1.  It serves dW_ih and db (a = dgin, b = x), dW_hh (a and b offset against each other by one time step: a = dgin + n 4F,
 *   b = y forward in time, a = dgin, b = y + n F in a reverse layer, M = (T - 1) n) and the head's dW, db (a = dZ, b = y).
 * xb_head_dz_dev: dz = dy * (((scale - y) * (scale + y)) / scale) over count elements, y the head's output scale * tanh(z): xb_head_grad's
 *   non-cancelling form without its power-of-two factor, one rounding per operation.  scale > 0.
 */
XB_API int xb_linear_f32_dev(xb_ctx *ctx, const float *d_a, const float *d_w, const float *d_bias, int64_t M, int N, int K, int act,
                             float scale, float *d_out);
XB_API int xb_wgrad_f32_dev(xb_ctx *ctx, const float *d_a, const float *d_b, int64_t M, int N, int K, float *d_dw, float *d_dcol);
XB_API int xb_head_dz_dev(xb_ctx *ctx, const float *d_y, const float *d_dy, int64_t count, float scale, float *d_dz);

/*
 * Training the head together with the top L LSTM layers, everything below them frozen: `bonito train -F --no-amp` at
 * --num-unfreeze-top K = L + 1 in 2 .. 6 (cli/train.py:134-158; the unfreeze loop sets requires_grad on every named parameter of
 * an unfrozen layer, so both biases of an LSTM layer train).  fp32 throughout from the frozen bottom's output on: the reference's
 * --no-amp.  F = features, C = S * n_base blank-less columns, T the context's time steps.
 *
 * xb_encode_bottom_dev: the frozen bottom.  It runs the convolutions and the first `layers` (0 .. 5) LSTM layers of the inference
 *   encoder -- the launches of xb_encode, the last layer without a consumer -- and writes that layer's output as x0 (T, n, F) fp32,
 *   16-byte aligned: x0 = (float)hi + (float)lo, one fp32 addition of the two fp16 planes the pass leaves (layers = 4 / 5: what
 *   xb_debug_layer_output(0 / 1) reads after a full pass).  It needs the fp16 residual as second part: any precision but
 *   XB_PREC_MIXED and XB_PREC_F16X3 is XB_ERR_INVALID with a message (the rule of xb_head_grad), as are layers outside 0 .. 5.
 *   Returns without waiting; x0 is ordered on xb_result_stream.
 * xb_transpose_f32_dev: out (cols, rows) = in (rows, cols)^T, fp32, exact (a copy through an LDS tile); rows, cols >= 1, any
 *   value (rows up to 2097120); in and out distinct.  It turns W_ih into (F, 4F) and the head's W into (F, C), the weight
 *   operands of xb_linear_f32_dev's dx products.  No weights need to be loaded.
 *
 * The trainer.  xb_top_train_begin(layers = L in 1 .. 5, params) takes the fp32 master weights from the host as ONE flat array in
 *   state-dict order: for each of encoder.(9 - L) .. encoder.8 the tensors rnn.weight_ih_l0 (4F, F), rnn.weight_hh_l0 (4F, F),
 *   rnn.bias_ih_l0 (4F), rnn.bias_hh_l0 (4F), then encoder.9.linear.weight (C, F) and .bias (C) -- 4 L + 2 tensors, one behind
 *   the other (csrc/xb_top_plan.h).  It allocates four such buffers (p, the gradient g, AdamW's m and v), zeroes m, v and the
 *   step count.  The activations of a step (T n (L 6F + 9F + 3C) floats) are allocated by the first step and grow with the
 *   batch.  An allocation that fails is XB_ERR_NOMEM, with the gigabytes a step needs and the advice to lower the batch.
 *   Refused: L outside 1 .. 5 (the convolutions stay frozen), a precision other than mixed / f16x3, a scale that is not positive
 *   (XB_ERR_INVALID); a second begin, or a head trainer open on the context (XB_ERR_STATE) -- and xb_head_train_begin is refused
 *   while this trainer is open.
 * xb_top_train_grad: the gradient of one batch of n chunks (signal (n, chunk_len), targets (n, Lt) uint8 labels, lengths (n),
 *   validated as xb_head_train_step validates them), in one call, nothing score-sized leaving the device:
 *     xb_encode_bottom with 5 - L layers -> x0;  per unfrozen layer, upwards: b = b_ih + b_hh (fp32, one rounding),
 *     gin = xb_linear_f32(x, W_ih, b), xb_lstm_train_forward (reverse where the LSTM layer's index encoder.N - 4 is even, as in
 *     the inference encoder);  scores = xb_linear_f32(y, W, b, act 1, scale);  xb_ctc_loss_grad (blank-less, ld = C, reduction
 *     mean, no loss_clip);  xb_head_dz;  the head's dW, db = xb_wgrad_f32(dz, y);  dy = xb_linear_f32(dz, W^T);  per layer,
 *     downwards: xb_lstm_train_backward, dW_ih and db = xb_wgrad_f32(dgin, x) with db written to both bias gradients,
 *     dW_hh = xb_wgrad_f32 on the operands shifted by one time step, and for all but the lowest unfrozen layer
 *     dy = xb_linear_f32(dgin, W_ih^T);  xb_grad_norm over the whole flat g.
 *   Every stage is the named entry point's arithmetic on the same operands: the scores and all gradients are, byte for byte, what
 *   those entry points give when a caller chains them (tests/toptrain_dev.py), and a repeated call gives the same bytes.  The
 *   forward reads the fp32 masters: nothing is re-packed per step.  g is left UNCLIPPED.  *loss = (float)(the chunks' losses summed
 *   in double in index order / n); *grad_norm the norm of g.  Returns synchronised.
 * xb_top_train_step: xb_top_train_grad, then clip = (float)min(1, 2.0 / ((double)norm + 1e-6)) and ONE xb_adamw_step over all
 *   the parameters at step t = steps taken + 1 (g keeps the clipped gradient).  *loss is the loss before the step, *grad_norm the
 *   norm before clipping.  A norm that is not finite leaves everything unchanged (XB_ERR_DEVICE).
 * xb_top_get_weights reads the masters back, flat as xb_top_train_begin took them; xb_top_train_end frees the trainer's state.
 *   Calls outside begin .. end: XB_ERR_STATE.
 * The inference forms are NOT the trainer's: xb_encode, xb_basecall_chunks, xb_validate_chunks go on computing with the weights
 *   last loaded.  xb_load_weights and xb_weights_ready stay allowed while this trainer is open; they replace the inference forms
 *   only, the masters remain the trainer's.  That is how trained layers reach the inference path: read the masters, load them
 *   (once per epoch, before validation; crf/trainer.py's TopTrainer.publish).
 * No counterpart in the reference (torch autograd, cuDNN, cuBLAS, torch.optim.AdamW).
 */
XB_API int xb_encode_bottom_dev(xb_ctx *ctx, const float *d_signal, int n, int layers, float *d_x0);
XB_API int xb_transpose_f32_dev(xb_ctx *ctx, const float *d_in, int rows, int cols, float *d_out);
XB_API int xb_top_train_begin(xb_ctx *ctx, int layers, const float *params);
XB_API int xb_top_train_grad(xb_ctx *ctx, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, float *loss,
                             float *grad_norm);
XB_API int xb_top_train_step(xb_ctx *ctx, const float *signal, int n, const uint8_t *targets, int Lt, const int32_t *lengths, float lr,
                             float *loss, float *grad_norm);
XB_API int xb_top_get_weights(xb_ctx *ctx, float *params);
XB_API int xb_top_train_end(xb_ctx *ctx);

/*
 * Training the convolutions (csrc/xb_conv_train.hip), and with them every layer: `bonito train --no-amp` without -f, the
 * reference's headline recipes.  One layer is the `Convolution` of rnn_encoder: Conv1d(Cin, Cout, K, stride, padding = K / 2,
 * bias) followed by swish.  Everything fp32, dense, on the device, 16-byte aligned; generic in (Cin, Cout, K, stride).
 *   x (n, Cin, Lin), w (Cout, Cin, K), b (Cout): torch's layouts.  Lout = (Lin + 2 (K / 2) - K) / stride + 1.
 *   z, y and dy: (n, Cout, Lout) with tnc = 0, (Lout, n, Cout) otherwise -- the encoder's Permute([2, 0, 1]) fused into conv3.
 * xb_conv_train_forward_dev: z[b, co, t] = sum_ci sum_k x[b, ci, t stride + k - K / 2] w[co, ci, k] + b[co] (x is 0 outside
 *   0 .. Lin - 1), the pre-activation and the only stash beside x; y = z sigma(z) with the training recurrence's sigma.
 * xb_conv_train_backward_dev: dz = dy (sigma(z) (1 + z (1 - sigma(z)))); db[co] = sum dz; dw[co, ci, k] = sum dz[b, co, t]
 *   x[b, ci, t stride + k - K / 2]; dx[b, ci, s] = sum_co sum_k dz[b, co, t] w[co, ci, k] over t stride + k - K / 2 = s.
 *   d_dx = NULL: not wanted (conv1); dw and db are the same bytes either way.
 * Two routes, and THE RULE that chooses reads the shape alone (csrc/xb_conv_plan.h): stride 1, at most 16 channels on either
 *   side and Cin K <= 64 is narrow, everything else wide.
 *   Narrow (conv1 1 -> 4, conv2 4 -> 16, K = 5): direct kernels.  A workgroup stages its 256 positions of x with their halo and all
 *   weights in LDS, a thread produces all Cout channels of its position, accesses run along L.  A sum of z runs over ci
 *   ascending, k ascending (one fma each), the bias last; dx is a gather over co ascending, k ascending.  dw and db: every
 *   workgroup sums its own 256 positions in float64 -- four runs of 64 in ascending order, added as (0 + 1) + (2 + 3) -- and
 *   writes one partial per element to scratch; a second kernel adds the workgroups' partials in ascending order in float64 and
 *   rounds once.  The number of workgroups is n ceil(max(Lin, Lout) / 256).
 *   Wide (conv3 16 -> F, K = 19, stride 5): an im2col writes col (Lout n, Cin K), row t n + b, column ci K + k, so that w as
 *   (Cout, Cin K) is xb_linear_f32's weight operand as it lies.  z = xb_linear_f32(col, w, b), then the swish.  Backward: dz,
 *   then dw, db = xb_wgrad_f32(dz, col), dcol = xb_linear_f32(dz, w^T) with w^T from xb_transpose_f32, and a gather col2im: a dx
 *   element adds its at most ceil(K / stride) terms of dcol in ascending k.  The backward recomputes col from x.  dz, col, dcol
 *   and w^T (Lout n (Cout + 2 Cin K) + Cin K Cout floats) live in a workspace of the context that grows with the calls.
 * No floating-point atomics; a repeated call gives the same bytes; a chunk's z, y and dx do not depend on which other chunks are
 *   in the call; zeros are written as +0.  Accepted: n, Cin, Cout, K, stride, Lin >= 1 with Cin K <= 4096 (Lout >= 1 follows),
 *   every tensor of the call, col included, below 2^38 elements; anything else, a null pointer (but d_dx) or one that is not
 *   16-byte aligned is XB_ERR_INVALID with the figures, before anything is launched.  No weights need to be loaded.  The calls
 *   return without waiting; the outputs are ordered on xb_result_stream.  Measured error and time: DESIGN.md 4.2.9.
 *
 * xb_full_train_begin(params): the trainer of xb_top_train_begin at L = 5 with the three convolutions trained as well.  params is
 *   ONE flat array in state-dict order: encoder.0.conv.weight (4, 1, 5), .bias (4), encoder.1.conv.weight (16, 4, 5), .bias (16),
 *   encoder.2.conv.weight (F, 16, W), .bias (F) -- 360 + F (16 W + 1) floats (csrc/xb_conv_plan.h) -- then the 4 * 5 + 2 tensors
 *   of xb_top_train_begin.  xb_top_train_grad, xb_top_train_step, xb_top_get_weights and xb_top_train_end serve this trainer too,
 *   on the whole flat array.  A gradient is the chain of xb_top_train_grad with
 *     the three xb_conv_train_forward in place of xb_encode_bottom -- conv1 on the signal as (n, 1, chunk_len), conv3 with tnc = 1
 *     writing x0 -- and, behind the lowest LSTM layer's backward, dy = xb_linear_f32(dgin, W_ih^T) for that layer too, then the
 *     three xb_conv_train_backward (conv3 with tnc = 1, conv1 with dx = NULL);  ONE xb_grad_norm over the whole flat g,
 *   byte for byte what the public entry points give when chained (tests/test_gpu_fulltrain.py), and the step ONE AdamW over all
 *   28 tensors.  The inference bottom never runs, so the context's precision is free; the other refusals are those of
 *   xb_top_train_begin (XB_ERR_STATE while any trainer is open on the context).
 */
XB_API int xb_conv_train_forward_dev(xb_ctx *ctx, const float *d_x, const float *d_w, const float *d_b, int n, int Cin, int Lin, int Cout,
                                     int K, int stride, int tnc, float *d_z, float *d_y);
XB_API int xb_conv_train_backward_dev(xb_ctx *ctx, const float *d_dy, const float *d_x, const float *d_z, const float *d_w, int n, int Cin,
                                      int Lin, int Cout, int K, int stride, int tnc, float *d_dx /* NULL: not wanted */, float *d_dw,
                                      float *d_db);
XB_API int xb_full_train_begin(xb_ctx *ctx, const float *params);

/* compute_scores (crf/basecall.py:27-82), viterbi branch: encode + decode without materialising
 * the blank column or copying scores off the device. */
XB_API int xb_basecall_chunks(xb_ctx *ctx, const float *signal, int n, const char *alphabet,
                              int8_t *seq, int32_t *seq_len);
XB_API int xb_basecall_chunks_dev(xb_ctx *ctx, const float *d_signal, int n, const char *alphabet,
                                  int8_t *d_seq, int32_t *d_seq_len);
/* ... with the qualities and moves of xb_decode_q (moves may be NULL). */
XB_API int xb_basecall_chunks_q(xb_ctx *ctx, const float *signal, int n, const char *alphabet, float qscale, float qoffset,
                                int8_t *seq, int8_t *qstring, uint8_t *moves, int32_t *seq_len);
/* ... with the qualities, moves and letter probabilities of xb_decode_ub (moves may be NULL; probs (n, nb, T)). */
XB_API int xb_basecall_chunks_ub(xb_ctx *ctx, const float *signal, int n, const char *alphabet, float qscale, float qoffset,
                                 int8_t *seq, int8_t *qstring, uint8_t *moves, uint8_t *probs, int32_t *seq_len);
/* Opt in to the co-scheduling of two calls in flight (see the header comment) and make room for it: the workspaces for
 * max_batch chunks are replaced by twice that -- which waits for everything in flight and takes a second or two, so callers
 * do it once, up front (bench.py: outside its timed region; Model: when the host pipeline starts).  XB_OK also when the
 * context cannot pair calls (XB_FUSE=0, max_batch > 512, serial schedule): xb_pairing_active tells (1: asynchronous calls
 * may be held back for a partner from now on; 0: every call is enqueued before it returns).  XB_ERR_NOMEM: no room for a
 * pair -- the context carries on unpaired.  No counterpart in the reference (single batch in flight, crf/basecall.py:109-111). */
XB_API int xb_reserve_pairing(xb_ctx *ctx);
XB_API int xb_pairing_active(const xb_ctx *ctx);

/*
 * The same operator for a host pipeline that keeps the device busy (crf/basecall.py:96-119: the reference overlaps its
 * stages with threads and bounded queues; here the overlap is two batches in flight on the device).
 * xb_submit_chunks copies `signal` (n, L) into pinned staging of `slot` (0 .. XB_PIPELINE_SLOTS - 1), enqueues H2D on a
 * copy stream, the fused encode + decode, and the D2H of the results into pinned staging, and returns without waiting.
 * xb_collect_chunks waits for that slot's batch only and copies seq (n, T) / seq_len (n) out.  Typical use: submit
 * batch k+1 into the next slot, then collect batch k -- results arrive one batch late, in order; with co-scheduled pairs
 * (xb_reserve_pairing) rotate all four slots -- submit batch k+3, then collect batch k -- so that pair (k+2, k+3) is on the
 * device before the host waits for pair (k, k+1).
 * A slot must be collected before it is submitted again (XB_ERR_STATE otherwise).
 */
#define XB_PIPELINE_SLOTS 4
XB_API int xb_submit_chunks(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet);
XB_API int xb_collect_chunks(xb_ctx *ctx, int slot, int8_t *seq, int32_t *seq_len);
/* The pipeline with the qualities and moves of xb_decode_q (_q) and with those and the letter probabilities of xb_decode_ub
 * (_ub): a slot's pinned staging for them is allocated by its first such submission.  A collect takes a submission of its
 * own kind or a richer one (XB_ERR_STATE otherwise; moves may be NULL): xb_collect_chunks_q of a _ub submission returns its
 * qualities, xb_collect_chunks of a _q or _ub submission its bases alone.  Co-scheduling (xb_reserve_pairing): a call pairs
 * only with a call of its own kind and, for _q / _ub, the same qscale / qoffset -- a held call that finds no such partner
 * runs on its own, so every call produces exactly the bytes it produces unpaired. */
XB_API int xb_submit_chunks_q(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet, float qscale,
                              float qoffset);
XB_API int xb_collect_chunks_q(xb_ctx *ctx, int slot, int8_t *seq, int32_t *seq_len, int8_t *qstring, uint8_t *moves);
XB_API int xb_submit_chunks_ub(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet, float qscale,
                               float qoffset);
XB_API int xb_collect_chunks_ub(xb_ctx *ctx, int slot, int8_t *seq, int32_t *seq_len, int8_t *qstring, uint8_t *moves,
                                uint8_t *probs);

XB_API int xb_synchronize(xb_ctx *ctx);

/*
 * The HIP stream (a hipStream_t, returned as void *) on which the outputs of the most recent *_dev call are produced.
 * A caller that consumes d_seq / d_seq_len on a stream of its own without a host-side xb_synchronize records an event
 * on this stream right after the call and waits for it there; before the same output buffers are handed to a later
 * call it makes this stream wait for its own "consumed" event.  This is how the gather of called sequences
 * (RCCL all_gather on a side stream) overlaps the next batch; the reference, single-device Python, has no
 * counterpart.
 */
XB_API void *xb_result_stream(xb_ctx *ctx);

/* ---- multi-GPU: the gather of called sequences --------------------------------------------------
 *
 * Reads shard over the GPUs of a node, one process and one xb_ctx per GPU, with no data-path collective; the only exchange
 * is this gather of the packed sequences (RCCL over xGMI; librccl is opened at run time).  The reference is single-device
 * Python and has no counterpart.
 *   xb_comm_unique_id   rank 0 draws the 128-byte id (ncclGetUniqueId) and hands it to the other ranks out of band (the
 *                       launcher's rendezvous: xna_basecaller_amd/dist.py exchanges it over a socket on MASTER_ADDR);
 *   xb_comm_create      every rank joins (ncclCommInitRank) on its device; collective: returns when all `world` ranks have;
 *   xb_gather_called    all-gather of one batch: d_seq (n, T) int8 / d_seq_len (n) int32 of this rank into
 *                       d_all_seq (world, n, T) / d_all_len (world, n) on every rank, enqueued on the communicator's own stream
 *                       behind xb_result_stream(ctx) (ctx may be NULL when the caller has synchronised) -- returns at once;
 *                       every rank passes the same n and T;
 *   xb_comm_fence       makes the streams of ctx wait (on the device) for the gather issued `lag` calls ago (0: the latest, 1: the
 *                       one before it) and everything older -- call it before output buffers a gather still reads are handed
 *                       to a later xb_basecall_chunks_dev (two buffer sets in rotation: lag 1 right before enqueueing a batch);
 *   xb_comm_synchronize host-side completion of the gathers asked for so far (one still waiting for a held-back basecall is
 *                       launched first).
 */
#define XB_COMM_ID_BYTES 128
typedef struct xb_comm xb_comm;
XB_API int xb_comm_unique_id(char id[XB_COMM_ID_BYTES]);
XB_API int xb_comm_create(xb_comm **out, int device, int rank, int world, const char id[XB_COMM_ID_BYTES]);
/* xb_comm_destroy: DESTROY ORDER -- the communicator first or the contexts first, both are safe, under one rule: every
 * context it gathered for and every buffer handed to xb_gather_called must still be alive when xb_comm_destroy is called if a
 * gather is still waiting for a held-back basecall of that context (see the header comment on co-scheduling).
 * xb_comm_destroy and xb_comm_synchronize launch such a basecall themselves (as xb_result_stream(ctx) would) and wait for
 * its gather, so no deferred gather outlives its communicator; after xb_comm_destroy the context holds no reference to it.
 * Destroying the context first launches the held call too (xb_ctx_destroy), with the communicator still alive.  What is NOT
 * allowed: freeing d_seq / d_seq_len / d_all_* of a batch before xb_synchronize(ctx) (or xb_comm_synchronize for the
 * gathered rows) has returned -- a held call writes them when it is launched. */
XB_API void xb_comm_destroy(xb_comm *comm);
XB_API int xb_comm_rank(const xb_comm *comm);
XB_API int xb_comm_world(const xb_comm *comm);
XB_API const char *xb_comm_last_error(const xb_comm *comm);
XB_API int xb_gather_called(xb_comm *comm, xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int T,
                            int8_t *d_all_seq, int32_t *d_all_len);
XB_API int xb_comm_fence(xb_comm *comm, xb_ctx *ctx, int lag);
XB_API int xb_comm_synchronize(xb_comm *comm);
/* Makes every stream of ctx wait for `hip_event` (a hipEvent_t passed as void *) -- the edge xb_comm_fence uses. */
XB_API int xb_stream_wait_event(xb_ctx *ctx, void *hip_event);

/* ---- host-side scoring used by `bonito evaluate` -----------------------------------------------------------------
 * util.accuracy(ref, seq, balanced, min_coverage) (util.py:402-424): Smith-Waterman local alignment of the called sequence
 * against its reference (gap open 8 / extend 4, match +5 / mismatch -4) and '=' / ('=' + 'I' + 'X' + 'D') * 100 from its trace
 * (balanced: ('=' - 'I') / ('=' + 'X' + 'D')); 0 when less than min_coverage of the reference is aligned.  A restatement of
 * the parasail call the reference makes (parasail is in no image): see csrc/xb_align.hip for the two stated choices.  Pure host
 * code, no context needed.  counts (optional) receives the numbers of '=', 'X', 'I', 'D' columns.
 */
XB_API int xb_align_accuracy(const char *ref, int ref_len, const char *seq, int seq_len, double min_coverage, int balanced,
                             double *accuracy, int32_t counts[4]);

/* ---- mapping calls to a template library (an extension: `basecaller --reference`) ----------------------------------
 * The reference maps its calls with minimap2 through mappy (bonito/aligner.py:12-16), a genome aligner no image here has.
 * XNA experiments map reads to a small TEMPLATE LIBRARY (tens to a thousand templates of about a hundred letters, reads about
 * as long), and at that size the device aligns every row against every template on both strands exhaustively: no seeding,
 * no chaining, optimal under its scoring.  minimap2 is absent, so there is nothing to pin it to: PARITY UNPINNED; the
 * contract below is this library's own and the kernels are bit-exact against a CPU restatement of it (tests/map_ref.py).
 *   letters    A C G T in either case are codes 0..3; every other byte (N, X, Y, ..) is code 4, "ambiguous", in the rows and in
 *              the templates alike (minimap2's own table).  The reverse strand aligns the reverse complement of the row's
 *              CODES (0 <-> 3, 1 <-> 2, 4 stays 4) to the template as it is.
 *   score      local (Smith-Waterman) alignment, one affine gap piece, int32 arithmetic: a column of equal codes below 4 scores
 *              +match, of different codes -mismatch, a column with a code 4 on either side -ambiguous (and counts as a
 *              mismatch column); a gap of k letters costs gap_open + k * gap_extend (minimap2's convention; xb_align_accuracy
 *              below follows parasail's open + (k - 1) * extend).  minimap2's map-ont first piece is 2 / 4 / 4 / 2 / 1.  All
 *              five are >= 0 and <= 1000.
 *   winner     of a row: the maximum score over (template t, strand, end cell (i, j)); ties go to the lowest t, then + before
 *              -, then the first cell in row-major order (row position i on the aligned strand, then template column j).  No
 *              positive score anywhere: unmapped.
 *   trace      back from the winning cell to the first cell of score 0; among equal predecessors the diagonal, then a deletion
 *              (a template letter with nothing opposite), then an insertion; a gap that can equally be opened or extended at a
 *              cell is opened there.
 *   second     the best score over all OTHER templates (either strand), 0 when there is none.  The callers' mapping quality is
 *              clamp((int)(60 * (1 - second / score)), 0, 60) -- NOT minimap2's formula, which needs chain scores; libraries whose
 *              templates share their flanks therefore report low to middling values.
 * Arguments: seq (n, W) int8 rows, left-packed as xb_decode writes them, seq_len (n) (a length outside [0, W] is clamped);
 * templates: the library's letters concatenated, offsets (R + 1) into them (offsets[0] = 0), both HOST pointers in both
 * forms -- the library's device image is kept by the context and rebuilt only when the bytes change.  Outputs, (n) each:
 * tmpl int32 (-1 unmapped), strand int8 (+1, -1; 0 unmapped), score, second, q_st, q_en (half-open, positions in the row ON THE
 * ALIGNED STRAND: for strand -1 in its reverse complement -- mappy's original-strand pair is (len - q_en, len - q_st)), r_st,
 * r_en (half-open, in the template), n_ops, and ops (n, W + Lmax) uint8, Lmax = the longest template: one byte per alignment
 * column in template order, '=' 'X' 'I' (row letter with nothing opposite) 'D', zero-filled behind n_ops.  Unmapped rows: all
 * zeros beside tmpl.
 * Limits: W <= 4096, templates of 1 .. 4096 letters, a library of at most 2^20 letters, and 2 n W sum(L) <= 1.2e11 cells a call
 * (XB_ERR_INVALID with the figures otherwise; the context stays usable).  Two launches on the main stream: a score pass over
 * every (row, template, strand) that keeps its anti-diagonals in registers and leaves one 24-byte record per (row, 16 KB of
 * templates), and a trace pass over the winners.  The _dev form returns without waiting (xb_synchronize).
 */
XB_API int xb_map_templates(xb_ctx *ctx, const int8_t *seq, const int32_t *seq_len, int n, int W, const char *templates,
                            const int32_t *offsets, int R, int match, int mismatch, int gap_open, int gap_extend, int ambiguous,
                            int32_t *tmpl, int8_t *strand, int32_t *score, int32_t *second, int32_t *q_st, int32_t *q_en,
                            int32_t *r_st, int32_t *r_en, uint8_t *ops, int32_t *n_ops);
XB_API int xb_map_templates_dev(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int W, const char *templates,
                                const int32_t *offsets, int R, int match, int mismatch, int gap_open, int gap_extend, int ambiguous,
                                int32_t *d_tmpl, int8_t *d_strand, int32_t *d_score, int32_t *d_second, int32_t *d_q_st,
                                int32_t *d_q_en, int32_t *d_r_st, int32_t *d_r_en, uint8_t *d_ops, int32_t *d_n_ops);

/* ---- ctc-data labels of mapped rows (`basecaller --save-ctc`) -------------------------------------------------------------
 * The reference's CTCWriter (bonito/io.py:448-585) decides per chunk, on the host and from a minimap2 mapping, whether the chunk
 * becomes training data, and cuts its label row from the reference.  Here the mapping is xb_map_templates' (above), so there
 * is nothing to pin the whole to: PARITY UNPINNED; the contract below restates io.py:495-540 over the mapper's outputs and the
 * kernel is bit-exact against a CPU restatement of it (tests/savectc_ref.py).
 *   inputs     per row seq_len (clamped to [0, W] as the mapper clamps it) and the mapper's tmpl, strand, q_st, q_en, r_st, r_en,
 *              ops (n, W + Lmax), n_ops; the library as xb_map_templates takes it (HOST pointers; the context's cached device
 *              image is reused).  n_ops is clamped to [0, W + Lmax], r_st / r_en to 0 <= r_st <= r_en <= the template's length.
 *   mlen       the number of '=' bytes among the row's first n_ops columns; blen = n_ops.  Written for every row.
 *   verdict    one byte, 0 = the chunk is kept:
 *                bit 0 FAILED_SEQ      seq_len == 0
 *                bit 1 FAILED_MAP      tmpl < 0 (or not below R); the mapper leaves an empty row unmapped, so such a row carries
 *                                      bits 0 and 1, as the reference counts both.  With bit 0 or 1 nothing else is looked at.
 *                bit 2 SKIPPED_NON_UB  ub_only != 0 and template[r_st:r_en] holds no letter outside ACGTacgt; nothing else is
 *                                      looked at (io.py:508-510 continues before the thresholds)
 *                bit 3 FAILED_ACC      (double)mlen / (double)blen < min_accuracy (blen == 0, which the mapper never reports for a
 *                                      mapped row, fails too)
 *                bit 4 FAILED_COV      (double)(q_en - q_st) / (double)seq_len < min_coverage
 *              Bits 3 and 4 may be set together.  Both quotients are IEEE float64, one correctly rounded division each, compared
 *              as Python compares them: 19 / 20 against 0.95 decides on the device as it does in the reference.
 *   target     for a row of verdict 0: template[r_st:r_en], on strand -1 reversed with A <-> T and C <-> G (any other letter
 *              stays), then A C G T (either case) -> 1 2 3 4 and EVERY other byte -> ub_plus on strand +1, ub_minus on strand -1
 *              (the reference maps 'N' alone, to its X = 5 and Y = 6; every non-ACGT byte is treated as it treats 'N' -- the
 *              mapper's own letter contract).  target is (n, TW) uint8 with TW = Lmax rounded up to a multiple of 16, 16-byte
 *              aligned, zero-filled behind target_len; target_len = r_en - r_st.  Rows of any other verdict: all zeros, length 0.
 * ub_plus and ub_minus lie in 1 .. 255; the thresholds must not be NaN.  One launch on the main stream, one wavefront per row;
 * not a stage of xb_get_stage_times (nor is the mapper).  The _dev form takes device pointers for the rows and the outputs and
 * returns without waiting (xb_synchronize).
 * xb_ctc_chunks is the fused form for the Viterbi decode: signal (n, chunk_len) fp32 on the HOST -> the basecall
 * (xb_basecall_chunks_dev), the mapper over its left-packed device rows (W = the model's time steps T, in as many launches as the
 * mapper's cell budget asks for) and the labels, on device buffers with one synchronisation at the end; it returns seq (n, T),
 * seq_len, every output of xb_map_templates and the five above, exactly what the three host-form calls return one after the
 * other.
 */
XB_API int xb_ctc_targets(xb_ctx *ctx, const int32_t *seq_len, int n, int W, const char *templates, const int32_t *offsets, int R,
                          const int32_t *tmpl, const int8_t *strand, const int32_t *q_st, const int32_t *q_en, const int32_t *r_st,
                          const int32_t *r_en, const uint8_t *ops, const int32_t *n_ops, double min_accuracy, double min_coverage,
                          int ub_only, int ub_plus, int ub_minus, int32_t *mlen, int32_t *blen, uint8_t *verdict, uint8_t *target,
                          int32_t *target_len);
XB_API int xb_ctc_targets_dev(xb_ctx *ctx, const int32_t *d_seq_len, int n, int W, const char *templates, const int32_t *offsets,
                              int R, const int32_t *d_tmpl, const int8_t *d_strand, const int32_t *d_q_st, const int32_t *d_q_en,
                              const int32_t *d_r_st, const int32_t *d_r_en, const uint8_t *d_ops, const int32_t *d_n_ops,
                              double min_accuracy, double min_coverage, int ub_only, int ub_plus, int ub_minus, int32_t *d_mlen,
                              int32_t *d_blen, uint8_t *d_verdict, uint8_t *d_target, int32_t *d_target_len);
XB_API int xb_ctc_chunks(xb_ctx *ctx, const float *signal, int n, const char *alphabet, const char *templates, const int32_t *offsets,
                         int R, int match, int mismatch, int gap_open, int gap_extend, int ambiguous, double min_accuracy,
                         double min_coverage, int ub_only, int ub_plus, int ub_minus, int8_t *seq, int32_t *seq_len, int32_t *tmpl,
                         int8_t *strand, int32_t *score, int32_t *second, int32_t *q_st, int32_t *q_en, int32_t *r_st, int32_t *r_en,
                         uint8_t *ops, int32_t *n_ops, int32_t *mlen, int32_t *blen, uint8_t *verdict, uint8_t *target,
                         int32_t *target_len);

/* ---- per-position UB accuracy of mapped rows (`basecaller --ub-report`, `analyze`) ----------------------------------------
 * The third stage of the reference's evaluation (eval_model.sh:91-177) is src/tools/analyze_paf.py -p over minimap2's PAF:
 * Python loops per read (utils.py:112-191 compute_read_matches, :661-725 polish_target_matches, :727-924 the errors and the
 * UB-area metrics, analyze_paf.py:520-536 the confusion matrix).  Here the mapping is xb_map_templates', so there is nothing to
 * pin the whole to: PARITY UNPINNED; the contract below restates those loops over the mapper's outputs and the kernel is
 * equal, integer for integer, to a CPU restatement of it (tests/ubtally_ref.py).
 *   inputs     the rows the mapper saw: seq (n, W) int8 ASCII, left-packed, and seq_len (clamped to [0, W]); the mapper's tmpl,
 *              strand, q_st, r_st, r_en, ops (n, W + Lmax), n_ops; the library as xb_map_templates takes it (HOST pointers; the
 *              context's cached device image is reused).  n_ops is clamped to [0, W + Lmax], r_st / r_en to 0 <= r_st <= r_en <=
 *              L (L = the template's length), q_st to [0, seq_len].  A row whose tmpl lies outside [0, R) is unmapped: its counts
 *              are zero and it adds nothing to the accumulators.  strand < 0 is the reverse strand, anything else the forward.
 *   target     T[j], j in [0, L): the template letter in upper case when it is one of A C G T, 'X' otherwise -- every non-ACGT
 *              byte is a UB site (the mapper's letter contract; the reference replaces 'N' alone).
 *   query      Q[i] on the aligned strand: strand +1 the row with a-z in upper case; strand -1 that row reversed, with A <-> T,
 *              C <-> G and X <-> Y (utils.py:26-31), every other byte unchanged.  NOT the mapper's own reverse strand, which
 *              complements codes and leaves X and Y what they are: there both are "ambiguous" either way, here a called X on
 *              the reverse strand is a Y of the template's strand.
 *   called     C[0 .. L), all '-' to start with; the columns ops[0 .. n_ops) are walked from ri = r_st, qi = q_st: '=' or 'X':
 *              C[ri] = Q[qi], both advance; 'I': qi advances; 'D': ri advances.  A column that needs a row letter when qi has
 *              reached seq_len, or a template position when ri has reached r_en, or that holds any other byte, ends the walk.
 *   polish     P = a copy of C, then for every UB site u (T[u] == 'X') in ascending order -- the conditions read C, the letter
 *              that moves is read from P, as the reference does:
 *                (a) C[u] == 'X': nothing;
 *                (b) C[u] == '-': with lo .. hi the run of '-' in C that contains u: if lo > 0 and C[lo-1] == 'X', P[lo-1] = '-'
 *                    and P[u] = 'X'; else if hi < L-1 and C[hi+1] == 'X', P[hi+1] = '-' and P[u] = 'X';
 *                (c) else if 1 <= u < L-1, C[u-1] == '-' and C[u+1] == 'X': P[u-1] = P[u], P[u] = 'X', P[u+1] = '-';
 *                (d) else if 1 <= u < L-1, C[u+1] == '-' and C[u-1] == 'X': P[u+1] = P[u], P[u] = 'X', P[u-1] = '-'.
 *              Where the reference's indices run off an end (Python wraps around or raises) the branch does not apply.
 *   errors     e[j] = (P[j] != T[j]) for every j in [0, L); positions outside [r_st, r_en) are '-' and count as errors.
 *   masks      ub[j] = (T[j] == 'X'); area[j] = not ub[j] and some UB site u has |j - u| <= 5 (clipped to [0, L)).
 *   counts     (n, 8) int32 per row: n_match = L - sum(e), ub_matches, ub_len, ub_area_matches, ub_area_len, non_ub_area_matches,
 *              non_ub_area_len (neither ub nor area), ubs_detected = the number of j with P[j] in {X, Y}.
 * Accumulators -- the call ADDS to them, the caller zeroes them:
 *   reads      (R, 2) int32: rows per (template, strand); strand index 0 is +, 1 is -.
 *   err        (2, sum(L)) int32: err[s][offsets[t] + p] += e[j] with p = j on +, p = L-1-j on - (errors[::-1], utils.py:764-765).
 *   cm         (6, 7) int64: rows = the target letter in the order A T C G X Y, columns = the called letter A T C G X Y '-', over
 *              every j: on + the pair (T[j], P[j]), on - the pair after complementing both with the X <-> Y table (a UB site is
 *              row Y there); a called byte outside the seven is not counted.
 * Everything is an integer, so the result does not depend on the order of the additions.  Limits: the mapper's -- W <= 4096,
 * templates of 1 .. 4096 letters, a library of at most 2^20 letters (XB_ERR_INVALID with the figures otherwise; the context
 * stays usable).  One launch on the main stream, one wavefront per row, T, C and P in LDS; not a stage of xb_get_stage_times.
 * The _dev form takes device pointers for the rows, the mapper's outputs, counts and the accumulators and returns without
 * waiting (xb_synchronize); the host form uploads, runs, waits and copies back -- the accumulators come back as they went in
 * plus this call's additions.
 */
XB_API int xb_ub_tally(xb_ctx *ctx, const int8_t *seq, const int32_t *seq_len, int n, int W, const char *templates,
                       const int32_t *offsets, int R, const int32_t *tmpl, const int8_t *strand, const int32_t *q_st,
                       const int32_t *r_st, const int32_t *r_en, const uint8_t *ops, const int32_t *n_ops, int32_t *counts,
                       int32_t *reads, int32_t *err, int64_t *cm);
XB_API int xb_ub_tally_dev(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int W, const char *templates,
                           const int32_t *offsets, int R, const int32_t *d_tmpl, const int8_t *d_strand, const int32_t *d_q_st,
                           const int32_t *d_r_st, const int32_t *d_r_en, const uint8_t *d_ops, const int32_t *d_n_ops,
                           int32_t *d_counts, int32_t *d_reads, int32_t *d_err, int64_t *d_cm);

/* ---- barcode distance of mapped rows (`basecaller --ub-report --max-bc-dist`, `analyze -d`) ---------------------------------
 * The templates of an XNA library share their primers and differ in a barcode; the reference's analyze_paf.py -d N keeps a PAF
 * row only when the read carries the barcode of the template it was mapped to, at an edit distance of at most N
 * (utils.py:1387-1434 get_barcode_match_score per row, analyze_paf.py:623-643 the filter).  Here the mapping is
 * xb_map_templates': PARITY UNPINNED for the mapping, the per-row function pinned by tests/golden/bcdist.json (what the
 * reference's own function returned); the kernel is equal, integer for integer, to a CPU restatement of the contract below
 * (tests/bcdist_ref.py).
 *   inputs     the rows the mapper saw: seq (n, W) int8 ASCII, left-packed, and seq_len (clamped to [0, W]); the mapper's tmpl,
 *              strand, q_st, r_st; the library as xb_map_templates takes it (HOST pointers; the context's cached device image is
 *              reused).  q_st is clamped to [0, seq_len], r_st to [0, L] (L = the template's length).  strand < 0 is the reverse
 *              strand, anything else the forward.  bc_pos: where the barcode starts in every template (the reference's
 *              left_primer_len), bc_len its length, relax the windows tried to either side (n_relax_bases); the reference's
 *              values are 25 / 24 / 3 (POC) and 23 / 30 / 3 (CPLX).
 *   barcode    B = template[bc_pos : bc_pos + bc_len], clipped to the template (short, or empty when bc_pos >= L), a-z in upper
 *              case, every other byte as it is -- the LETTERS, not the mapper's codes: an 'N' of the template equals an 'N' only.
 *   query      Q[i] on the aligned strand, exactly xb_ub_tally's Q: upper case; on strand -1 the row reversed with A <-> T,
 *              C <-> G and X <-> Y (utils.py:26-31), every other byte unchanged.
 *   start      max(q_st + bc_pos - r_st, 0): the two branches of utils.py:1400-1404 in the mapper's own coordinates.
 *   windows    i = max(start - relax, 0) .. start + relax in ascending order; obs = Q[i : min(i + bc_len, seq_len)], empty when
 *              i >= seq_len (Python's slice); d = the unit-cost Levenshtein distance of B and obs, bytes compared as they are;
 *              the first strictly smaller d wins.
 *   outputs    (n) int32 each: bc_dist = the winning d, bc_start = its i, bc_end = i + bc_len (NOT clipped, as the reference
 *              reports it), bc_obs_len = len(obs).  A row whose tmpl lies outside [0, R) is unmapped: bc_dist = -1, zeros
 *              elsewhere.
 * Everything is an integer.  Limits: 0 <= bc_pos <= 2^30, 1 <= bc_len <= 64, 0 <= relax <= 8, and the mapper's -- W <= 4096,
 * templates of 1 .. 4096 letters, a library of at most 2^20 letters (XB_ERR_INVALID with the figures otherwise; the context
 * stays usable).  One launch on the main stream, one wavefront per row: B as one 64-bit word per query letter (which barcode
 * positions it matches), a lane per window running the bit-vector recurrence of the global distance, the windows side by
 * side; no scratch, no atomics; not a stage of xb_get_stage_times.  The _dev form takes device pointers for the rows, the
 * mapper's outputs and the four outputs and returns without waiting (xb_synchronize); the host form uploads, runs, waits and
 * copies back.
 */
XB_API int xb_barcode_dist(xb_ctx *ctx, const int8_t *seq, const int32_t *seq_len, int n, int W, const char *templates,
                           const int32_t *offsets, int R, const int32_t *tmpl, const int8_t *strand, const int32_t *q_st,
                           const int32_t *r_st, int bc_pos, int bc_len, int relax, int32_t *bc_dist, int32_t *bc_start, int32_t *bc_end,
                           int32_t *bc_obs_len);
XB_API int xb_barcode_dist_dev(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int W, const char *templates,
                               const int32_t *offsets, int R, const int32_t *d_tmpl, const int8_t *d_strand, const int32_t *d_q_st,
                               const int32_t *d_r_st, int bc_pos, int bc_len, int relax, int32_t *d_bc_dist, int32_t *d_bc_start,
                               int32_t *d_bc_end, int32_t *d_bc_obs_len);

/* ---- DTW signal segmentation of ctc-data (an extension of the device path: `segment`) --------------------------------
 * The reference's src/tools/dtw_segmentation.py aligns every training chunk to the expected current levels of its reference
 * sequence with dtw-python (dtw(chunk, reference, step_pattern=my_asymmetric, window_type='slantedband'), :128-202) on the
 * host.  dtw-python is in no image, so there is nothing to pin it to: PARITY UNPINNED; the contract below is this library's
 * own restatement of that call and the kernel is bit-exact against a CPU restatement of it (tests/dtw_ref.py).
 *   problem    per chunk the query q[0..N) (the chunk's samples, converted exactly to float64) and the reference r[0..M),
 *              M = ref_rep * K: the chunk's K levels, each held for ref_rep consecutive columns (the kernel repeats them).
 *   cost       d(i, j) = |q[i] - r[j]| in float64.
 *   steps      every sample matches exactly one column and no column is skipped: g(0, 0) = d(0, 0);
 *              g(i, j) = d(i, j) + min(g(i-1, j), g(i-1, j-1)) -- ONE float64 addition per cell, in that order, no contraction;
 *              a cell with no finite predecessor is unreachable (+infinity), and so is g(0, j > 0).
 *   TIES       go to the stay step (i-1, j): the diagonal (i-1, j-1) replaces it only when it is STRICTLY smaller.  This is
 *              this library's statement of dtw-python's loop (pattern 1 first); with ref_rep > 1 neighbouring columns carry
 *              equal levels, so the rule decides real breakpoints.
 *   band       window[c] >= 0: cell (i, j) is allowed iff |j - i * M / N| <= window[c], evaluated in float64 as written (i * M
 *              exact, one division, one subtraction); the callers pass (N / K) * window_size (:160-161).  window[c] < 0, or
 *              window == NULL: every cell is allowed.  A cell that is not allowed is unreachable.
 *   end        (N-1, M-1).  Unreachable (always when M > N; possible under a narrow band): the chunk FAILS -- ok = 0,
 *              cost = +infinity, and the breakpoints are the naive ones of :186-191: N / K samples per base, the first N % K
 *              bases one more.
 *   trace      back from (N-1, M-1) along the recorded choices to (0, 0); reps[k] = the samples whose column j has
 *              j / ref_rep == k; breakpoints = cumsum(reps): breakpoints[K-1] == N, every base gets at least ref_rep samples.
 * Arguments: signal (n, N) fp32; levels: the chunks' float64 levels concatenated, BEFORE repetition; offsets (n + 1) int32 into
 * them (offsets[0] = 0), a HOST pointer in both forms (the library sizes its launches from it); window (n) float64 or NULL.
 * Outputs per chunk: breakpoints (n, Kmax) int32, zero-filled behind the chunk's K; ok (n) int8; cost (n) float64 = g(N-1, M-1).
 * Limits: 1 <= N <= 65535 (breakpoints.npy is uint16), 1 <= K, ref_rep * K <= 65535, Kmax >= every K (XB_ERR_INVALID with the
 * figures otherwise; the context stays usable).  One wave per chunk; a bit per feasible cell goes to a scratch buffer the
 * context owns, and a call is split into launches whose scratch stays under XB_DTW_SCRATCH_MB (default 1024) megabytes.
 * The _dev form returns without waiting (xb_synchronize).  xb_dtw_scratch_bytes: the choice-bit bytes the last call's
 * launches wrote, summed over its chunks (a measurement aid).
 */
XB_API int xb_dtw_segment(xb_ctx *ctx, const float *signal, int n, int N, const double *levels, const int32_t *offsets, int ref_rep,
                          const double *window, int Kmax, int32_t *breakpoints, int8_t *ok, double *cost);
XB_API int xb_dtw_segment_dev(xb_ctx *ctx, const float *d_signal, int n, int N, const double *d_levels, const int32_t *offsets,
                              int ref_rep, const double *d_window, int Kmax, int32_t *d_breakpoints, int8_t *d_ok, double *d_cost);
XB_API int64_t xb_dtw_scratch_bytes(const xb_ctx *ctx);

/* ---- XNA spliced augmentation of ctc-data (an extension of the device path: `splice`) ----------------------------------
 * The reference's ub-bonito/bonito/stitch_chunks.py (`bonito train -m per_kmer`) cuts the signal of the six k-mers around an
 * unnatural base out of XNA chunks and pastes it into DNA chunks, per read, in the data loader.  Here one wave per chunk does
 * it.  Everything but the random stream is pinned to the reference (tests/golden/splice.json); the DRAWS are this library's
 * own: parity unpinned.  The kernel is bit-exact against a CPU restatement of the contract (tests/splice_ref.py).
 *
 * xb_splice_library keeps the candidates of slice_xna(.., 'per_kmer') (:127-239) on the device until the next call or until
 * the context is destroyed (host pointers; the call waits):
 *   pool       pool_len float16 samples (their bit patterns): the kept windows of the XNA chunks, back to back.
 *   rows       (n_rows, 2) int32: pool offset and length (1 .. 100 samples) of every row, in the reference's order
 *              (ub, template, kmer_ub_pos, kmer, read_idx).
 *   table      (table_len, 2) int32, table_len = 2 * 7^5 * 6: first row and count of the group (ub, template, kmer_ub_pos) at
 *              index ((ub - 5) * 7^5 + t) * 6 + kmer_ub_pos, t = the template's five labels as base-7 digits, the first the
 *              most significant.  Grouped WITHOUT the k-mer, as the reference looks candidates up (:377): a group may hold
 *              rows of different k-mers.  count 0: no such group.
 *
 * xb_splice_chunks: signal (n, N) fp32, targets (n, Lt) labels 0 .. 6, lengths (n) int32, breakpoints (n, Lt) uint16 (the
 * sample where each base's signal ends; non-decreasing and at most N within a chunk's length).  A chunk's result depends only
 * on its data, the library, the parameters, `seed` and its GLOBAL index c = first_index + row -- never on the batch.
 *   draws      draw k of chunk c: z = mix(mix(seed + G (c + 1)) + G (k + 1)) in uint64, G = 0x9E3779B97F4A7C15, mix =
 *              splitmix64's finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB,
 *              z ^= z >> 31).  bounded(m) = ((z >> 32) * m) >> 32; unit = (z >> 11) * 2^-53.  k counts from 0 in the order
 *              below; a draw is spent exactly where the reference calls its generator (rng.choice(ubs) with one UB included).
 *   proportion var_prop > 0: prop = lo + (hi - lo) * unit with lo = prop - var_prop, hi = prop + var_prop, in float64 as
 *              written.  n_pos = max(rint(length * prop) - #existing UBs, 1), rint to even (Python's round of a float64).
 *   positions  choose_positions (:104-125): a base is valid unless it is among the first or last 10 or within 2 * pad of a
 *              label above 4.  Up to n_pos rounds; a round without a valid base ends them all; otherwise it takes
 *              valid[bounded(#valid)] and invalidates pos - pad .. pos + pad.  The positions are then handled in ascending order.
 *   per position (stitch_read_per_kmer, :349-446)  ub = ubs[bounded(#ubs)], ubs = the set bits of ubs_mask (1: X = 5, 2: Y = 6)
 *              in that order.  The six k-mers come from the ORIGINAL labels pos - 5 .. pos + 5 with the UB in the middle; k-mer
 *              i = 0 .. 5 looks up the group (ub, its five labels behind the UB followed by those in front of it, 5 - i).  A
 *              missing group abandons the position; the draws already spent stay spent.  cand_sample_size > 1: m =
 *              min(count, cand_sample_size) rows are sampled without replacement by a partial Fisher-Yates shuffle over the
 *              virtual identity permutation (draw j picks slot j + bounded(count - j)), and the first sampled row with the
 *              smallest |length - kmer_rep| is kept.  cand_sample_size = 1: the row bounded(count).
 *   resample   prepare_slice_chunk (:241-271), numpy's float64 arithmetic, no contraction.  The six rows have slice_len samples
 *              together, the signal they replace ins_len = breakpoints[pos] - breakpoints[pos - 6].  Stretch (slice_len <
 *              ins_len): xp as the reference builds it -- linspace (i * step + start, the last value the stop), .round() to
 *              even, astype(int) -- then numpy.interp: j = the largest with xp[j] <= x; xp[j] == x or j last: fp[j]; else
 *              slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]), y = slope * (x - xp[j]) + fp[j].  Shrink: the samples at
 *              linspace(0, slice_len - 1, slice_len - ins_len, dtype=int) are dropped.  Equal: a copy.
 *   outputs    the pasted values are the float16 pool values or the float64 interpolation, rounded ONCE to float32; the label
 *              at the position becomes ub; out_signal / out_targets are copies of the inputs elsewhere.  success (n) int8: at
 *              least one paste; inserted (n) int32: how many.
 * Limits: 1 <= N <= 65535, 1 <= Lt <= 65535, 1 <= cand_sample_size <= 32, pad >= 0, 0 <= prop, var_prop, prop + var_prop <= 1,
 * ubs_mask 1 .. 3, pool < 2^31 samples (XB_ERR_INVALID with the figures otherwise, before any launch; the context stays
 * usable); XB_ERR_STATE without a library.  Outputs must not alias inputs.  The host form checks lengths and breakpoints and
 * names the chunk; the _dev form (device pointers, returns without waiting: xb_synchronize) clamps them instead, so that no
 * access leaves the rows.
 */
XB_API int xb_splice_library(xb_ctx *ctx, const uint16_t *pool, int64_t pool_len, const int32_t *rows, int n_rows,
                             const int32_t *table, int table_len);
XB_API int xb_splice_chunks(xb_ctx *ctx, const float *signal, const uint8_t *targets, const int32_t *lengths,
                            const uint16_t *breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                            double prop, double var_prop, int cand_sample_size, int pad, float *out_signal, uint8_t *out_targets,
                            int8_t *success, int32_t *inserted);
XB_API int xb_splice_chunks_dev(xb_ctx *ctx, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
                                const uint16_t *d_breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                                double prop, double var_prop, int cand_sample_size, int pad, float *d_out_signal,
                                uint8_t *d_out_targets, int8_t *d_success, int32_t *d_inserted);

/* ---- XNA synthetic spiking of ctc-data (an extension of the device path: `spike`) ---------------------------------------
 * The reference's ub-bonito/bonito/spike_chunks.py (`bonito train --spike`, the default of its training recipe) replaces the
 * signal of the six k-mers around chosen bases of a DNA chunk with a synthetic squiggle drawn from a k-mer pore model and
 * normalised with the med / mad of the whole chunk's synthetic squiggle, per read, in the data loader.  Here one wave per
 * chunk does it.  Everything but the random stream restates spike_read (:247-297) with equal_kmer_reps=False, mix_ubs=True,
 * legacy_pos=False, fully_synth=False and is pinned to the reference (tests/golden/spike.json); the DRAWS are this library's
 * own: parity unpinned.  The kernel is bit-exact against a CPU restatement of the contract (tests/spike_ref.py).
 *
 * xb_spike_model keeps a k-mer table on the device until the next call or until the context is destroyed (host pointers; the
 * call waits): n = 7^6 level means and standard deviations; a k-mer is indexed by its six labels as base-7 digits, the first
 * letter the most significant (N A C G T X Y = 0 .. 6); mean = NaN: the model lacks the k-mer.  Other means must be finite,
 * their stdv finite and >= 0.
 *
 * xb_spike_chunks: signal, targets, lengths, breakpoints, n, N, Lt, first_index as xb_splice_chunks takes them.  A chunk's
 * result depends only on its data, the model, the parameters, `seed` and its GLOBAL index c = first_index + row.
 *   draws      z = mix(mix(mix(seed + G (c + 1)) + G (s + 1)) + G (k + 1)), with splice's mix, G, bounded(m) and unit: draw k of
 *              stream s of chunk c, so that a lane computes the index of its own draw.  s = 0: proportion, positions and the UB
 *              shuffle, k counting from 0 in that order, spent exactly where the reference calls its generator.  s = 1: the
 *              squiggle, k = the sample 0 .. 100 length - 1.  s = 2 + j: the j-th position in ascending order; k = 0 the shift
 *              choice, k = 1 the variable noise std, k = 2 + i the level noise of window sample i, k = 2 + len + i its added
 *              noise (len = the window's samples).
 *   proportion, n_pos, positions   as xb_splice_chunks (spike_chunks.py:194-215 = stitch_chunks.py:104-125).
 *   UBs        ubs_mask 1 = X, 2 = Y: every position gets it, no draw.  3 = both (:273-277): the list X, Y, X, Y, .. of
 *              m = n + n % 2 entries (n = the positions found) is shuffled from its end (i = m - 1 .. 1: j = bounded(i + 1), swap
 *              entries i and j), trimmed to n and zipped with the ascending positions.  0 = the reference's --ubs N: the DNA
 *              k-mers are re-synthesised and the labels stay.
 *   k-mers     a k-mer with a NaN mean among those named below ends the chunk before anything else: out_signal / out_targets
 *              are the inputs, spiked = 0, status = 2, mad = NaN and med = the table index of the first such k-mer (those of
 *              med / mad by base, then the windows' by position and k-mer).
 *   med, mad   (:44-52, :150-151) from the ORIGINAL labels: the k-mers of target[:length] + ATATA (TATAT when the last letter
 *              is A), one per base, each repeated 100 times; sample k = mean + (lo + (s - lo) * unit) with lo = -s, in float64
 *              as written.  med = (a + b) / 2.0 of the two middle order statistics of the 100 length values (-0 counted as +0);
 *              mad = the same median of |x - med|, * 1.4826 + 2^-23.  Exact selection, no floating-point accumulation.
 *   per position (:156-190)  the window is [breakpoints[pos - 6], breakpoints[pos]); k-mer i = 0 .. 5 covers its samples
 *              breakpoints[pos - 6 + i] .. breakpoints[pos - 5 + i] (none is allowed) and is letters i .. i + 5 of the ORIGINAL
 *              target[pos - 5 .. pos + 5] with the middle letter replaced by the UB (ubs_mask 0: not replaced).  Level noise of
 *              a sample with stdv s: dist_rows = 0 (`uniform`): lo + (s - lo) * unit, lo = -s.  dist_rows >= 1 (truncated
 *              normal): row r = bounded(dist_rows) of `phi` (the reference's shift choice; `truncnorm` is one row), p =
 *              phi[r][0] + unit * phi[r][1], noise = PPND16(p) * s.  phi is (dist_rows + 1, 2) float64 on the HOST in both
 *              forms: per shift value Phi(a) and Phi(b) - Phi(a) of the truncation a, b; the last row is the truncation of the
 *              added noise (-3, 3), read when noise_std > 0.  Added noise: sigma = noise_std, or 0.0 + (noise_std - 0.0) * unit
 *              with variable_noise; noise = PPND16(phi[dist_rows][0] + unit * phi[dist_rows][1]) * sigma.  The pasted value is
 *              ((mean + level) + noise - med) / mad -- without the noise term when noise_std = 0 -- rounded ONCE to float32; the
 *              label at pos becomes the UB.  Later windows overwrite earlier ones where they overlap (pad < 5).
 *   PPND16     Wichura's AS241 with the coefficients and the operation order of CPython's statistics._normal_dist_inv_cdf;
 *              its sqrt is the correctly rounded one, its log this library's own, from IEEE + - * / and bit operations only:
 *              x = m 2^e with m in [1, 2) from the bits; m > 1.4142135623730951: m = m * 0.5, e = e + 1; f = m - 1; s = f / (2 +
 *              f); z = s * s; q = Horner in z over 1/21, 1/19, .. 1/3 (q = q * z + c); t = (s * z) * q; logm = 2 * (s + t);
 *              log = e * 6.93147180369123816490e-01 + (logm + e * 1.90821492927058770002e-10).
 *   outputs    out_signal / out_targets are copies of the inputs elsewhere; spiked (n) int32: the positions pasted; med, mad
 *              (n) float64 (a chunk of length 0: 0, 0); status (n) int8: 0, or 2 (a k-mer is missing).
 * Limits: those of xb_splice_chunks for N, Lt, pad, prop, var_prop, first_index; ubs_mask 0 .. 3; 0 <= dist_rows <= 32; every
 * row read has 1e-300 <= phi[r][0], 0 < phi[r][1], phi[r][0] + phi[r][1] < 1; noise_std finite and >= 0 (XB_ERR_INVALID with
 * the figures otherwise, before any launch; the context stays usable); XB_ERR_STATE without a model.  Outputs must not alias
 * inputs.  The host form checks lengths and breakpoints and names the chunk; the _dev form (device pointers but for phi,
 * returns without waiting: xb_synchronize) clamps them instead, so that no access leaves the rows.
 */
XB_API int xb_spike_model(xb_ctx *ctx, const double *mean, const double *stdv, int64_t n);
XB_API int xb_spike_chunks(xb_ctx *ctx, const float *signal, const uint8_t *targets, const int32_t *lengths,
                           const uint16_t *breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                           double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                           int variable_noise, float *out_signal, uint8_t *out_targets, int32_t *spiked, double *med, double *mad,
                           int8_t *status);
XB_API int xb_spike_chunks_dev(xb_ctx *ctx, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
                               const uint16_t *d_breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                               double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                               int variable_noise, float *d_out_signal, uint8_t *d_out_targets, int32_t *d_spiked, double *d_med,
                               double *d_mad, int8_t *d_status);

/* ---- XNA fully synthetic chunks of ctc-data (an extension of the device path: `synth`) ------------------------------------
 * The reference's `bonito train --spike --fully_synth` (the -Z runs of its training recipe) does not paste windows: it throws
 * the chunk's signal away and synthesises all of it from the spiked labels and the breakpoints.  xb_synth_chunks restates
 * spike_read(..., fully_synth=True, equal_kmer_reps=False, mix_ubs=True, legacy_pos=False) -> sim_target -> sim_signals(append=
 * True) (spike_chunks.py:217-297) and is pinned to the reference (tests/golden/synth.json); the draws are this library's own:
 * parity unpinned.  The kernel is bit-exact against a CPU restatement of the contract (tests/synth_ref.py).  The arguments are
 * xb_spike_chunks', the model is the one xb_spike_model uploaded; mix, G, bounded, unit, the streams, PPND16 and its logarithm
 * are those of the section above.  What differs:
 *   draws      s = 0: proportion, positions and the UB shuffle, unchanged.  s = 1: the squiggle.  s = 2 serves the WHOLE chunk:
 *              k = 0 the shift choice, k = 1 the variable noise std, k = 2 + i the level noise of chunk sample i, k = 2 + total +
 *              i its added noise, total = min(breakpoints[length - 1], N).
 *   labels     positions and UBs are chosen as in xb_spike_chunks; the spiked row is the input row with the UB written at every
 *              position (ubs_mask 0: nothing is written, the chunk is re-synthesised DNA).
 *   k-mers     one per base i of the SPIKED row plus its tail (ATATA, or TATAT when the last letter is A).  The first base, in
 *              base order, whose k-mer has a NaN mean ends the chunk: out_signal / out_targets are the inputs, spiked = 0, status
 *              = 2, mad = NaN and med = that k-mer's table index.  The k-mers of the original row are never looked up.
 *   med, mad   as xb_spike_chunks (100 squiggle samples per base, exact selection, * 1.4826 + 2^-23), over the SPIKED row's
 *              k-mers (:223-224).
 *   samples    base b covers the samples breakpoints[b - 1] .. breakpoints[b] - 1 (breakpoints[-1] = 0); a base with no sample
 *              draws nothing.  Sample i < total becomes ((mean + level) [+ noise] - med) / mad of its base's k-mer, rounded ONCE
 *              to float32; level and noise exactly as in xb_spike_chunks (uniform, or PPND16(phi[r][0] + unit * phi[r][1]) * s),
 *              r and sigma drawn once per chunk.  Samples i >= total keep the input's value (the reference returns a shorter
 *              array there).
 *   outputs    spiked: the number of positions; it may be 0 (no base was free) with the chunk still synthesised.  A chunk of
 *              length 0: the inputs, spiked = med = mad = status = 0.
 * Limits, messages (under the name xb_synth_chunks), XB_ERR_STATE without a model and the host / _dev conventions are those of
 * xb_spike_chunks.  The _dev form clamps lengths, labels and breakpoints so that no access leaves the rows whatever they hold;
 * the values of rows the host form would refuse are unspecified.
 */
XB_API int xb_synth_chunks(xb_ctx *ctx, const float *signal, const uint8_t *targets, const int32_t *lengths,
                           const uint16_t *breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                           double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                           int variable_noise, float *out_signal, uint8_t *out_targets, int32_t *spiked, double *med, double *mad,
                           int8_t *status);
XB_API int xb_synth_chunks_dev(xb_ctx *ctx, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
                               const uint16_t *d_breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                               double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                               int variable_noise, float *d_out_signal, uint8_t *d_out_targets, int32_t *d_spiked, double *d_med,
                               double *d_mad, int8_t *d_status);

/* ---- introspection / measurement ---------------------------------------------------------- */

enum { XB_STAGE_CONV = 0, XB_STAGE_LSTM_IN = 1, XB_STAGE_LSTM_REC = 2, XB_STAGE_LINEAR = 3,
       XB_STAGE_DECODE = 4, XB_STAGE_COUNT = 5 };

/* Turn per-stage HIP-event timing on/off (events are recorded on the ctx stream). */
XB_API int xb_set_profiling(xb_ctx *ctx, int on);
/* Accumulated per-stage device time (ms) and kernel launch counts since the last reset;
 * synchronises the stream.  Either pointer may be NULL. */
XB_API int xb_get_stage_times(xb_ctx *ctx, float ms[XB_STAGE_COUNT], int64_t launches[XB_STAGE_COUNT]);
XB_API int xb_reset_stage_times(xb_ctx *ctx);
/* Output time steps per chunk, states, score columns of the loaded config. */
XB_API int xb_geometry(const xb_ctx *ctx, int *T, int *S, int *C_blank, int *C_noblank);
/* Diagnostic, no counterpart in the reference (tests of the mixed-precision encoder, XB_PREC_MIXED): the activations the
 * last xb_encode / xb_encode_dev of n chunks left on the device -- which = 0: output of LSTM layer 3 (nn.py:216-220, module
 * encoder.7), 1: of LSTM layer 4 (encoder.8) -- as (T, n, features) fp16 bit patterns `hi` plus the raw second part (2 bytes per
 * element: the fp16 residual, or the q8 image of DESIGN.md 2, whichever the consuming stage's arithmetic reads). */
XB_API int xb_debug_layer_output(xb_ctx *ctx, int which, int n, uint16_t *hi, uint16_t *second);
XB_API const char *xb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* XNA_BASECALLER_H */
