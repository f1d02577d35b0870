// xb_ctx.h -- the context behind the C ABI, shared by the translation units that implement it.  Inference: xb_api.hip (the
// context core: lifetime, weights, and what every entry point shares -- the call prologue `enter`, the status words, the
// workspaces), xb_run_encoder.hip (executes the encoder's plans), xb_api_scores.hip (every call on a score tensor),
// xb_api_basecall.hip (pairing, basecalls, host pipeline), xb_api_data.hip (the ctc-data tools); xb_api_priv.h holds what only
// these share.  Training: xb_head.hip (the head's trainer and the step tail every trainer ends in), xb_lstm_train.hip,
// xb_train_gemm.hip, xb_conv_train.hip, xb_top.hip (the trainers of the top LSTM layers and of every layer).  xb_comm.hip reaches
// a context through the C ABI and xb_internal_defer_after only.  The host arithmetic lives in three headers without HIP that are
// checked on their own: xb_schedule.h, xb_pack.h, xb_status.h.  Below the context: `grow`, the view of its one staging buffer
// (Staging) and the label batch every loss and training call takes (label_batch_check, LabelBatch).  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/xna_basecaller.h"
#include "xb_ctc_check.h"
#include "xb_internal.h"
#include "xb_pack.h"
#include "xb_schedule.h"
#include "xb_status.h"

using xb::half_t;

struct xb_ctx;
int fail(const xb_ctx *ctx, int code, const char *fmt, ...);     // sets the context's (or, without one, the thread's) last error

// Device memory that belongs to whoever holds the DevBuf: freed by release(), by the assignment of another buffer, or with
// its holder -- for the context's members that is xb_ctx_destroy's `delete`, with the context's device set and its streams
// drained.  Movable, not copyable.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes;
            o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // fresh memory of at least `want` bytes (a multiple of 256), whatever was held released first: the library's one hipMalloc
    int alloc(const xb_ctx *ctx, size_t want)
    {
        release();
        want = (want + 255) & ~(size_t)255;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(ctx, XB_ERR_NOMEM, "hipMalloc of %zu bytes failed: %s", want, hipGetErrorString(e));
        }
        bytes = want;
        return XB_OK;
    }
};

// Allocations that live and die together, handed out as typed pointers.  A context has three (xb_ctx: mem_ctx, mem_ws, mem_w).
struct DevPool {
    std::vector<DevBuf> bufs;

    template <typename Tp>
    int alloc(const xb_ctx *ctx, Tp **out, size_t count)
    {
        DevBuf b;
        if (int rc = b.alloc(ctx, count * sizeof(Tp))) return rc;
        *out = static_cast<Tp *>(b.p);
        bufs.push_back(std::move(b));
        return XB_OK;
    }
    bool empty() const { return bufs.empty(); }
    void release() { bufs.clear(); }
};

struct StageEvent {
    int stage;
    hipEvent_t a, b;
};

// What a Viterbi decode writes beside the bases (seq, len), by output level: 0 nothing, 1 qualities and moves (the kernel's
// quality variant), 2 those and the letter probabilities (its UB variant).  Device pointers, except in the bodies of the
// host-pointer entry points.
struct DecodeOut {
    int level = 0;
    float qscale = 1.0f, qoffset = 0.0f;
    int8_t *qstr = nullptr;      // (n, T), level >= 1
    uint8_t *moves = nullptr;    // (n, T) or nullptr, level >= 1
    uint8_t *probs = nullptr;    // (n, nb, T), level 2
};

// A decode's outputs as byte planes: seq (T bytes per chunk), len (4), qstring (T), moves (T), probs (nb T).  A level writes
// the first plane_count(level); len and moves may be null.
constexpr int PLANES = 5;
struct Planes {
    void *p[PLANES];
};

struct xb_ctx {
    xb_config cfg{};
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;    // main stream (highest priority): everything except the overlapped GEMM slabs
    hipStream_t stream2 = nullptr;   // low-priority stream: the next layer's input GEMM, slab by slab, beside the recurrence
    hipStream_t stream3 = nullptr;   // low-priority stream: CRF decode of batch k beside the encoder of batch k+1
    hipEvent_t dec_done[2] = {};     // decode that last read scores buffer p has finished
    bool dec_pending[2] = {};
    unsigned batch_idx = 0;
    hipStream_t result_stream = nullptr;   // stream that produces the outputs of the most recent *_dev call
    // host pipeline (xb_submit_chunks / xb_collect_chunks): two slots of pinned staging + device buffers
    struct Slot {
        float *h_signal = nullptr, *d_signal = nullptr;
        // pinned + device outputs of max_batch chunks, plane by plane: those of an output level are allocated by the slot's
        // first submission at that level
        Planes h{}, d{};
        unsigned *h_err = nullptr;             // snapshot of the device sync word taken on the result stream behind this batch
        hipEvent_t h2d = nullptr, done = nullptr;
        int n = 0;
        bool busy = false;
        int level = 0;                         // output level of the batch in flight
    } slots[XB_PIPELINE_SLOTS];
    bool pipeline_failed = false;          // a collected batch reported a lost rendezvous: every batch in flight fails with it
    hipStream_t stream_copy = nullptr;     // H2D of the next batch beside the compute of the current one
    std::vector<hipEvent_t> deps;    // timing-less events for the cross-stream dependencies (reused every call)
    size_t dep_next = 0;
    // the environment knobs (xb_schedule.h), read once by xb_ctx_create; lstm_mode starts from xb_config's, and lstm_signal is
    // switched off where the device or a profiler cannot serve the signal-ordered slabs
    xb::Knobs knobs;
    // one recurrence launch per layer that reports its time slabs to the GEMM stream (knobs.lstm_signal): flag word, the value
    // the last slab of the previous layer published, slab counters
    unsigned *sig_flag = nullptr, *sig_done = nullptr;
    unsigned sig_seq = 0;
    mutable std::string err;
    int T = 0, S = 0, hi = 0, O = 0, kp = 0, ld_nb = 0;
    bool weights_ready = false;
    std::map<std::string, std::vector<float>> host_w;
    // Who owns the device memory behind the typed pointers below:
    DevPool mem_ctx;                           // what lives as long as the context (and what a call allocates lazily, once)
    DevPool mem_ws;                            // the batch-sized workspaces, replaced as a whole by alloc_workspaces
    DevPool mem_w;                             // the weight set of the last xb_weights_ready, released by the next one

    // weights on device
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *b3 = nullptr;
    half_t *w3_hi = nullptr, *w3_lo = nullptr;
    half_t *wih_hi[5] = {}, *wih_lo[5] = {}, *whh_hi[5] = {}, *whh_lo[5] = {};
    float *lbias[5] = {};
    half_t *wl_hi = nullptr, *wl_lo = nullptr;
    float *bl = nullptr;
    int w3_exp = 0, wih_exp[5] = {}, whh_exp[5] = {}, wl_exp = 0;   // q8 exponents (XB_PREC_F16F8)
    // fragment-major images of the GEMM B operands (gemm4p_kernel, xb_internal.h) and their k-tile strides; the input
    // projections also as hi-only images for XB_PREC_F16F8_IN1
    unsigned char *w3_f4 = nullptr, *wih_f4[5] = {}, *wih_f4h[5] = {}, *wl_f4 = nullptr;
    size_t w3_ks = 0, wih_ks = 0, wih_ksh = 0, wl_ks = 0;
    int8_t *whh_q1[5] = {}, *whh_q0[5] = {};   // int8-limb recurrence (knobs.lstm_i8): balanced digits of W_hh, gate-interleaved rows
    float *whh_sc[5] = {};                     // ... and the factor that turns the integer sum into the recurrent term

    // activations / workspaces
    float *d_signal = nullptr;
    half_t *im_hi = nullptr, *im_lo = nullptr;
    half_t *x_hi[2] = {}, *x_lo[2] = {};
    float *gin = nullptr, *gin2 = nullptr, *c_state = nullptr, *scores = nullptr, *scores2 = nullptr;
    half_t *xh = nullptr;        // LSTM exchange buffer: 64 groups x 2 parity x 2 parts x 64 chunks x F
    float *alpha = nullptr, *beta = nullptr, *bmax = nullptr, *qbuf = nullptr, *logz = nullptr;
    // beam search workspaces and staging (lazily allocated: most contexts never use them)
    uint32_t *beam_hist = nullptr;
    int32_t *beam_path = nullptr;
    float *beam_prob = nullptr, *beam_score = nullptr;
    int8_t *beam_seq = nullptr, *beam_q = nullptr;
    uint8_t *beam_moves = nullptr;
    int8_t *labels = nullptr, *seq = nullptr;
    int32_t *seq_len = nullptr;
    // the planes of output levels 1 (qstring, moves) and 2 (probs), lazily allocated by ensure_staging: the device staging
    // of the host-pointer calls (max_batch chunks) and the results of a co-scheduled pair before they are split
    // (2 max_batch); level 2 also the per-step letter mass workspace (cap, T, nb) fp32
    int8_t *q_seq = nullptr, *q_fseq = nullptr;
    uint8_t *q_moves = nullptr, *q_fmoves = nullptr;
    uint8_t *u_probs = nullptr, *u_fprobs = nullptr;
    float *u_buf = nullptr;
    // [64 groups * 32] arrival counters, then 32 words that hold the two status words (xb_status.h), then the slab counters.
    // error: the sync word, which the recurrence polls and stores (LstmParams::error); error_data: the data word of the
    // validating kernels (CtcParams::error, CtcLossParams::error), STATUS_DATA_AT words on: another 64-byte line
    unsigned *sync = nullptr;
    unsigned *error = nullptr, *error_data = nullptr;
    static constexpr int STATUS_DATA_AT = 16;
    // workgroups of the persistent kernel admitted per CU, by recurrence arithmetic (nsplit 1..5) and one / two groups per
    // workgroup (occupancy query, lazily; -1 = not asked yet)
    int lstm_resident[6][2] = {{-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}};
    // Arithmetic of every contraction stage (GemmParams::nsplit: 1 fp16 product, 2 + FP8 corrections, 3 three fp16 products):
    // conv3, the five input projections, the five recurrences, the CRF linear layer.  One value everywhere for the plain
    // precisions; XB_PREC_MIXED (and the diagnostic XB_X3_STAGES mask) mix 2 and 3.  An activation tensor's second part
    // (q8 image or fp16 residual) follows the stage that CONSUMES it.
    int ns_conv = 3, ns_in[5] = {3, 3, 3, 3, 3}, ns_rec[5] = {3, 3, 3, 3, 3}, ns_lin = 3;

    // Two asynchronous basecalls in flight are co-scheduled once the caller has opted in with xb_reserve_pairing (contexts of at
    // most 512 chunks; XB_FUSE=0 refuses): the first xb_basecall_chunks_dev of a pair is held back until the second arrives, then
    // both batches go through the encoder and the decode as ONE batch (the recurrence then runs two chunk groups per workgroup,
    // DESIGN.md 4.1 / 4.5).  Every other entry point, xb_synchronize and xb_result_stream first launch a held-back call on its own.
    // Without the opt-in every asynchronous call is enqueued before it returns.
    struct Call {
        const float *signal = nullptr;
        int n = 0;
        char alphabet[16] = {};
        int8_t *seq = nullptr;
        int32_t *len = nullptr;
        int slot = -1;                          // host pipeline slot whose D2H copies and done event follow the launch
        void (*after)(void *) = nullptr;        // xb_comm: the gather of this call's results, enqueued right behind it
        void *after_arg = nullptr;
        DecodeOut out;                          // output level (xb_basecall_chunks_q / _ub, xb_submit_chunks_q / _ub) and its planes
    };
    int fuse_ok = 1;                            // pairing is possible in this context (schedule, batch size, XB_FUSE)
    int fuse = 0;                               // ... and the caller asked for it (xb_reserve_pairing)
    int cap = 0;                                // chunks the workspaces hold (2 * max_batch when fusing is possible)
    Call held;
    bool holding = false, flushing = false;
    int deferred_rc = 0;                        // failure of a held-back call that was launched where no status could be returned
    int8_t *fseq = nullptr;                     // (cap, T) / (cap) results of a fused pair before they are split
    int32_t *flen = nullptr;
    const float *last_scores = nullptr;         // the blank-less scores (T, last_n, ld_nb) of the most recent basecall pass, until the
    int last_n = 0;                             // next encoder run (xb_validate_chunks reads them where they lie)

    // The device staging of every host-pointer form that needs some (Staging, below): the ctc-data tools, the losses,
    // xb_head_grad, and the label batch of the trainers' steps.  One buffer for all of them -- each returns synchronised, so no
    // two are ever live at once.  Grows with the calls; lives as long as the context.
    DevBuf staging;

    // template mapper (xb_map_templates): the library last passed in (host copy and its device image: codes, offsets, the
    // chunks of the score pass) and buffers that grow with the calls -- the score pass's records, the trace pass's direction
    // scratch.  Live as long as the context.
    struct MapState {
        std::vector<char> lib;
        std::vector<int32_t> off;
        int Lmax = 0, nchunks = 0;
        DevBuf image, partial, scratch;
        // the image's layout: codes | offsets, 16-byte aligned | the first template of every chunk and the count of templates |
        // the letters as they were passed in (xb_barcode_dist compares bytes, not codes)
        static size_t off_at(size_t total) { return (total + 15) & ~(size_t)15; }
        const uint8_t *tcodes() const { return static_cast<const uint8_t *>(image.p); }
        const int32_t *toff() const { return reinterpret_cast<const int32_t *>(tcodes() + off_at(lib.size())); }
        const int32_t *chunk_first() const { return toff() + off.size(); }
        const uint8_t *tletters() const { return reinterpret_cast<const uint8_t *>(chunk_first() + nchunks + 1); }
    } map;

    // DTW segmentation (xb_dtw_segment): the choice-bit scratch of the launches in flight and the chunks' level offsets on
    // their way to the device -- two pinned slots in rotation, so that a call returns without waiting for its own device
    // work.  The device side lives as long as the context; xb_ctx_destroy frees the pinned side and the events.
    struct DtwState {
        DevBuf scratch;
        struct Slot {
            int32_t *h = nullptr;
            DevBuf d;                                   // `count` int32
            size_t count = 0;
            hipEvent_t copied = nullptr;
        } off[2];
        unsigned calls = 0;
        size_t scratch_written = 0;                 // bytes of choice words the last call's launches were sized for
    } dtw;

    // XNA spliced augmentation (xb_splice_library / xb_splice_chunks): the library's device image, kept until the next
    // xb_splice_library.  Lives as long as the context.
    struct SpliceState {
        DevBuf pool, rows, table;
        bool loaded = false;
    } splice;

    // XNA synthetic spiking (xb_spike_model / xb_spike_chunks / xb_synth_chunks): the k-mer table, kept until the next xb_spike_model.  Lives
    // as long as the context.
    struct SpikeState {
        DevBuf model;
        bool loaded = false;
    } spike;

    // The loss gradient (xb_ctc_loss_grad): the alpha stash of one launch of the lattice kernel (bounded by XB_CTC_SCRATCH_MB)
    // and the chunks' weights; the posteriors lie in the decode's qbuf.  Grow with the calls; live as long as the context.
    struct CtcGradState {
        DevBuf stash, w;
    } ctcgrad;

    // The head's gradient and trainer (xb_head.hip).  part: the slabs' partial sums of one launch of xb_head_grad (bounded by
    // XB_HEAD_SCRATCH_MB); small: max |dY| word, the norm's partial sums and result.  While a trainer is open
    // (xb_head_train_begin .. _end): the fp32 master weights, AdamW's moments and the gradient in one buffer (W, b, mW, mb, vW,
    // vb, dW, db), the batch's score gradient, and the step count; a step's labels and losses lie in `staging`.  part and small
    // live as long as the context; the trainer's two from xb_head_train_begin / _step to close() (xb_head_train_end).
    struct HeadState {
        DevBuf part, small, train, grad;
        bool open = false;
        long step = 0;
        void close()
        {
            train.release(); grad.release();
            open = false;
            step = 0;
        }
    } head;
    // The LSTM layer's training recurrence (xb_lstm_train.hip): the (n, F) cell-gradient carry of the backward's steps and the
    // transposed recurrent weights (F, 4F) of the call in flight.  Grow with the calls; live as long as the context.
    struct LstmTrainState {
        DevBuf carry, wt;
    } lstmtrain;
    // The convolutions' training (xb_conv_train.hip): the wide route's workspace of the call in flight (dz | col | dcol | wt,
    // xb_conv_plan.h) and the narrow route's float64 partials of dw and db.  Grow with the calls; live as long as the context.
    struct ConvTrainState {
        DevBuf ws, part;
    } convtrain;
    // The trainer of the head and the top L LSTM layers (xb_top.hip), open from xb_top_train_begin to _end.  train: p, g, m, v in
    // the layout of xb::top_plan, four strides; small: the norm word (64 floats), the layers' summed biases, one transposed
    // weight; act: the activations of a step of `rows` = T n rows, allocated by the first step and grown with the batch; a
    // step's labels and losses lie in `staging`.  full (xb_full_train_begin, L = 5): the six conv tensors lie in front of the LSTM
    // section in each of p, g, m, v, and the conv stack's activations (xb_conv_plan.h) behind the others in act.
    struct TopState {
        DevBuf train, small, act;
        bool open = false, full = false;
        int L = 0;
        long step = 0;
        size_t rows = 0;                        // rows the activations were last laid out for (0: no step yet)
        void close()
        {
            train.release(); small.release(); act.release();
            open = full = false;
            L = 0; step = 0; rows = 0;
        }
    } top;
    int enc_n = 0;                              // chunks of the most recent full encoder pass (whose layer outputs lie in x_hi / x_lo)

    bool profiling = false;
    std::vector<StageEvent> events;
    float stage_ms[XB_STAGE_COUNT] = {};
    int64_t stage_launches[XB_STAGE_COUNT] = {};
};

#define XB_HIP(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, e_ == hipErrorOutOfMemory ? XB_ERR_NOMEM : XB_ERR_HIP,           \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// a buffer that grows with the calls: at least `bytes` afterwards, contents not kept
inline int grow(xb_ctx *ctx, DevBuf *b, size_t bytes)
{
    if (bytes <= b->bytes) return XB_OK;
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));                     // nothing in flight reads the old buffer
    return b->alloc(ctx, bytes);
}

// The device staging of a host-pointer form: typed pieces of xb_ctx::staging in the order they are taken, each 256-byte
// aligned.  `used` is their total; once ready() has grown the buffer to it, a piece converts to its device pointer.  The buffer
// is the context's only one, so it relies on this: whoever takes pieces returns synchronised (xb_synchronize) -- no two uses
// are ever live at once, and nothing in flight reads the buffer when the next call lays it out anew.
struct Staging {
    xb_ctx *ctx;
    size_t used = 0;
    template <typename Tp> struct Piece {
        const DevBuf *buf; size_t at;
        operator Tp *() const { return reinterpret_cast<Tp *>(static_cast<uint8_t *>(buf->p) + at); }
    };
    template <typename Tp> Piece<Tp> take(size_t count)
    {
        const size_t at = used;
        used += (count * sizeof(Tp) + 255) & ~(size_t)255;
        return {&ctx->staging, at};
    }
    int ready() { return grow(ctx, &ctx->staging, used); }
};

// What every loss and training call refuses of a label batch (n rows of Lt labels, their lengths) before any device work: a
// width whose positions the lattice kernels do not hold, then -- where the rows are on the host (targets != null) -- the first
// length or label out of range.  The _dev forms pass null: their rows are validated by the kernel, on the device.
inline int label_batch_check(xb_ctx *ctx, const char *who, const uint8_t *targets, int n, int Lt, const int32_t *lengths)
{
    const int np = Lt - (ctx->cfg.state_len - 1);
    if (np < 1 || np > xb::ctc_max_positions())
        return fail(ctx, XB_ERR_INVALID, "%s: target width %d gives %d positions, supported: 1..%d", who, Lt, np, xb::ctc_max_positions());
    char msg[160];
    if (targets && xb::ctc_labels_check(targets, n, Lt, lengths, ctx->cfg.state_len, ctx->cfg.n_base, msg, sizeof msg))
        return fail(ctx, XB_ERR_INVALID, "%s: %s", who, msg);
    return XB_OK;
}

// A label batch on the device: the targets, the lengths and the chunks' losses as three pieces of a Staging, taken in this
// order.  upload() follows the Staging's ready().
struct LabelBatch {
    size_t n, Lt;
    Staging::Piece<uint8_t> targets;
    Staging::Piece<int32_t> len;
    Staging::Piece<float> loss;
    LabelBatch(Staging &st, int n_, int Lt_)
        : n((size_t)n_), Lt((size_t)Lt_), targets(st.take<uint8_t>(n * Lt)), len(st.take<int32_t>(n)), loss(st.take<float>(n)) {}
    int upload(xb_ctx *ctx, const uint8_t *h_targets, const int32_t *h_lengths) const
    {
        XB_HIP(ctx, hipMemcpyAsync(targets, h_targets, n * Lt, hipMemcpyHostToDevice, ctx->stream));
        XB_HIP(ctx, hipMemcpyAsync(len, h_lengths, n * 4, hipMemcpyHostToDevice, ctx->stream));
        return XB_OK;
    }
};

// what follows the launches of an entry point `who`: a launch the runtime refused
inline int launched(const xb_ctx *ctx, const char *who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, XB_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return XB_OK;
}

// the core (xb_api.hip) as the other translation units call it; none is exported (the library is built with hidden visibility)
int check_ready(xb_ctx *ctx, int n);     // a context with weights and room for a batch of n
int check_alphabet(xb_ctx *ctx, const char *alphabet);
int join_async_decode(xb_ctx *ctx);      // flush_held, then the main stream waits for decodes in flight on the third stream
// The entry of a call, after its own checks: the context's device, nothing held back, the main stream behind decodes in flight
// beside it.  dev: the call leaves its results to the main stream (every _dev form), named after a held call was launched.
int enter(xb_ctx *ctx, bool dev);
// the loss runners (xb_api_scores.hip) and the encoder's (xb_run_encoder.hip), as the trainers call them too
int ctc_loss_run(xb_ctx *ctx, const char *who, const float *d_scores, int T, int n, int has_blank, int ld, const uint8_t *d_targets,
                 int Lt, const int32_t *d_len, float *d_loss, float *d_logz);
int ctc_grad_run(xb_ctx *ctx, const char *who, const float *d_scores, int T, int n, int has_blank, int ld, const uint8_t *d_targets,
                 int Lt, const int32_t *d_len, float loss_clip, int mean, float *d_loss, float *d_grad);
int encoder_run(xb_ctx *ctx, const float *d_signal, int n, float *d_scores, int ldc);   // blank-less scores (T, n, ldc), main stream
// the convolutions and the first `layers` (0 .. 5) LSTM layers of the same pass; the output lies in x_hi / x_lo [layers & 1]
int encoder_bottom_run(xb_ctx *ctx, const float *d_signal, int n, int layers);
