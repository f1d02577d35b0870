// xb_api_scores.hip -- every call of the C ABI on a (T, n, C) score tensor: the Viterbi decodes at three output levels, the CRF
// scans, the CTC scan, the beam search and the losses, each in a host and a _dev form; the decode runner and the staging planes
// they share with the basecalls.  The public header declares every XB_API function extern "C"; nothing else here is.
#include "xb_api_priv.h"

// What every entry point here refuses first, before its pointers and before enter(): no context, the batch range, then T.
// *ld = the row stride of the scores' layout.  who: what the loss family's messages begin with ("xb_ctc_loss: "), "" for the others.
static int score_args(xb_ctx *ctx, const char *who, int T, int n, int has_blank, int *ld)
{
    if (!ctx) return XB_ERR_INVALID;
    if (n < 1 || n > ctx->cfg.max_batch)
        return fail(ctx, XB_ERR_INVALID, "%sbatch %d outside [1, max_batch=%d]", who, n, ctx->cfg.max_batch);
    if (T < 1 || T > ctx->T) return fail(ctx, XB_ERR_INVALID, "%sT=%d outside [1, %d]", who, T, ctx->T);
    *ld = has_blank ? ctx->S * (ctx->cfg.n_base + 1) : ctx->O;
    return XB_OK;
}

// host scores (T, n, ld) into ctx->scores on the main stream
static int stage_scores(xb_ctx *ctx, const float *scores, int T, int n, int ld)
{
    XB_HIP(ctx, hipMemcpyAsync(ctx->scores, scores, sizeof(float) * (size_t)T * n * ld, hipMemcpyHostToDevice, ctx->stream));
    return XB_OK;
}

Planes planes(void *seq, void *len, const DecodeOut &o) { return {{seq, len, o.qstr, o.moves, o.probs}}; }
int plane_count(int level) { return level == 0 ? 2 : (level == 1 ? 4 : 5); }
size_t plane_bytes(int T, int nb, int i) { return i == 1 ? sizeof(int32_t) : (i == 4 ? (size_t)nb * T : (size_t)T); }
// seq, and by level qstring and probs: the planes an entry point requires (xb_decode alone may leave seq out)
bool has_required(const Planes &o, int level) { return o.p[0] && (level < 1 || o.p[2]) && (level < 2 || o.p[4]); }

// out: the outputs of level 1 and 2 (the quality variant writes its beta rows into the beta stash); null for level 0
int run_decode(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, int ld, const char *alphabet, int8_t *d_labels,
               int8_t *d_seq, int32_t *d_len, hipStream_t st, const ScanOut *scan, const DecodeOut *out)
{
    if (!st) st = ctx->stream;
    const xb_config &c = ctx->cfg;
    xb::DecodeParams p{};
    p.scores = d_scores; p.T = T; p.N = n; p.S = ctx->S; p.hi = ctx->hi; p.nb = c.n_base;
    p.cin = has_blank ? ctx->S * (c.n_base + 1) : ctx->S * c.n_base;
    p.ld = ld; p.has_blank = has_blank; p.blank = c.blank_score;
    p.alpha = ctx->alpha; p.beta = ctx->beta; p.bmax = ctx->bmax;
    p.qbuf = ctx->qbuf; p.ldq = (ctx->S * (c.n_base + 1) + 3) & ~3;
    if (scan) {
        if (scan->alpha) p.alpha = scan->alpha;
        p.logz = scan->logz;
        p.beta_out = scan->beta;
        if (scan->post) { p.qbuf = scan->post; p.post_mode = 1; }
        p.stop_after = (scan->beta || scan->post) ? 2 : 1;
    }
    p.labels = d_labels; p.seq = d_seq; p.seq_len = d_len;
    if (out && out->level >= 1) {
        if (!out->qstr || !d_seq) return fail(ctx, XB_ERR_INVALID, "qualities need the seq and qstring outputs");
        p.qstr = out->qstr; p.moves = out->moves; p.qscale = out->qscale; p.qoffset = out->qoffset;
        p.beta_out = ctx->beta;
        if (out->level == 2) {
            if (!ctx->u_buf) return fail(ctx, XB_ERR_INVALID, "letter probabilities need their workspace");
            p.probs = out->probs; p.ubuf = ctx->u_buf;
        }
    }
    memset(p.alphabet, 0, sizeof p.alphabet);
    if (alphabet) {
        if ((int)strlen(alphabet) < c.n_base + 1) return fail(ctx, XB_ERR_INVALID, "alphabet needs %d symbols", c.n_base + 1);
        memcpy(p.alphabet, alphabet, (size_t)c.n_base + 1);
    } else if (d_seq) {
        return fail(ctx, XB_ERR_INVALID, "alphabet is required when seq is requested");
    }
#ifdef XB_LSTM_STAMPS
    if (const char *e = getenv("XB_DECODE_STOP")) p.debug_stop = atoi(e);
    if (const char *e = getenv("XB_DECODE_LINEAR_LDS")) p.debug_lds = atoi(e);
#endif
    StageScope sc(ctx, XB_STAGE_DECODE, 1, st);
    hipError_t e = xb::launch_crf_decode(p, st);
    if (e != hipSuccess) return fail(ctx, e == hipErrorInvalidValue ? XB_ERR_INVALID : XB_ERR_HIP, "crf decode launch failed: %s", hipGetErrorString(e));
    return XB_OK;
}

template <typename Tp>
static int dev_alloc_once(xb_ctx *ctx, Tp **out, size_t count) { return *out ? XB_OK : ctx->mem_ctx.alloc(ctx, out, count); }

// device staging and workspace of an output level (once per context; level 2 includes level 1's).  The pair planes exist
// only where calls can pair (enqueue_call pairs none of a level while they are missing).
int ensure_staging(xb_ctx *ctx, int level)
{
    const size_t NT = (size_t)ctx->cfg.max_batch * ctx->T, NPT = NT * ctx->cfg.n_base;
    const bool pairs = ctx->fuse_ok != 0;
    int rc = XB_OK;
    if (level >= 1) {
        rc = rc ? rc : dev_alloc_once(ctx, &ctx->q_seq, NT);
        rc = rc ? rc : dev_alloc_once(ctx, &ctx->q_moves, NT);
        if (pairs) rc = rc ? rc : dev_alloc_once(ctx, &ctx->q_fseq, 2 * NT);
        if (pairs) rc = rc ? rc : dev_alloc_once(ctx, &ctx->q_fmoves, 2 * NT);
    }
    if (level == 2) {
        rc = rc ? rc : dev_alloc_once(ctx, &ctx->u_buf, (pairs ? 2 : 1) * NPT);
        rc = rc ? rc : dev_alloc_once(ctx, &ctx->u_probs, NPT);
        if (pairs) rc = rc ? rc : dev_alloc_once(ctx, &ctx->u_fprobs, 2 * NPT);
    }
    return rc;
}

// the device staging of a host-pointer call with outputs o: the same level and calibration, moves only where o has them
DecodeOut staging_of(const xb_ctx *ctx, const DecodeOut &o)
{
    DecodeOut d = o;
    d.qstr = ctx->q_seq; d.moves = o.moves ? ctx->q_moves : nullptr; d.probs = ctx->u_probs;
    return d;
}

// chunks [c0, c0 + n) of the planes of a level from src to chunks [0, n) of dst (rows of T steps); planes null on either
// side are skipped
int copy_planes(xb_ctx *ctx, int level, const Planes &dst, const Planes &src, int c0, int n, int T, hipMemcpyKind kind,
                hipStream_t st)
{
    for (int i = 0; i < plane_count(level); ++i) {
        const size_t b = plane_bytes(T, ctx->cfg.n_base, i);
        if (dst.p[i] && src.p[i])
            XB_HIP(ctx, hipMemcpyAsync(dst.p[i], static_cast<const char *>(src.p[i]) + (size_t)c0 * b, (size_t)n * b, kind, st));
    }
    return XB_OK;
}

// what the loss and its gradient tell the lattice kernels alike: the scores, the labels, logZ_crf where the Log forward scan of
// run_decode leaves it, and the experiments' workgroup size
static xb::CtcLossParams ctc_loss_params(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, int ld,
                                         const uint8_t *d_targets, int Lt, const int32_t *d_len, float *d_loss, float *d_logz)
{
    const xb_config &c = ctx->cfg;
    xb::CtcLossParams p{};
    p.scores = d_scores; p.T = T; p.N = n; p.ld = ld; p.has_blank = has_blank; p.blank = c.blank_score;
    p.nb = c.n_base; p.sl = c.state_len; p.targets = d_targets; p.Lt = Lt; p.tlen = d_len;
    p.logz_crf = ctx->logz; p.loss = d_loss; p.logz = d_logz; p.error = ctx->error_data;
    if (const char *e = getenv("XB_CTC_LOSS_THREADS")) p.threads = atoi(e);
    return p;
}

static int ctc_launched(xb_ctx *ctx, const char *who, hipError_t e)
{
    if (e == hipSuccess) return XB_OK;
    return fail(ctx, e == hipErrorInvalidValue ? XB_ERR_INVALID : XB_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

// The validation loss of n chunks from device-resident RAW scores (T, n, ld), for xb_ctc_loss and xb_validate_chunks: the Log
// forward scan leaves logZ_crf in the decode's own (max_batch) buffer, the CTC forward scan of the labels reads it there.  Two
// launches on the main stream, nothing waited for; the callers have checked n, T, the pointers and the width (label_batch_check).
int ctc_loss_run(xb_ctx *ctx, const char *who, const float *d_scores, int T, int n, int has_blank, int ld, const uint8_t *d_targets,
                 int Lt, const int32_t *d_len, float *d_loss, float *d_logz)
{
    ScanOut so;
    so.logz = ctx->logz;
    if (int rc = run_decode(ctx, d_scores, T, n, has_blank, ld, nullptr, nullptr, nullptr, nullptr, nullptr, &so)) return rc;
    const xb::CtcLossParams p = ctc_loss_params(ctx, d_scores, T, n, has_blank, ld, d_targets, Lt, d_len, d_loss, d_logz);
    StageScope sc(ctx, XB_STAGE_DECODE, 1);
    return ctc_launched(ctx, who, xb::launch_ctc_loss(p, ctx->stream));
}

// The loss and d loss / d scores of n chunks from device-resident RAW scores (T, n, ld), for xb_ctc_loss_grad and the trainers'
// steps (every caller has been through label_batch_check): the Log scans leave logZ_crf and the edge posteriors in the decode's
// own workspaces (logz, qbuf); the lattice kernel runs over as many chunks per launch as the stash bound holds, then the fill
// kernel over all.  All on the main stream, nothing waited for unless a workspace grows.
int ctc_grad_run(xb_ctx *ctx, const char *who, const float *d_scores, int T, int n, int has_blank, int ld, const uint8_t *d_targets,
                 int Lt, const int32_t *d_len, float loss_clip, int mean, float *d_loss, float *d_grad)
{
    const xb_config &c = ctx->cfg;
    const int np = Lt - (c.state_len - 1);
    const size_t slot = xb::ctc_grad_slot_floats(T, np);
    const size_t per_launch = xb::ctc_grad_chunks_per_launch(T, np, n, xb::ctc_scratch_bound(getenv("XB_CTC_SCRATCH_MB")));
    if (int rc = grow(ctx, &ctx->ctcgrad.stash, per_launch * slot * sizeof(float))) return rc;
    if (int rc = grow(ctx, &ctx->ctcgrad.w, sizeof(float) * (size_t)c.max_batch)) return rc;
    ScanOut so;
    so.logz = ctx->logz; so.post = ctx->qbuf;
    if (int rc = run_decode(ctx, d_scores, T, n, has_blank, ld, nullptr, nullptr, nullptr, nullptr, nullptr, &so)) return rc;
    xb::CtcGradParams q{};
    q.l = ctc_loss_params(ctx, d_scores, T, n, has_blank, ld, d_targets, Lt, d_len, d_loss, nullptr);
    q.post = ctx->qbuf; q.ldq = (ctx->S * (c.n_base + 1) + 3) & ~3;
    q.stash = static_cast<float *>(ctx->ctcgrad.stash.p); q.slot = slot;
    q.loss_clip = loss_clip; q.mean = mean ? 1 : 0;
    q.w = static_cast<float *>(ctx->ctcgrad.w.p); q.grad = d_grad;
    for (size_t first = 0; first < (size_t)n; first += per_launch) {
        q.first = (int)first;
        q.count = (int)std::min<size_t>(per_launch, (size_t)n - first);
        if (int rc = ctc_launched(ctx, who, xb::launch_ctc_grad(q, ctx->stream))) return rc;
    }
    return ctc_launched(ctx, who, xb::launch_ctc_grad_fill(q, ctx->stream));
}

// the device-pointer decodes: labels (level 0 only), the bases and the outputs of o's level, on the main stream
static int decode_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet, int8_t *d_labels,
                      int8_t *d_seq, int32_t *d_seq_len, const DecodeOut &o)
{
    int ld = 0;
    if (int rc = score_args(ctx, "", T, n, has_blank, &ld)) return rc;
    if (o.level == 0 && !d_scores) return fail(ctx, XB_ERR_INVALID, "null device pointer");
    if (o.level >= 1 && (!d_scores || !has_required(planes(d_seq, d_seq_len, o), o.level) || !alphabet))
        return fail(ctx, XB_ERR_INVALID, "null argument");
    if (int rc = enter(ctx, true)) return rc;
    if (o.level == 2)                                 // the letter mass workspace
        if (int rc = ensure_staging(ctx, 2)) return rc;
    return run_decode(ctx, d_scores, T, n, has_blank ? 1 : 0, ld, alphabet, d_labels, d_seq, d_seq_len, nullptr, nullptr, &o);
}

// the host-pointer decodes: through the context's staging; labels and a null seq at level 0 only
static int decode_host(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, int8_t *labels,
                       int8_t *seq, int32_t *seq_len, const DecodeOut &o)
{
    int ld = 0;
    if (int rc = score_args(ctx, "", T, n, has_blank, &ld)) return rc;
    const Planes dst = planes(seq, seq_len, o);
    if (o.level == 0 && !scores) return fail(ctx, XB_ERR_INVALID, "null host pointer");
    if (o.level >= 1 && (!scores || !has_required(dst, o.level) || !alphabet)) return fail(ctx, XB_ERR_INVALID, "null argument");
    if (int rcj = enter(ctx, false)) return rcj;
    if (o.level)
        if (int rcs = ensure_staging(ctx, o.level)) return rcs;
    if (int rcs = stage_scores(ctx, scores, T, n, ld)) return rcs;
    const DecodeOut d = staging_of(ctx, o);
    int rc = run_decode(ctx, ctx->scores, T, n, has_blank ? 1 : 0, ld, alphabet, o.level ? nullptr : ctx->labels,
                        seq ? ctx->seq : nullptr, ctx->seq_len, nullptr, nullptr, &d);
    if (rc) return rc;
    if (labels) XB_HIP(ctx, hipMemcpyAsync(labels, ctx->labels, (size_t)n * T, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = copy_planes(ctx, o.level, dst, planes(ctx->seq, ctx->seq_len, d), 0, n, T, hipMemcpyDeviceToHost, ctx->stream)))
        return rc;
    return xb_synchronize(ctx);
}

XB_API int xb_decode_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet,
                         int8_t *d_labels, int8_t *d_seq, int32_t *d_seq_len)
{
    return decode_dev(ctx, d_scores, T, n, has_blank, alphabet, d_labels, d_seq, d_seq_len, {});
}

XB_API int xb_decode(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet,
                     int8_t *labels, int8_t *seq, int32_t *seq_len)
{
    return decode_host(ctx, scores, T, n, has_blank, alphabet, labels, seq, seq_len, {});
}

XB_API int xb_decode_q_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet, float qscale,
                           float qoffset, int8_t *d_seq, int8_t *d_qstring, uint8_t *d_moves, int32_t *d_seq_len)
{
    return decode_dev(ctx, d_scores, T, n, has_blank, alphabet, nullptr, d_seq, d_seq_len, {1, qscale, qoffset, d_qstring, d_moves});
}

XB_API int xb_decode_q(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, float qscale,
                       float qoffset, int8_t *seq, int8_t *qstring, uint8_t *moves, int32_t *seq_len)
{
    return decode_host(ctx, scores, T, n, has_blank, alphabet, nullptr, seq, seq_len, {1, qscale, qoffset, qstring, moves});
}

XB_API int xb_decode_ub_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet,
                            float qscale, float qoffset, int8_t *d_seq, int8_t *d_qstring, uint8_t *d_moves, uint8_t *d_probs,
                            int32_t *d_seq_len)
{
    return decode_dev(ctx, d_scores, T, n, has_blank, alphabet, nullptr, d_seq, d_seq_len,
                      {2, qscale, qoffset, d_qstring, d_moves, d_probs});
}

XB_API int xb_decode_ub(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, float qscale,
                        float qoffset, int8_t *seq, int8_t *qstring, uint8_t *moves, uint8_t *probs, int32_t *seq_len)
{
    return decode_host(ctx, scores, T, n, has_blank, alphabet, nullptr, seq, seq_len, {2, qscale, qoffset, qstring, moves, probs});
}

XB_API int xb_crf_scans_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, float *d_alpha, float *d_beta,
                            float *d_logz, float *d_post)
{
    int ld = 0;
    if (int rc = score_args(ctx, "", T, n, has_blank, &ld)) return rc;
    if (!d_scores) return fail(ctx, XB_ERR_INVALID, "null device pointer");
    if (!d_alpha && !d_beta && !d_logz && !d_post) return fail(ctx, XB_ERR_INVALID, "no output requested");
    if (int rc = enter(ctx, true)) return rc;       // the scans run on the main stream (not on the async decode stream)
    ScanOut so;
    so.alpha = d_alpha; so.beta = d_beta; so.logz = d_logz; so.post = d_post;
    return run_decode(ctx, d_scores, T, n, has_blank ? 1 : 0, ld, nullptr, nullptr, nullptr, nullptr, nullptr, &so);
}

XB_API int xb_crf_scans(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, float *alpha, float *beta, float *logz,
                        float *post)
{
    int ld = 0;
    if (int rc = score_args(ctx, "", T, n, has_blank, &ld)) return rc;
    if (!scores) return fail(ctx, XB_ERR_INVALID, "null host pointer");
    if (!alpha && !beta && !logz && !post) return fail(ctx, XB_ERR_INVALID, "no output requested");
    if (int rcj = enter(ctx, false)) return rcj;
    const int S = ctx->S, E = ctx->cfg.n_base + 1;
    if (int rcs = stage_scores(ctx, scores, T, n, ld)) return rcs;
    // device staging in the decode's own workspaces: alpha -> its stash, beta -> the (otherwise unused) beta stash, P -> the
    // Q buffer (row stride ldq), logZ -> its own (max_batch) buffer
    const int ldq = (S * E + 3) & ~3;
    ScanOut so;
    so.alpha = ctx->alpha; so.beta = beta ? ctx->beta : nullptr; so.post = post ? ctx->qbuf : nullptr;
    so.logz = logz ? ctx->logz : nullptr;
    int rc = run_decode(ctx, ctx->scores, T, n, has_blank ? 1 : 0, ld, nullptr, nullptr, nullptr, nullptr, nullptr, &so);
    if (rc) return rc;
    const size_t sv = sizeof(float) * (size_t)(T + 1) * n * S;
    if (alpha) XB_HIP(ctx, hipMemcpyAsync(alpha, ctx->alpha, sv, hipMemcpyDeviceToHost, ctx->stream));
    if (beta) XB_HIP(ctx, hipMemcpyAsync(beta, ctx->beta, sv, hipMemcpyDeviceToHost, ctx->stream));
    if (logz) XB_HIP(ctx, hipMemcpyAsync(logz, so.logz, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (post)
        XB_HIP(ctx, hipMemcpy2DAsync(post, sizeof(float) * (size_t)S * E, ctx->qbuf, sizeof(float) * (size_t)ldq,
                                     sizeof(float) * (size_t)S * E, (size_t)T * n, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

XB_API int xb_crf_logz_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, float *d_logz)
{
    return xb_crf_scans_dev(ctx, d_scores, T, n, has_blank, nullptr, nullptr, d_logz, nullptr);
}

XB_API int xb_crf_logz(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, float *logz)
{
    return xb_crf_scans(ctx, scores, T, n, has_blank, nullptr, nullptr, logz, nullptr);
}

static int run_ctc(xb_ctx *ctx, const float *scores, int T, int n, const int32_t *targets, int Lt, const int32_t *tlen,
                   int semiring, float *logz, float *gstay, float *gmove)
{
    int C = 0;                                              // the scores have the blank column
    if (int rc = score_args(ctx, "", T, n, 1, &C)) return rc;
    const int sl = ctx->cfg.state_len, nb = ctx->cfg.n_base;
    if (!scores || !targets || !tlen) return fail(ctx, XB_ERR_INVALID, "null host pointer");
    if (!logz && !gstay && !gmove) return fail(ctx, XB_ERR_INVALID, "no output requested");
    const int np = Lt - (sl - 1);
    if (np < 1 || np > xb::ctc_max_positions())
        return fail(ctx, XB_ERR_INVALID, "target width %d gives %d positions, supported: 1..%d", Lt, np, xb::ctc_max_positions());
    for (int b = 0; b < n; ++b) {
        if (tlen[b] < sl || tlen[b] > Lt)
            return fail(ctx, XB_ERR_INVALID, "target_lengths[%d] = %d outside [state_len = %d, %d]", b, tlen[b], sl, Lt);
        for (int l = 0; l < Lt; ++l)
            if (targets[(size_t)b * Lt + l] < 0 || targets[(size_t)b * Lt + l] > nb)
                return fail(ctx, XB_ERR_INVALID, "targets[%d][%d] = %d outside [0, n_base = %d]", b, l, targets[(size_t)b * Lt + l], nb);
    }
    if (int rcj = enter(ctx, true)) return rcj;             // (a host form that has always named the main stream)
    const std::vector<uint8_t> labels(targets, targets + (size_t)n * Lt);      // the kernels' label type; every value is in [0, nb]
    const size_t nm = np > 1 ? np - 1 : 1;
    // per-call device scratch (a training-side operator: sizes follow the targets, not the context), freed on every return
    DevBuf b_lab, b_len, b_alpha, b_gs, b_gm;
    const bool grads = gstay || gmove;
    if (int rc = b_lab.alloc(ctx, labels.size())) return rc;
    if (int rc = b_len.alloc(ctx, sizeof(int32_t) * (size_t)n)) return rc;
    if (grads) {
        if (int rc = b_alpha.alloc(ctx, sizeof(float) * (size_t)n * (T + 1) * np)) return rc;
        if (int rc = b_gs.alloc(ctx, sizeof(float) * (size_t)T * n * np)) return rc;
        if (gmove)
            if (int rc = b_gm.alloc(ctx, sizeof(float) * (size_t)T * n * nm)) return rc;
    }
    uint8_t *d_lab = static_cast<uint8_t *>(b_lab.p);
    int32_t *d_len = static_cast<int32_t *>(b_len.p);
    float *d_alpha = static_cast<float *>(b_alpha.p), *d_gs = static_cast<float *>(b_gs.p), *d_gm = static_cast<float *>(b_gm.p);
    hipStream_t st = ctx->stream;
    XB_HIP(ctx, hipMemcpyAsync(d_lab, labels.data(), labels.size(), hipMemcpyHostToDevice, st));
    XB_HIP(ctx, hipMemcpyAsync(d_len, tlen, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (int rc = stage_scores(ctx, scores, T, n, C)) return rc;
    if (d_gs) XB_HIP(ctx, hipMemsetAsync(d_gs, 0, sizeof(float) * (size_t)T * n * np, st));
    if (d_gm) XB_HIP(ctx, hipMemsetAsync(d_gm, 0, sizeof(float) * (size_t)T * n * nm, st));
    xb::CtcParams p{};
    p.scores = ctx->scores; p.T = T; p.N = n; p.C = C; p.targets = d_lab; p.Lt = Lt; p.nb = nb; p.tlen = d_len;
    p.sl = sl; p.semiring = semiring; p.alpha = d_alpha; p.logz = ctx->logz; p.gstay = d_gs; p.gmove = d_gm; p.error = ctx->error_data;
    XB_HIP(ctx, xb::launch_ctc_scan(p, st));
    if (logz) XB_HIP(ctx, hipMemcpyAsync(logz, ctx->logz, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (gstay) XB_HIP(ctx, hipMemcpyAsync(gstay, d_gs, sizeof(float) * (size_t)T * n * np, hipMemcpyDeviceToHost, st));
    if (gmove && np > 1) XB_HIP(ctx, hipMemcpyAsync(gmove, d_gm, sizeof(float) * (size_t)T * n * nm, hipMemcpyDeviceToHost, st));
    XB_HIP(ctx, hipStreamSynchronize(st));
    return check_device_error(ctx);
}

XB_API int xb_ctc_logz(xb_ctx *ctx, const float *scores, int T, int n, const int32_t *targets, int Lt,
                       const int32_t *target_lengths, float *logz, float *gstay, float *gmove)
{
    return run_ctc(ctx, scores, T, n, targets, Lt, target_lengths, 0, logz, gstay, gmove);
}

XB_API int xb_ctc_alignments(xb_ctx *ctx, const float *scores, int T, int n, const int32_t *targets, int Lt,
                             const int32_t *target_lengths, float *alignments, float *max_score)
{
    if (!alignments) return fail(ctx, XB_ERR_INVALID, "null host pointer");        // (before anything else, as it always was)
    return run_ctc(ctx, scores, T, n, targets, Lt, target_lengths, 1, max_score, alignments, nullptr);
}

// beam search over device-resident scores: the Log scans (alpha, beta, logZ) into the decode workspaces, then one wave per chunk
int run_beam(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, int ld, const char *alphabet, int beam_width,
             float beam_cut, float qscale, float qoffset, int8_t *d_seq, int8_t *d_q, uint8_t *d_moves, float *d_score)
{
    const xb_config &c = ctx->cfg;
    if (beam_width < 1 || beam_width > xb::BEAM_MAX_WIDTH)
        return fail(ctx, XB_ERR_INVALID, "beam_width %d outside [1, %d]", beam_width, xb::BEAM_MAX_WIDTH);
    // log(beam_cut) < 0: the maximum itself is below max - log(beam_cut), the front would be empty and the trace-back read history
    // that nobody wrote
    if (beam_cut > 0.0f && beam_cut < 1.0f)
        return fail(ctx, XB_ERR_INVALID, "beam_cut %g inside (0, 1): no candidate can reach it", (double)beam_cut);
    if (ctx->S > xb::BEAM_MAX_STATES) return fail(ctx, XB_ERR_INVALID, "beam search supports at most %d states", xb::BEAM_MAX_STATES);
    if (!alphabet || (int)strlen(alphabet) < c.n_base + 1) return fail(ctx, XB_ERR_INVALID, "alphabet needs %d symbols", c.n_base + 1);
    if (!ctx->beam_hist) {
        const size_t N = (size_t)c.max_batch, Tm = (size_t)ctx->T;
        DevPool &mem = ctx->mem_ctx;
        int rc = mem.alloc(ctx, &ctx->beam_hist, N * (Tm + 1) * xb::BEAM_MAX_WIDTH);
        rc = rc ? rc : mem.alloc(ctx, &ctx->beam_path, N * Tm);
        rc = rc ? rc : mem.alloc(ctx, &ctx->beam_prob, N * Tm);
        rc = rc ? rc : mem.alloc(ctx, &ctx->beam_score, N);
        rc = rc ? rc : mem.alloc(ctx, &ctx->beam_seq, N * Tm);
        rc = rc ? rc : mem.alloc(ctx, &ctx->beam_q, N * Tm);
        rc = rc ? rc : mem.alloc(ctx, &ctx->beam_moves, N * Tm);
        if (rc) { ctx->beam_hist = nullptr; return rc; }
    }
    ScanOut so;
    so.alpha = ctx->alpha; so.beta = ctx->beta; so.logz = ctx->logz;
    int rc = run_decode(ctx, d_scores, T, n, has_blank, ld, nullptr, nullptr, nullptr, nullptr, nullptr, &so);
    if (rc) return rc;
    xb::BeamParams p{};
    p.scores = d_scores; p.ld = ld; p.has_blank = has_blank; p.blank = c.blank_score;
    p.alpha = ctx->alpha; p.beta = ctx->beta; p.logz = ctx->logz;
    p.T = T; p.N = n; p.S = ctx->S; p.nb = c.n_base; p.hi = ctx->hi;
    p.W = beam_width;
    p.log_cut = beam_cut > 0.0f ? (float)log((double)beam_cut) : 3.402823466e+38f;
    p.qscale = qscale; p.qoffset = qoffset;
    memset(p.base_chars, 0, sizeof p.base_chars);
    memcpy(p.base_chars, alphabet + 1, (size_t)c.n_base);
    p.hist = ctx->beam_hist; p.path = ctx->beam_path; p.prob = ctx->beam_prob;
    p.seq = d_seq ? d_seq : ctx->beam_seq; p.qstr = d_q ? d_q : ctx->beam_q; p.moves = d_moves ? d_moves : ctx->beam_moves;
    p.score = d_seq ? d_score : ctx->beam_score;
    StageScope sc(ctx, XB_STAGE_DECODE, 1, ctx->stream);
    hipError_t e = xb::launch_beam_search(p, ctx->stream);
    if (e != hipSuccess) return fail(ctx, e == hipErrorInvalidValue ? XB_ERR_INVALID : XB_ERR_HIP, "beam search launch failed: %s", hipGetErrorString(e));
    return XB_OK;
}

XB_API int xb_beam_search_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const char *alphabet,
                              int beam_width, float beam_cut, float qscale, float qoffset, int8_t *d_sequence, int8_t *d_qstring,
                              uint8_t *d_moves, float *d_score)
{
    int ld = 0;
    if (int rc = score_args(ctx, "", T, n, has_blank, &ld)) return rc;
    if (!d_scores || !d_sequence || !d_qstring || !d_moves) return fail(ctx, XB_ERR_INVALID, "null device pointer");
    if (int rc = enter(ctx, true)) return rc;
    return run_beam(ctx, d_scores, T, n, has_blank ? 1 : 0, ld, alphabet, beam_width, beam_cut, qscale, qoffset, d_sequence,
                    d_qstring, d_moves, d_score);
}

// the three (n, T) byte planes and the optional path scores back to the host
int beam_results_to_host(xb_ctx *ctx, int T, int n, int8_t *sequence, int8_t *qstring, uint8_t *moves, float *score)
{
    const size_t nt = (size_t)n * T;
    XB_HIP(ctx, hipMemcpyAsync(sequence, ctx->beam_seq, nt, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(qstring, ctx->beam_q, nt, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(moves, ctx->beam_moves, nt, hipMemcpyDeviceToHost, ctx->stream));
    if (score) XB_HIP(ctx, hipMemcpyAsync(score, ctx->beam_score, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

XB_API int xb_beam_search(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const char *alphabet, int beam_width,
                          float beam_cut, float qscale, float qoffset, int8_t *sequence, int8_t *qstring, uint8_t *moves,
                          float *score)
{
    int ld = 0;
    if (int rc = score_args(ctx, "", T, n, has_blank, &ld)) return rc;
    if (!scores || !sequence || !qstring || !moves) return fail(ctx, XB_ERR_INVALID, "null host pointer");
    if (int rcj = enter(ctx, true)) return rcj;             // (a host form that has always named the main stream)
    if (int rcs = stage_scores(ctx, scores, T, n, ld)) return rcs;
    // the first call allocates the staging planes inside run_beam; pass them after the allocation
    int rc = run_beam(ctx, ctx->scores, T, n, has_blank ? 1 : 0, ld, alphabet, beam_width, beam_cut, qscale, qoffset, nullptr,
                      nullptr, nullptr, nullptr);
    if (rc) return rc;
    return beam_results_to_host(ctx, T, n, sequence, qstring, moves, score);
}

// ---- the validation loss and its gradient (xb_ctc_loss, xb_ctc_loss_grad): RAW scores where they lie, the labels as
// references.npy holds them; the _dev forms' rows are the kernel's to check ----
XB_API int xb_ctc_loss_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const uint8_t *d_targets, int Lt,
                           const int32_t *d_target_lengths, float *d_loss, float *d_logz)
{
    int ld = 0;
    if (int rc = score_args(ctx, "xb_ctc_loss: ", T, n, has_blank, &ld)) return rc;
    if (!d_scores || !d_targets || !d_target_lengths || !d_loss) return fail(ctx, XB_ERR_INVALID, "xb_ctc_loss: null device pointer");
    if (int rc = label_batch_check(ctx, "xb_ctc_loss", nullptr, n, Lt, nullptr)) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return ctc_loss_run(ctx, "xb_ctc_loss", d_scores, T, n, has_blank ? 1 : 0, ld, d_targets, Lt, d_target_lengths, d_loss, d_logz);
}

XB_API int xb_ctc_loss(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const uint8_t *targets, int Lt,
                       const int32_t *target_lengths, float *loss, float *logz)
{
    int ld = 0;
    if (int rc = score_args(ctx, "xb_ctc_loss: ", T, n, has_blank, &ld)) return rc;
    if (!scores || !targets || !target_lengths || !loss) return fail(ctx, XB_ERR_INVALID, "xb_ctc_loss: null host pointer");
    if (int rc = label_batch_check(ctx, "xb_ctc_loss", targets, n, Lt, target_lengths)) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t N = (size_t)n;
    Staging st{ctx};
    const LabelBatch lb(st, n, Lt);
    const auto d_logz = st.take<float>(N);
    if (int rc = st.ready()) return rc;
    if (int rc = stage_scores(ctx, scores, T, n, ld)) return rc;
    if (int rc = lb.upload(ctx, targets, target_lengths)) return rc;
    if (int rc = ctc_loss_run(ctx, "xb_ctc_loss", ctx->scores, T, n, has_blank ? 1 : 0, ld, lb.targets, Lt, lb.len, lb.loss, d_logz)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(loss, lb.loss, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (logz) XB_HIP(ctx, hipMemcpyAsync(logz, d_logz, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// the loss with d loss / d scores (the contract is in the public header)
XB_API int xb_ctc_loss_grad_dev(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, const uint8_t *d_targets, int Lt,
                                const int32_t *d_target_lengths, float loss_clip, int mean, float *d_loss, float *d_grad)
{
    int ld = 0;
    if (int rc = score_args(ctx, "xb_ctc_loss_grad: ", T, n, has_blank, &ld)) return rc;
    if (!d_scores || !d_targets || !d_target_lengths || !d_loss || !d_grad)
        return fail(ctx, XB_ERR_INVALID, "xb_ctc_loss_grad: null device pointer");
    if (int rc = label_batch_check(ctx, "xb_ctc_loss_grad", nullptr, n, Lt, nullptr)) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return ctc_grad_run(ctx, "xb_ctc_loss_grad", d_scores, T, n, has_blank ? 1 : 0, ld, d_targets, Lt, d_target_lengths, loss_clip, mean,
                        d_loss, d_grad);
}

XB_API int xb_ctc_loss_grad(xb_ctx *ctx, const float *scores, int T, int n, int has_blank, const uint8_t *targets, int Lt,
                            const int32_t *target_lengths, float loss_clip, int mean, float *loss, float *grad)
{
    int ld = 0;
    if (int rc = score_args(ctx, "xb_ctc_loss_grad: ", T, n, has_blank, &ld)) return rc;
    if (!scores || !targets || !target_lengths || !loss || !grad) return fail(ctx, XB_ERR_INVALID, "xb_ctc_loss_grad: null host pointer");
    if (int rc = label_batch_check(ctx, "xb_ctc_loss_grad", targets, n, Lt, target_lengths)) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t N = (size_t)n, cells = (size_t)T * N * ld;
    Staging st{ctx};
    const LabelBatch lb(st, n, Lt);
    const auto d_grad = st.take<float>(cells);
    if (int rc = st.ready()) return rc;
    if (int rc = stage_scores(ctx, scores, T, n, ld)) return rc;
    if (int rc = lb.upload(ctx, targets, target_lengths)) return rc;
    if (int rc = ctc_grad_run(ctx, "xb_ctc_loss_grad", ctx->scores, T, n, has_blank ? 1 : 0, ld, lb.targets, Lt, lb.len, loss_clip, mean,
                              lb.loss, d_grad))
        return rc;
    XB_HIP(ctx, hipMemcpyAsync(loss, lb.loss, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(grad, d_grad, sizeof(float) * cells, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}
