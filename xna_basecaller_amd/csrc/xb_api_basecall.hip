// xb_api_basecall.hip -- signal chunks to called bases through the C ABI: pairing (a held-back asynchronous basecall and its
// partner as one pass), the blocking and the asynchronous basecalls, the beam basecall, xb_validate_chunks, and the four-slot host
// pipeline.  The public header declares every XB_API function extern "C"; nothing else here is.
#include "xb_api_priv.h"

// room for two co-scheduled calls (once per context; everything in flight is waited for, no held call exists here)
static int reserve_pairing(xb_ctx *ctx)
{
    if (!ctx->fuse_ok) return XB_ERR_STATE;
    if (ctx->cap >= 2 * ctx->cfg.max_batch) return XB_OK;
    int rc = sync_all(ctx);
    if (rc) return rc;
    rc = alloc_workspaces(ctx, 2 * ctx->cfg.max_batch);
    if (rc) {                                           // out of memory: back to one call per pass for good
        ctx->fuse = ctx->fuse_ok = 0;
        const int rc2 = alloc_workspaces(ctx, ctx->cfg.max_batch);
        // (should even that fail the context has no workspaces left: cap == 0, and check_ready refuses every call)
        return rc2 ? rc2 : rc;
    }
    return XB_OK;
}

XB_API int xb_reserve_pairing(xb_ctx *ctx)
{
    if (!ctx) return XB_ERR_INVALID;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = flush_held(ctx)) return rc;
    if (!ctx->fuse_ok) return XB_OK;                    // this context does not pair calls: every call runs on its own
    const int rc = reserve_pairing(ctx);
    if (rc == XB_OK) ctx->fuse = 1;                     // from now on an asynchronous basecall may be held back for its partner
    return rc;                                          // (XB_ERR_NOMEM: no room for a pair; the context carries on unpaired)
}

XB_API int xb_pairing_active(const xb_ctx *ctx) { return ctx && ctx->fuse ? 1 : 0; }

// what follows a call's decode on its result stream: the host pipeline's D2H copies and done event, a deferred gather
static int call_post_actions(xb_ctx *ctx, const xb_ctx::Call &c, hipStream_t rs)
{
    if (c.slot >= 0) {
        xb_ctx::Slot &sl = ctx->slots[c.slot];
        if (int rc = copy_planes(ctx, c.out.level, sl.h, sl.d, 0, c.n, ctx->T, hipMemcpyDeviceToHost, rs)) return rc;
        // the sync word as THIS batch left it (stream order: behind its recurrences and its decode), not as whatever batch
        // happens to be running when the slot is collected finds it
        XB_HIP(ctx, hipMemcpyAsync(sl.h_err, ctx->error, sizeof(unsigned), hipMemcpyDeviceToHost, rs));
        XB_HIP(ctx, hipEventRecord(sl.done, rs));
    }
    if (c.after) c.after(c.after_arg);
    return XB_OK;
}

// The asynchronous basecall of one call, or of two calls as one batch (chunks [0, a.n) = a, [a.n, a.n + b->n) = b).
static int launch_calls(xb_ctx *ctx, const xb_ctx::Call &a, const xb_ctx::Call *b)
{
    const int n = a.n + (b ? b->n : 0);
    const float *sig2 = b ? b->signal : nullptr;
    // a pair (enqueue_call: the same level and calibration) decodes into the pair planes, which are then split
    const Planes fused = {{ctx->fseq, ctx->flen, ctx->q_fseq, ctx->q_fmoves, ctx->u_fprobs}};
    int8_t *d_seq = b ? ctx->fseq : a.seq;
    int32_t *d_len = b ? ctx->flen : a.len;
    DecodeOut out = a.out;
    if (b) { out.qstr = ctx->q_fseq; out.moves = ctx->q_fmoves; out.probs = ctx->u_fprobs; }
    int rc;
    hipStream_t rs;
    if (!ctx->knobs.overlap || !ctx->stream3 || !ctx->scores2 || !ctx->knobs.decode_async) {
        rs = ctx->result_stream = ctx->stream;
        ctx->last_scores = ctx->scores; ctx->last_n = n;
        rc = run_encoder(ctx, a.signal, n, 0, ctx->scores, ctx->ld_nb, sig2, a.n);
        if (rc) return rc;
        rc = run_decode(ctx, ctx->scores, ctx->T, n, 0, ctx->ld_nb, a.alphabet, nullptr, d_seq, d_len, nullptr, nullptr, &out);
        if (rc) return rc;
    } else {
        // asynchronous decode: the encoder of this batch writes score buffer p while the decode of the previous batch may
        // still be reading buffer p ^ 1 on the third stream; the decode that used buffer p two calls ago must be done first
        const int pb = (int)(ctx->batch_idx++ & 1u);
        float *sc = pb ? ctx->scores2 : ctx->scores;
        ctx->last_scores = sc; ctx->last_n = n;
        rs = ctx->result_stream = ctx->stream3;
        if (ctx->dec_pending[pb]) XB_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->dec_done[pb], 0));
        rc = run_encoder(ctx, a.signal, n, 0, sc, ctx->ld_nb, sig2, a.n);
        if (rc) return rc;
        hipEvent_t enc;
        if ((rc = next_dep(ctx, &enc))) return rc;
        XB_HIP(ctx, hipEventRecord(enc, ctx->stream));
        XB_HIP(ctx, hipStreamWaitEvent(ctx->stream3, enc, 0));
        rc = run_decode(ctx, sc, ctx->T, n, 0, ctx->ld_nb, a.alphabet, nullptr, d_seq, d_len, ctx->stream3, nullptr, &out);
        if (rc) return rc;
    }
    if (b) {        // the pair's rows back to where each caller wants them
        const int level = a.out.level;
        if ((rc = copy_planes(ctx, level, planes(a.seq, a.len, a.out), fused, 0, a.n, ctx->T, hipMemcpyDeviceToDevice, rs)))
            return rc;
        if ((rc = copy_planes(ctx, level, planes(b->seq, b->len, b->out), fused, a.n, b->n, ctx->T, hipMemcpyDeviceToDevice, rs)))
            return rc;
    }
    if (rs == ctx->stream3) {
        const int pb = (int)((ctx->batch_idx - 1) & 1u);
        XB_HIP(ctx, hipEventRecord(ctx->dec_done[pb], ctx->stream3));
        ctx->dec_pending[pb] = true;
    }
    if ((rc = call_post_actions(ctx, a, rs))) return rc;
    if (b && (rc = call_post_actions(ctx, *b, rs))) return rc;
    return XB_OK;
}

// launch a held-back call on its own (every entry point that is not the asynchronous basecall comes through here first)
int flush_held(xb_ctx *ctx)
{
    if (!ctx->holding || ctx->flushing) return XB_OK;
    ctx->flushing = true;
    const xb_ctx::Call h = ctx->held;
    ctx->holding = false;
    const int rc = launch_calls(ctx, h, nullptr);
    ctx->flushing = false;
    if (rc) {                                   // the call itself had already returned XB_OK
        ctx->pipeline_failed = true;
        ctx->deferred_rc = rc;                  // ... so the next call that can return a status reports it
    }
    return rc;
}

// Two calls share one pass only where it produces exactly what each produces alone: the same alphabet and output level (and
// at level >= 1 the same qscale / qoffset), different seq / qstring / probs buffers, at most 2 max_batch chunks, and the
// level's pair planes in place (enqueue_call then makes room for the pair's workspaces).
static bool can_pair(const xb_ctx *ctx, const xb_ctx::Call &h, const xb_ctx::Call &c)
{
    const DecodeOut &x = h.out, &y = c.out;
    if (!ctx->fuse || h.n + c.n > 2 * ctx->cfg.max_batch || strcmp(h.alphabet, c.alphabet) != 0 || h.seq == c.seq) return false;
    if (x.level != y.level) return false;
    if (x.level >= 1 && (x.qscale != y.qscale || x.qoffset != y.qoffset || x.qstr == y.qstr || !ctx->q_fseq)) return false;
    if (x.level == 2 && (x.probs == y.probs || !ctx->u_fprobs)) return false;
    return true;
}

static int enqueue_call(xb_ctx *ctx, const xb_ctx::Call &c)
{
    if (ctx->deferred_rc) {
        const int rc = ctx->deferred_rc;
        ctx->deferred_rc = 0;
        return rc;               // xb_last_error still holds the message of the launch that failed
    }
    if (ctx->holding) {
        const xb_ctx::Call h = ctx->held;
        ctx->holding = false;
        bool pair = can_pair(ctx, h, c);
        if (pair && h.n + c.n > ctx->cap && reserve_pairing(ctx) != XB_OK) pair = false;     // no room for both: one by one
        if (pair) {
            const int rc = launch_calls(ctx, h, &c);
            if (rc) ctx->pipeline_failed = true;
            return rc;
        }
        const int rc = launch_calls(ctx, h, nullptr);
        if (rc) { ctx->pipeline_failed = true; return rc; }
    }
    if (ctx->fuse) {
        ctx->held = c;
        ctx->holding = true;
        return XB_OK;
    }
    return launch_calls(ctx, c, nullptr);
}

int basecall_async(xb_ctx *ctx, const float *d_signal, int n, const char *alphabet, int8_t *seq, int32_t *len, const DecodeOut &out,
                   int slot)
{
    xb_ctx::Call c;
    c.signal = d_signal; c.n = n; c.seq = seq; c.len = len; c.slot = slot; c.out = out;
    strcpy(c.alphabet, alphabet);
    return enqueue_call(ctx, c);
}

XB_API int xb_basecall_chunks_dev(xb_ctx *ctx, const float *d_signal, int n, const char *alphabet, int8_t *d_seq,
                                  int32_t *d_seq_len)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    if (!d_signal || !d_seq || !alphabet) return fail(ctx, XB_ERR_INVALID, "null argument");
    if ((rc = check_alphabet(ctx, alphabet))) return rc;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    return basecall_async(ctx, d_signal, n, alphabet, d_seq, d_seq_len, {});
}

// the blocking basecalls: through the context's staging, and back to the host
static int basecall_host(xb_ctx *ctx, const float *signal, int n, const char *alphabet, int8_t *seq, int32_t *seq_len,
                         const DecodeOut &o)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    const Planes dst = planes(seq, seq_len, o);
    if (!signal || !has_required(dst, o.level) || !alphabet) return fail(ctx, XB_ERR_INVALID, "null argument");
    if ((rc = check_alphabet(ctx, alphabet))) return rc;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (o.level && (rc = ensure_staging(ctx, o.level))) return rc;
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * (size_t)n * ctx->cfg.chunk_len,
                               hipMemcpyHostToDevice, ctx->stream));
    const DecodeOut d = staging_of(ctx, o);
    if ((rc = basecall_async(ctx, ctx->d_signal, n, alphabet, ctx->seq, ctx->seq_len, d))) return rc;
    if ((rc = join_async_decode(ctx))) return rc;
    if ((rc = copy_planes(ctx, o.level, dst, planes(ctx->seq, ctx->seq_len, d), 0, n, ctx->T, hipMemcpyDeviceToHost, ctx->stream)))
        return rc;
    return xb_synchronize(ctx);
}

XB_API int xb_basecall_chunks(xb_ctx *ctx, const float *signal, int n, const char *alphabet, int8_t *seq,
                              int32_t *seq_len)
{
    return basecall_host(ctx, signal, n, alphabet, seq, seq_len, {});
}

XB_API int xb_basecall_chunks_q(xb_ctx *ctx, const float *signal, int n, const char *alphabet, float qscale, float qoffset,
                                int8_t *seq, int8_t *qstring, uint8_t *moves, int32_t *seq_len)
{
    return basecall_host(ctx, signal, n, alphabet, seq, seq_len, {1, qscale, qoffset, qstring, moves});
}

XB_API int xb_basecall_chunks_ub(xb_ctx *ctx, const float *signal, int n, const char *alphabet, float qscale, float qoffset,
                                 int8_t *seq, int8_t *qstring, uint8_t *moves, uint8_t *probs, int32_t *seq_len)
{
    return basecall_host(ctx, signal, n, alphabet, seq, seq_len, {2, qscale, qoffset, qstring, moves, probs});
}

// a slot's staging, lazily (most contexts -- tests, bench -- never use the host pipeline): the signal, and the planes of an
// output level on the slot's first submission at that level
static int ensure_slot(xb_ctx *ctx, int slot, int level)
{
    xb_ctx::Slot &sl = ctx->slots[slot];
    const size_t N = ctx->cfg.max_batch, L = ctx->cfg.chunk_len;
    if (!sl.h_signal) {
        if (!ctx->stream_copy) XB_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream_copy, hipStreamNonBlocking));
        XB_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&sl.h_signal), sizeof(float) * N * L, hipHostMallocDefault));
        XB_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&sl.h_err), sizeof(unsigned), hipHostMallocDefault));
        if (int rc = ctx->mem_ctx.alloc(ctx, &sl.d_signal, N * L)) return rc;
        XB_HIP(ctx, hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
        XB_HIP(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    for (int i = 0; i < plane_count(level); ++i) {
        const size_t bytes = N * plane_bytes(ctx->T, ctx->cfg.n_base, i);
        if (!sl.h.p[i]) XB_HIP(ctx, hipHostMalloc(&sl.h.p[i], bytes, hipHostMallocDefault));
        if (!sl.d.p[i]) {
            uint8_t *p = nullptr;
            if (int rc = ctx->mem_ctx.alloc(ctx, &p, bytes)) return rc;
            sl.d.p[i] = p;
        }
    }
    return level ? ensure_staging(ctx, level) : XB_OK;
}

static int submit_chunks(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet, const DecodeOut &o)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    if (slot < 0 || slot >= XB_PIPELINE_SLOTS || !signal || !alphabet) return fail(ctx, XB_ERR_INVALID, "bad slot / null argument");
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_slot(ctx, slot, o.level))) return rc;
    xb_ctx::Slot &sl = ctx->slots[slot];
    if (sl.busy) return fail(ctx, XB_ERR_STATE, "slot %d was submitted and not collected", slot);
    const size_t bytes = sizeof(float) * (size_t)n * ctx->cfg.chunk_len;
    memcpy(sl.h_signal, signal, bytes);                       // the caller's buffer is free again on return
    XB_HIP(ctx, hipMemcpyAsync(sl.d_signal, sl.h_signal, bytes, hipMemcpyHostToDevice, ctx->stream_copy));
    XB_HIP(ctx, hipEventRecord(sl.h2d, ctx->stream_copy));
    XB_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.h2d, 0));
    if ((rc = check_alphabet(ctx, alphabet))) return rc;
    // the D2H copies of the results, the error-word snapshot and the slot's done event follow the launch of this call
    // (call_post_actions) -- which may be held back until the next submit so that the two batches share one pass
    DecodeOut d = o;
    d.qstr = static_cast<int8_t *>(sl.d.p[2]); d.moves = static_cast<uint8_t *>(sl.d.p[3]); d.probs = static_cast<uint8_t *>(sl.d.p[4]);
    rc = basecall_async(ctx, sl.d_signal, n, alphabet, static_cast<int8_t *>(sl.d.p[0]), static_cast<int32_t *>(sl.d.p[1]), d, slot);
    if (rc) return rc;
    sl.n = n;
    sl.busy = true;
    sl.level = o.level;
    return XB_OK;
}

XB_API int xb_submit_chunks(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet)
{
    return submit_chunks(ctx, slot, signal, n, alphabet, {});
}

XB_API int xb_submit_chunks_q(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet, float qscale,
                              float qoffset)
{
    return submit_chunks(ctx, slot, signal, n, alphabet, {1, qscale, qoffset});
}

XB_API int xb_submit_chunks_ub(xb_ctx *ctx, int slot, const float *signal, int n, const char *alphabet, float qscale,
                               float qoffset)
{
    return submit_chunks(ctx, slot, signal, n, alphabet, {2, qscale, qoffset});
}

// collects the planes of an output level: a submission at that level or above (below: XB_ERR_STATE)
static int collect_chunks(xb_ctx *ctx, int slot, int level, const Planes &dst)
{
    static const char *const none_in_flight[3] = {"slot %d has nothing in flight", "slot %d has no submission with qualities in flight",
                                                  "slot %d has no submission with letter probabilities in flight"};
    if (!ctx) return XB_ERR_INVALID;
    if (slot < 0 || slot >= XB_PIPELINE_SLOTS || !has_required(dst, level)) return fail(ctx, XB_ERR_INVALID, "bad slot / null argument");
    xb_ctx::Slot &sl = ctx->slots[slot];
    if (!sl.busy || sl.level < level) return fail(ctx, XB_ERR_STATE, none_in_flight[level], slot);
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->holding && ctx->held.slot == slot) (void)flush_held(ctx);      // a failure shows as pipeline_failed below
    XB_HIP(ctx, hipEventSynchronize(sl.done));
    sl.busy = false;
    for (int i = 0; i < plane_count(level); ++i)
        if (dst.p[i]) memcpy(dst.p[i], sl.h.p[i], (size_t)sl.n * plane_bytes(ctx->T, ctx->cfg.n_base, i));
    // the persistent recurrence reports a lost rendezvous through the sync word (snapshot taken behind this batch):
    // results would be garbage.  The word is not cleared while another batch is in flight -- that batch fails too (it ran
    // on a device in an unknown state) -- and is reset once the pipeline has drained.  The data word is not looked at: a
    // refused label of some loss call says nothing about this batch, and the next synchronising call reports it.
    if (*sl.h_err != 0) ctx->pipeline_failed = true;
    if (ctx->pipeline_failed) {
        bool any_busy = false;
        for (auto &s2 : ctx->slots) any_busy = any_busy || s2.busy;
        if (!any_busy) {
            (void)sync_all(ctx);
            (void)hipMemset(ctx->error, 0, sizeof(unsigned));
            ctx->pipeline_failed = false;
        }
        const xb::DeviceStatus lost = xb::decode_status(xb::SYNC_LOST, 0u);
        return fail(ctx, lost.code, "%s", lost.message);
    }
    return XB_OK;
}

XB_API int xb_collect_chunks_ub(xb_ctx *ctx, int slot, int8_t *seq, int32_t *seq_len, int8_t *qstring, uint8_t *moves,
                                uint8_t *probs)
{
    return collect_chunks(ctx, slot, 2, {{seq, seq_len, qstring, moves, probs}});
}

XB_API int xb_collect_chunks_q(xb_ctx *ctx, int slot, int8_t *seq, int32_t *seq_len, int8_t *qstring, uint8_t *moves)
{
    return collect_chunks(ctx, slot, 1, {{seq, seq_len, qstring, moves, nullptr}});
}

XB_API int xb_collect_chunks(xb_ctx *ctx, int slot, int8_t *seq, int32_t *seq_len)
{
    return collect_chunks(ctx, slot, 0, {{seq, seq_len, nullptr, nullptr, nullptr}});
}

// signal chunks -> encoder (scores without the blank column, as the reference's beam branch sees them) -> beam search
XB_API int xb_basecall_chunks_beam(xb_ctx *ctx, const float *signal, int n, const char *alphabet, int beam_width, float beam_cut,
                                   float qscale, float qoffset, int8_t *sequence, int8_t *qstring, uint8_t *moves, float *score)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    if (!signal || !sequence || !qstring || !moves || !alphabet) return fail(ctx, XB_ERR_INVALID, "null argument");
    if ((rc = enter(ctx, true))) return rc;                 // (a host form that has always named the main stream)
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * (size_t)n * ctx->cfg.chunk_len, hipMemcpyHostToDevice,
                               ctx->stream));
    rc = run_encoder(ctx, ctx->d_signal, n, 0, ctx->scores, ctx->ld_nb);
    if (rc) return rc;
    rc = run_beam(ctx, ctx->scores, ctx->T, n, 0, ctx->ld_nb, alphabet, beam_width, beam_cut, qscale, qoffset, nullptr, nullptr,
                  nullptr, nullptr);
    if (rc) return rc;
    return beam_results_to_host(ctx, ctx->T, n, sequence, qstring, moves, score);
}

// validate_one_step's device half: signal -> encoder (blank-less scores) -> Viterbi decode, as xb_basecall_chunks runs them, then the
// loss from the scores the decode read
XB_API int xb_validate_chunks(xb_ctx *ctx, const float *signal, int n, const char *alphabet, const uint8_t *targets, int Lt,
                              const int32_t *target_lengths, int8_t *seq, int32_t *seq_len, float *loss)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    if (!signal || !alphabet || !targets || !target_lengths || !seq || !seq_len || !loss)
        return fail(ctx, XB_ERR_INVALID, "xb_validate_chunks: null argument");
    if ((rc = check_alphabet(ctx, alphabet))) return rc;
    if ((rc = label_batch_check(ctx, "xb_validate_chunks", targets, n, Lt, target_lengths))) return rc;
    // nothing held back may pair with this call: its scores are read where the encoder left them, as a batch of their own
    if ((rc = enter(ctx, false))) return rc;
    const size_t N = (size_t)n, W = (size_t)ctx->T;
    Staging st{ctx};
    const LabelBatch lb(st, n, Lt);
    if ((rc = st.ready())) return rc;
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * N * ctx->cfg.chunk_len, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = lb.upload(ctx, targets, target_lengths))) return rc;
    if ((rc = basecall_async(ctx, ctx->d_signal, n, alphabet, ctx->seq, ctx->seq_len, {}))) return rc;
    if ((rc = join_async_decode(ctx))) return rc;
    if (!ctx->last_scores || ctx->last_n != n) return fail(ctx, XB_ERR_STATE, "xb_validate_chunks: the pass of %d chunks left no scores of its own", n);
    if ((rc = ctc_loss_run(ctx, "xb_validate_chunks", ctx->last_scores, ctx->T, n, 0, ctx->ld_nb, lb.targets, Lt, lb.len, lb.loss, nullptr)))
        return rc;
    XB_HIP(ctx, hipMemcpyAsync(seq, ctx->seq, N * W, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(seq_len, ctx->seq_len, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(loss, lb.loss, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}
