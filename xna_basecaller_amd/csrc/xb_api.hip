// xb_api.hip -- the context core of the C ABI of libxnacall.so (see include/xna_basecaller.h for the contract and the reference
// call sites each entry point replaces): a context's lifetime and weights, what every entry point shares (fail, check_ready,
// enter, the status words, the workspaces), profiling, the debug calls and the host-logic exports.  The calls themselves live in
// xb_run_encoder.hip, xb_api_scores.hip, xb_api_basecall.hip and xb_api_data.hip.
#include "xb_api_priv.h"

namespace { thread_local std::string g_create_error; }

int fail(const xb_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

int check_ready(xb_ctx *ctx, int n)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!ctx->weights_ready) return fail(ctx, XB_ERR_STATE, "weights not loaded: call xb_load_weights for all 28 tensors, then xb_weights_ready");
    if (n < 1 || n > ctx->cfg.max_batch) return fail(ctx, XB_ERR_INVALID, "batch %d outside [1, max_batch=%d]", n, ctx->cfg.max_batch);
    if (ctx->cap < ctx->cfg.max_batch) return fail(ctx, XB_ERR_NOMEM, "the context lost its workspaces (a reallocation failed)");
    return XB_OK;
}

// every entry point except the asynchronous basecall first orders the main stream behind decodes still in flight on the
// third stream (they share the decode workspaces and the score buffers)
int join_async_decode(xb_ctx *ctx)
{
    if (int rc = flush_held(ctx)) return rc;
    for (int p = 0; p < 2; ++p)
        if (ctx->dec_pending[p]) {
            XB_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->dec_done[p], 0));
            ctx->dec_pending[p] = false;
        }
    return XB_OK;
}

// result_stream is named last: launching a held-back call names its own
int enter(xb_ctx *ctx, bool dev)
{
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = join_async_decode(ctx)) return rc;
    if (dev) ctx->result_stream = ctx->stream;
    return XB_OK;
}

int check_alphabet(xb_ctx *ctx, const char *alphabet)
{
    if ((int)strlen(alphabet) < ctx->cfg.n_base + 1 || strlen(alphabet) >= sizeof(xb_ctx::Call{}.alphabet))
        return fail(ctx, XB_ERR_INVALID, "alphabet needs %d symbols", ctx->cfg.n_base + 1);
    return XB_OK;
}

// The workspaces whose size follows the number of chunks in a pass.  A context starts with room for max_batch chunks; the
// first time two calls are co-scheduled (or on xb_reserve_pairing) they are replaced by twice that.
int alloc_workspaces(xb_ctx *ctx, int cap)
{
    DevPool &ws = ctx->mem_ws;
    ws.release();
    ctx->cap = 0;
    // nothing of an earlier pass lies in the new workspaces: no layer outputs in x_hi / x_lo, no scores to validate from
    ctx->enc_n = 0;
    ctx->last_scores = nullptr;
    ctx->last_n = 0;
    const xb_config *cfg = &ctx->cfg;
    const int S = ctx->S;
    const size_t N = (size_t)cap, T = ctx->T, F = cfg->features, L = cfg->chunk_len;
    const size_t Cb = (size_t)S * (cfg->n_base + 1);
    const size_t Cmax = Cb > (size_t)ctx->ld_nb ? Cb : (size_t)ctx->ld_nb;
    int rc = XB_OK;
    rc = rc ? rc : ws.alloc(ctx, &ctx->d_signal, N * L);
    rc = rc ? rc : ws.alloc(ctx, &ctx->im_hi, T * N * ctx->kp);
    rc = rc ? rc : ws.alloc(ctx, &ctx->im_lo, T * N * ctx->kp);
    for (int i = 0; i < 2 && !rc; ++i) {
        rc = rc ? rc : ws.alloc(ctx, &ctx->x_hi[i], T * N * F);
        rc = rc ? rc : ws.alloc(ctx, &ctx->x_lo[i], T * N * F);
    }
    // + 64 rows: the recurrence's LDS-DMA of a ragged last group reads (and ignores) up to 63 rows past the last chunk
    rc = rc ? rc : ws.alloc(ctx, &ctx->gin, (T * N + 64) * 4 * F);
    if (ctx->knobs.overlap) rc = rc ? rc : ws.alloc(ctx, &ctx->gin2, (T * N + 64) * 4 * F);
    rc = rc ? rc : ws.alloc(ctx, &ctx->c_state, N * F);
    rc = rc ? rc : ws.alloc(ctx, &ctx->scores, T * N * Cmax);
    if (ctx->knobs.overlap && ctx->knobs.decode_async) rc = rc ? rc : ws.alloc(ctx, &ctx->scores2, T * N * (size_t)ctx->ld_nb);
    rc = rc ? rc : ws.alloc(ctx, &ctx->alpha, (T + 1) * N * S);
    rc = rc ? rc : ws.alloc(ctx, &ctx->beta, (T + 1) * N * S);
    rc = rc ? rc : ws.alloc(ctx, &ctx->bmax, (T + 1) * N * S);
    rc = rc ? rc : ws.alloc(ctx, &ctx->logz, N);
    rc = rc ? rc : ws.alloc(ctx, &ctx->qbuf, T * N * ((Cb + 3) & ~(size_t)3));
    rc = rc ? rc : ws.alloc(ctx, &ctx->labels, N * T);
    rc = rc ? rc : ws.alloc(ctx, &ctx->seq, N * T);
    rc = rc ? rc : ws.alloc(ctx, &ctx->seq_len, N);
    if (ctx->fuse_ok) {      // results of a pair before they are split (two short calls can pair inside max_batch chunks)
        rc = rc ? rc : ws.alloc(ctx, &ctx->fseq, N * T);
        rc = rc ? rc : ws.alloc(ctx, &ctx->flen, N);
    }
    if (!rc) ctx->cap = cap;
    return rc;
}

namespace {

int collect_events(xb_ctx *ctx)
{
    for (auto &ev : ctx->events) {
        float ms = 0.f;
        if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess)
            ctx->stage_ms[ev.stage] += ms;
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    ctx->events.clear();
    return XB_OK;
}

// expected element count of each state-dict tensor
int64_t expected_size(const xb_ctx *c, const std::string &name)
{
    const int64_t F = c->cfg.features, W = c->cfg.winlen;
    if (name == "encoder.0.conv.weight") return 4 * 1 * 5;
    if (name == "encoder.0.conv.bias") return 4;
    if (name == "encoder.1.conv.weight") return 16 * 4 * 5;
    if (name == "encoder.1.conv.bias") return 16;
    if (name == "encoder.2.conv.weight") return F * 16 * W;
    if (name == "encoder.2.conv.bias") return F;
    for (int l = 4; l <= 8; ++l) {
        const std::string pre = "encoder." + std::to_string(l) + ".rnn.";
        if (name == pre + "weight_ih_l0" || name == pre + "weight_hh_l0") return 4 * F * F;
        if (name == pre + "bias_ih_l0" || name == pre + "bias_hh_l0") return 4 * F;
    }
    if (name == "encoder.9.linear.weight") return (int64_t)c->O * F;
    if (name == "encoder.9.linear.bias") return c->O;
    return -1;
}

// weight upload: the allocation belongs to the current weight set (ctx->mem_w), which the next xb_weights_ready releases
template <typename Tp>
int upload(xb_ctx *ctx, Tp **dst, const std::vector<Tp> &src)
{
    if (int rc = ctx->mem_w.alloc(ctx, dst, src.size())) return rc;
    XB_HIP(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(Tp), hipMemcpyHostToDevice));
    return XB_OK;
}

}  // namespace

// What the two status words say once the main stream has drained (xb_status.h): one condition per call, and that one is taken
// out of its word -- a validation bit beside it is the next synchronising call's to report.
int check_device_error(xb_ctx *ctx)
{
    unsigned w[xb_ctx::STATUS_DATA_AT + 1] = {};
    XB_HIP(ctx, hipMemcpyAsync(w, ctx->error, sizeof w, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned sync_word = w[0], data_word = w[xb_ctx::STATUS_DATA_AT];
    const xb::DeviceStatus s = xb::decode_status(sync_word, data_word);
    if (s.code == XB_OK) return XB_OK;
    if (s.sync_left != sync_word) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->error), (int)s.sync_left, 1, ctx->stream);
    if (s.data_left != data_word) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->error_data), (int)s.data_left, 1, ctx->stream);
    return fail(ctx, s.code, "%s", s.message);
}

int next_dep(xb_ctx *ctx, hipEvent_t *ev)
{
    if (ctx->dep_next == ctx->deps.size()) {
        hipEvent_t e;
        XB_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->deps.push_back(e);
    }
    *ev = ctx->deps[ctx->dep_next++];
    return XB_OK;
}

int sync_all(xb_ctx *ctx)
{
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) XB_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    if (ctx->stream3) XB_HIP(ctx, hipStreamSynchronize(ctx->stream3));
    ctx->dec_pending[0] = ctx->dec_pending[1] = false;
    return XB_OK;
}

extern "C" {

XB_API const char *xb_version(void) { return "xnacall 0.1.0 (gfx950)"; }

XB_API int xb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

XB_API const char *xb_last_error(const xb_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

XB_API int xb_ctx_create(xb_ctx **out, int device, const xb_config *cfg)
{
    if (!out || !cfg) return fail(nullptr, XB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->n_base < 4 || cfg->n_base > 6) return fail(nullptr, XB_ERR_INVALID, "n_base %d not in {4,5,6}", cfg->n_base);
    if (cfg->state_len < 2 || cfg->state_len > 5) return fail(nullptr, XB_ERR_INVALID, "state_len %d not in [2,5]", cfg->state_len);
    const int64_t S = ipow(cfg->n_base, cfg->state_len);
    if (S > 1024) return fail(nullptr, XB_ERR_INVALID, "n_base^state_len = %lld exceeds 1024 states", (long long)S);
    if (!xb::lstm_supported_features(cfg->features))
        return fail(nullptr, XB_ERR_INVALID, "features %d unsupported (32,64,96,128,256,384,512,768)", cfg->features);
    if (cfg->winlen < 1 || cfg->winlen > 31 || cfg->winlen % 2 == 0 || cfg->stride < 1 || cfg->stride > 8)
        return fail(nullptr, XB_ERR_INVALID, "winlen %d / stride %d unsupported", cfg->winlen, cfg->stride);
    if (cfg->chunk_len < cfg->stride || cfg->max_batch < 1) return fail(nullptr, XB_ERR_INVALID, "bad chunk_len/max_batch");
    if (cfg->precision < XB_PREC_F16X3 || cfg->precision > XB_PREC_MIXED) return fail(nullptr, XB_ERR_INVALID, "bad precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, XB_ERR_NO_GPU, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(nullptr, XB_ERR_INVALID, "device %d out of range (%d devices)", device, ndev);

    xb_ctx *ctx = new (std::nothrow) xb_ctx();
    if (!ctx) return fail(nullptr, XB_ERR_NOMEM, "out of host memory");
    ctx->cfg = *cfg;
    ctx->device = device;
    const int pad = cfg->winlen / 2;
    ctx->T = (cfg->chunk_len + 2 * pad - cfg->winlen) / cfg->stride + 1;
    ctx->S = (int)S;
    ctx->hi = (int)ipow(cfg->n_base, cfg->state_len - 1);
    ctx->O = (int)(S * cfg->n_base);
    ctx->kp = (16 * cfg->winlen + 31) & ~31;
    ctx->ld_nb = (ctx->O + 3) & ~3;
    {
        xb::Knobs k;
        k.lstm_mode = cfg->lstm_mode;
        ctx->knobs = xb::knobs_from_env(k);
    }
    set_stage_arithmetic(ctx, ctx->knobs.x3_stages >= 0 ? ctx->knobs.x3_stages : (cfg->precision == XB_PREC_MIXED ? X3_MIXED_STAGES : 0));

#define XB_CREATE_HIP(call)                                                                   \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            int rc_ = fail(nullptr, XB_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
            xb_ctx_destroy(ctx);                                                              \
            return rc_;                                                                       \
        }                                                                                     \
    } while (0)
    XB_CREATE_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    XB_CREATE_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        int rc = fail(nullptr, XB_ERR_NO_GPU, "device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
        xb_ctx_destroy(ctx);
        return rc;
    }
    ctx->cu_count = prop.multiProcessorCount;
    {
        int least = 0, greatest = 0;
        XB_CREATE_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        XB_CREATE_HIP(hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest));
        XB_CREATE_HIP(hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, least));
        // (a high-priority decode stream was measured: no difference, 6.64 vs 6.69 ms per decode, 125.0 vs 124.7 ms per step)
        XB_CREATE_HIP(hipStreamCreateWithPriority(&ctx->stream3, hipStreamNonBlocking, least));
        for (int p = 0; p < 2; ++p) XB_CREATE_HIP(hipEventCreateWithFlags(&ctx->dec_done[p], hipEventDisableTiming));
        // rocprofv3 counter collection (--pmc) runs one kernel at a time; hipStreamWaitValue32 is a spinning kernel
        // (__amd_rocclr_streamOpsWait) there, which would wait for a flag the serialised recurrence can never raise: slab launches
        if (xb::counter_collection_from_env()) ctx->knobs.lstm_signal = 0;
    }

    // co-scheduling two calls: only where the pair fits one launch of two groups per workgroup
    ctx->fuse_ok = ctx->knobs.fuse && ctx->knobs.overlap == 1 && ctx->knobs.lstm_dual != 0 &&
                   cfg->max_batch <= xb::pair_capacity(cfg->features, ctx->cu_count, ctx->knobs.lstm_wide);
    const size_t F = cfg->features;
    int rc = alloc_workspaces(ctx, cfg->max_batch);
    rc = rc ? rc : ctx->mem_ctx.alloc(ctx, &ctx->xh, (size_t)64 * 2 * 2 * 64 * F);
    rc = rc ? rc : ctx->mem_ctx.alloc(ctx, &ctx->sync, (size_t)SYNC_SLOTS * 32 + 32 + 64);      // group slots, status words, slab arrival counters
    if (rc) {
        g_create_error = ctx->err;
        xb_ctx_destroy(ctx);
        return rc;
    }
    static_assert(xb_ctx::STATUS_DATA_AT * sizeof(unsigned) >= 64 && xb_ctx::STATUS_DATA_AT < 32, "the status words: two 64-byte lines of the 32 words");
    ctx->error = ctx->sync + SYNC_SLOTS * 32;
    ctx->error_data = ctx->error + xb_ctx::STATUS_DATA_AT;
    XB_CREATE_HIP(hipMemset(ctx->sync, 0, sizeof(unsigned) * (SYNC_SLOTS * 32 + 32 + 64)));
    ctx->sig_done = ctx->sync + SYNC_SLOTS * 32 + 32;
    if (ctx->knobs.lstm_signal) {
        int can = 0;
        if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess || !can) {
            ctx->knobs.lstm_signal = 0;
        } else {
            // signal memory where the device has it, plain device memory otherwise; owned like everything else of the context
            DevBuf flag;
            if (hipExtMallocWithFlags(&flag.p, 8, hipMallocSignalMemory) == hipSuccess) {
                flag.bytes = 8;
            } else {
                (void)hipGetLastError();
                flag.p = nullptr;
                if (flag.alloc(ctx, 8)) (void)hipGetLastError();
            }
            if (flag.p) {
                ctx->sig_flag = static_cast<unsigned *>(flag.p);
                ctx->mem_ctx.bufs.push_back(std::move(flag));
                XB_CREATE_HIP(hipMemset(ctx->sig_flag, 0, 8));
            } else {
                ctx->knobs.lstm_signal = 0;
            }
        }
    }
#undef XB_CREATE_HIP
    *out = ctx;
    return XB_OK;
}

XB_API void xb_ctx_destroy(xb_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // a call nobody waited for: launch it all the same -- its deferred gather (xb_gather_called) is a collective the other ranks
    // enter too, and the streams are drained below before anything is freed
    if (ctx->holding && ctx->weights_ready && ctx->cap > 0) (void)flush_held(ctx);
    ctx->holding = false;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    for (auto &e : ctx->dec_done) if (e) (void)hipEventDestroy(e);
    for (auto &sl : ctx->slots) {
        if (sl.h_signal) (void)hipHostFree(sl.h_signal);
        if (sl.h_err) (void)hipHostFree(sl.h_err);
        for (void *h : sl.h.p) if (h) (void)hipHostFree(h);
        if (sl.h2d) (void)hipEventDestroy(sl.h2d);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (ctx->stream_copy) { (void)hipStreamSynchronize(ctx->stream_copy); (void)hipStreamDestroy(ctx->stream_copy); }
    for (auto &e : ctx->deps) (void)hipEventDestroy(e);
    for (auto &ev : ctx->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto &o : ctx->dtw.off) {
        if (o.h) (void)hipHostFree(o.h);
        if (o.copied) (void)hipEventDestroy(o.copied);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    delete ctx;      // every DevBuf and DevPool of the context frees its device memory here: the device is set, nothing is in flight
}

XB_API int xb_load_weights(xb_ctx *ctx, const char *name, const float *host, int64_t n)
{
    if (!ctx || !name || !host) return fail(ctx, XB_ERR_INVALID, "null argument");
    const int64_t want = expected_size(ctx, name);
    if (want < 0) return fail(ctx, XB_ERR_INVALID, "unknown state-dict key '%s'", name);
    if (want != n) return fail(ctx, XB_ERR_INVALID, "'%s': got %lld elements, config implies %lld", name, (long long)n, (long long)want);
    if (ctx->head.open) return fail(ctx, XB_ERR_STATE, "xb_load_weights: a head trainer is open on this context; call xb_head_train_end first");
    // a held-back basecall belongs to the weights it was called with (loading clears weights_ready, the launch needs it)
    if (ctx->holding) {
        XB_HIP(ctx, hipSetDevice(ctx->device));
        if (int rc = flush_held(ctx)) return rc;
    }
    ctx->host_w[name].assign(host, host + n);
    ctx->weights_ready = false;
    return XB_OK;
}

XB_API int xb_weights_ready(xb_ctx *ctx)
{
    if (!ctx) return XB_ERR_INVALID;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (int rcf = flush_held(ctx)) return rcf;          // with the weights it was called with
    const int F = ctx->cfg.features, W = ctx->cfg.winlen;
    auto need = [&](const std::string &k) -> const std::vector<float> * {
        auto it = ctx->host_w.find(k);
        return it == ctx->host_w.end() ? nullptr : &it->second;
    };
    std::vector<std::string> keys = {"encoder.0.conv.weight", "encoder.0.conv.bias", "encoder.1.conv.weight",
                                     "encoder.1.conv.bias", "encoder.2.conv.weight", "encoder.2.conv.bias",
                                     "encoder.9.linear.weight", "encoder.9.linear.bias"};
    for (int l = 4; l <= 8; ++l)
        for (const char *s : {"weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"})
            keys.push_back("encoder." + std::to_string(l) + ".rnn." + s);
    for (auto &k : keys)
        if (!need(k)) return fail(ctx, XB_ERR_STATE, "missing tensor '%s'", k.c_str());
    // a second load_state_dict on a live context: nothing may still be reading the previous weight set
    if (!ctx->mem_w.empty()) {
        if (int rcs = sync_all(ctx)) return rcs;
        ctx->mem_w.release();
    }

    int rc;
    if ((rc = upload(ctx, &ctx->w1, *need("encoder.0.conv.weight")))) return rc;
    if ((rc = upload(ctx, &ctx->b1, *need("encoder.0.conv.bias")))) return rc;
    if ((rc = upload(ctx, &ctx->w2, *need("encoder.1.conv.weight")))) return rc;
    if ((rc = upload(ctx, &ctx->b2, *need("encoder.1.conv.bias")))) return rc;
    if ((rc = upload(ctx, &ctx->b3, *need("encoder.2.conv.bias")))) return rc;
    std::vector<half_t> hi, lo;
    // every weight tensor in the form its stage's arithmetic reads (q8 image for nsplit 2, fp16 residual for 3)
    xb::split_rows(need("encoder.2.conv.weight")->data(), F, 16 * W, ctx->kp, hi, lo, ctx->ns_conv == 2 ? &ctx->w3_exp : nullptr);
    if ((rc = upload(ctx, &ctx->w3_hi, hi))) return rc;
    if ((rc = upload(ctx, &ctx->w3_lo, lo))) return rc;
    std::vector<unsigned char> f4;
    xb::fragment_major(hi, lo, F, ctx->kp, ctx->kp, ctx->ns_conv, f4, &ctx->w3_ks);
    if ((rc = upload(ctx, &ctx->w3_f4, f4))) return rc;
    for (int l = 0; l < 5; ++l) {
        const std::string pre = "encoder." + std::to_string(4 + l) + ".rnn.";
        const float *wih = need(pre + "weight_ih_l0")->data(), *whh = need(pre + "weight_hh_l0")->data();
        const float *bih = need(pre + "bias_ih_l0")->data(), *bhh = need(pre + "bias_hh_l0")->data();
        std::vector<float> wi, wh, bb;
        xb::gate_interleave(wih, whh, bih, bhh, F, wi, wh, bb);
        xb::split_rows(wi.data(), 4 * F, F, F, hi, lo, ctx->ns_in[l] == 2 ? &ctx->wih_exp[l] : nullptr);
        if ((rc = upload(ctx, &ctx->wih_hi[l], hi))) return rc;
        if ((rc = upload(ctx, &ctx->wih_lo[l], lo))) return rc;
        xb::fragment_major(hi, lo, 4 * F, F, F, ctx->ns_in[l], f4, &ctx->wih_ks);       // (the k-tile stride is the same for nsplit 2 and 3)
        if ((rc = upload(ctx, &ctx->wih_f4[l], f4))) return rc;
        if (ctx->cfg.precision == XB_PREC_F16F8_IN1) {
            xb::fragment_major(hi, lo, 4 * F, F, F, 1, f4, &ctx->wih_ksh);
            if ((rc = upload(ctx, &ctx->wih_f4h[l], f4))) return rc;
        }
        xb::split_rows(wh.data(), 4 * F, F, F, hi, lo, ctx->ns_rec[l] == 2 ? &ctx->whh_exp[l] : nullptr);
        if ((rc = upload(ctx, &ctx->whh_hi[l], hi))) return rc;
        if ((rc = upload(ctx, &ctx->whh_lo[l], lo))) return rc;
        ctx->whh_q1[l] = nullptr;
        if (ctx->knobs.lstm_i8 && ctx->ns_rec[l] == 2 && (F == 64 || F % 128 == 0)) {
            std::vector<int8_t> d1, d0;
            std::vector<float> sc;
            xb::i8_limbs(wh.data(), 4 * F, F, d1, d0, sc);
            if ((rc = upload(ctx, &ctx->whh_q1[l], d1))) return rc;
            if ((rc = upload(ctx, &ctx->whh_q0[l], d0))) return rc;
            if ((rc = upload(ctx, &ctx->whh_sc[l], sc))) return rc;
        }
        if ((rc = upload(ctx, &ctx->lbias[l], bb))) return rc;
    }
    xb::split_rows(need("encoder.9.linear.weight")->data(), ctx->O, F, F, hi, lo, ctx->ns_lin == 2 ? &ctx->wl_exp : nullptr);
    if ((rc = upload(ctx, &ctx->wl_hi, hi))) return rc;
    if ((rc = upload(ctx, &ctx->wl_lo, lo))) return rc;
    xb::fragment_major(hi, lo, ctx->O, F, F, ctx->ns_lin, f4, &ctx->wl_ks);
    if ((rc = upload(ctx, &ctx->wl_f4, f4))) return rc;
    if ((rc = upload(ctx, &ctx->bl, *need("encoder.9.linear.bias")))) return rc;
    ctx->host_w.clear();
    ctx->weights_ready = true;
    return XB_OK;
}

XB_API int xb_synchronize(xb_ctx *ctx)
{
    if (!ctx) return XB_ERR_INVALID;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    int rc = flush_held(ctx);
    if (!rc && ctx->deferred_rc) rc = ctx->deferred_rc;
    ctx->deferred_rc = 0;
    if (rc) return rc;
    rc = sync_all(ctx);
    if (rc) return rc;
    return check_device_error(ctx);
}

XB_API void *xb_result_stream(xb_ctx *ctx)
{
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    (void)flush_held(ctx);        // a failure is recorded (pipeline_failed, xb_last_error) and reported by the next call
    return ctx->result_stream ? ctx->result_stream : ctx->stream;
}

// xb_comm: run fn(arg) right behind the held-back call that will write d_seq, instead of now (returns 1), or report that no
// such call is held (0: the caller proceeds at once).  Not part of the public header.
extern "C" __attribute__((visibility("default"))) int xb_internal_defer_after(xb_ctx *ctx, const void *d_seq, void (*fn)(void *), void *arg)
{
    if (!ctx || !ctx->holding || ctx->held.seq != d_seq || ctx->held.after) return 0;
    ctx->held.after = fn;
    ctx->held.after_arg = arg;
    return 1;
}

// The host logic on its own, for the CPU tests (tests/host_logic.py): the planner and the knobs of xb_schedule.h, the packer
// of xb_pack.h, the decoder of xb_status.h, the lattice rules of xb_ctc_lattice.h.  None touches the device or needs a context.  Not part of the public header.
#define XB_INTERNAL extern "C" __attribute__((visibility("default")))
XB_INTERNAL void xb_internal_knobs_from_env(xb::Knobs *out) { *out = xb::knobs_from_env(); }
XB_INTERNAL int xb_internal_pair_capacity(int F, int cu_count, int lstm_wide) { return xb::pair_capacity(F, cu_count, lstm_wide); }
// -> the plan's error, or the number of its launch records (xb::LayerPlan::launch), of which the first max_launches are written
XB_INTERNAL int xb_internal_plan_layer(const xb::PlanQuery *q, xb::LayerPlan *plan, xb::PlanLaunch *launches, int max_launches)
{
    *plan = xb::plan_layer(*q);
    if (plan->error) return plan->error;
    const bool one = plan->mode != 2 || plan->ordering == xb::PLAN_SIGNAL;
    const int nts = one ? 1 : plan->nts, slabs = one ? 1 : plan->chunk_slabs;
    for (int i = 0, r = 0; i < nts; ++i)
        for (int j = 0; j < slabs && r < max_launches; ++j) launches[r++] = plan->launch(i, j);
    return nts * slabs;
}
// -> the status a synchronising call returns for the two device status words; *message its text, null with XB_OK
XB_INTERNAL int xb_internal_decode_status(unsigned sync_word, unsigned data_word, const char **message)
{
    const xb::DeviceStatus s = xb::decode_status(sync_word, data_word);
    if (message) *message = s.message;
    return s.code;
}
XB_INTERNAL int xb_internal_f32_to_e4m3(float x) { return xb::f32_to_e4m3(x); }
// hi, lo: (rows, ld) fp16; q8_exp as xb::split_rows takes it
XB_INTERNAL void xb_internal_split_rows(const float *src, int rows, int cols, int ld, half_t *hi, half_t *lo, int *q8_exp)
{
    std::vector<half_t> h, l;
    xb::split_rows(src, rows, cols, ld, h, l, q8_exp);
    memcpy(hi, h.data(), h.size() * sizeof(half_t));
    memcpy(lo, l.data(), l.size() * sizeof(half_t));
}
// -> the image's bytes; written to `out` when it has room for them
XB_INTERNAL size_t xb_internal_fragment_major(const half_t *hi, const half_t *lo, int rows, int ld, int K, int nsplit, unsigned char *out,
                                              size_t out_bytes, size_t *kstride)
{
    const std::vector<half_t> h(hi, hi + (size_t)rows * ld), l(lo, lo + (size_t)rows * ld);
    std::vector<unsigned char> f4;
    xb::fragment_major(h, l, rows, ld, K, nsplit, f4, kstride);
    if (out && out_bytes >= f4.size()) memcpy(out, f4.data(), f4.size());
    return f4.size();
}
// wi, wh: (4F, F); bb: (4F)
XB_INTERNAL void xb_internal_gate_interleave(const float *wih, const float *whh, const float *bih, const float *bhh, int F, float *wi,
                                             float *wh, float *bb)
{
    std::vector<float> a, b, c;
    xb::gate_interleave(wih, whh, bih, bhh, F, a, b, c);
    memcpy(wi, a.data(), a.size() * sizeof(float));
    memcpy(wh, b.data(), b.size() * sizeof(float));
    memcpy(bb, c.data(), c.size() * sizeof(float));
}
// d1, d0: (rows, cols); scale: (rows)
XB_INTERNAL void xb_internal_i8_limbs(const float *w, int rows, int cols, int8_t *d1, int8_t *d0, float *scale)
{
    std::vector<int8_t> a, b;
    std::vector<float> c;
    xb::i8_limbs(w, rows, cols, a, b, c);
    memcpy(d1, a.data(), a.size());
    memcpy(d0, b.data(), b.size());
    memcpy(scale, c.data(), c.size() * sizeof(float));
}
// the lattice kernels' column rule over n label rows of Lt labels: stay, move, post: (n, Lt - sl + 1), cell l = position l's
// stay column, the move column into it and that column in the posteriors' layout
XB_INTERNAL void xb_internal_ctc_columns(const uint8_t *labels, int n, int Lt, int nb, int sl, int has_blank, int32_t *stay, int32_t *move,
                                         int32_t *post)
{
    const int np = Lt - (sl - 1);
    for (int b = 0; b < n; ++b)
        for (int l = 0; l < np; ++l) {
            int cs, cm, cp;
            if (has_blank) xb::ctc_columns<true>(labels + (size_t)b * Lt, l, nb, sl, cs, cm, cp);
            else xb::ctc_columns<false>(labels + (size_t)b * Lt, l, nb, sl, cs, cm, cp);
            stay[(size_t)b * np + l] = cs; move[(size_t)b * np + l] = cm; post[(size_t)b * np + l] = cp;
        }
}
// -> the PMAX instantiation (0: refused); *threads, *lds_bytes: the rest of xb::ctc_launch
XB_INTERNAL int xb_internal_ctc_launch(int positions, int threads_override, int chains, int *threads, size_t *lds_bytes)
{
    const xb::CtcLaunch L = xb::ctc_launch(positions, threads_override, chains != 0);
    if (threads) *threads = L.threads;
    if (lds_bytes) *lds_bytes = L.lds;
    return L.pmax;
}
#undef XB_INTERNAL

XB_API int xb_stream_wait_event(xb_ctx *ctx, void *hip_event)
{
    if (!ctx || !hip_event) return XB_ERR_INVALID;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    hipEvent_t ev = static_cast<hipEvent_t>(hip_event);
    XB_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
    if (ctx->stream3) XB_HIP(ctx, hipStreamWaitEvent(ctx->stream3, ev, 0));
    return XB_OK;
}

XB_API int xb_set_profiling(xb_ctx *ctx, int on)
{
    if (!ctx) return XB_ERR_INVALID;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = flush_held(ctx)) return rc;            // a held-back call is timed (or not) as it was when it was made
    ctx->profiling = on != 0;
    return XB_OK;
}

XB_API int xb_get_stage_times(xb_ctx *ctx, float ms[XB_STAGE_COUNT], int64_t launches[XB_STAGE_COUNT])
{
    if (!ctx) return XB_ERR_INVALID;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = flush_held(ctx)) return rc;
    if (int rc = sync_all(ctx)) return rc;
    collect_events(ctx);
    for (int i = 0; i < XB_STAGE_COUNT; ++i) {
        if (ms) ms[i] = ctx->stage_ms[i];
        if (launches) launches[i] = ctx->stage_launches[i];
    }
    return XB_OK;
}

XB_API int xb_reset_stage_times(xb_ctx *ctx)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = flush_held(ctx)) return rc;
    if (int rc = sync_all(ctx)) return rc;
    collect_events(ctx);
    for (int i = 0; i < XB_STAGE_COUNT; ++i) { ctx->stage_ms[i] = 0.f; ctx->stage_launches[i] = 0; }
    return XB_OK;
}

XB_API int xb_geometry(const xb_ctx *ctx, int *T, int *S, int *C_blank, int *C_noblank)
{
    if (!ctx) return XB_ERR_INVALID;
    if (T) *T = ctx->T;
    if (S) *S = ctx->S;
    if (C_blank) *C_blank = ctx->S * (ctx->cfg.n_base + 1);
    if (C_noblank) *C_noblank = ctx->O;
    return XB_OK;
}

// Diagnostic (tests of the mixed-precision encoder): the activation tensors the last xb_encode / xb_encode_dev of `n` chunks left
// in the ping-pong buffers -- which = 0: output of LSTM layer 3, 1: output of LSTM layer 4 -- as (T, n, features) fp16 bit
// patterns `hi` and the raw 2-byte-per-element second part (fp16 residual or q8 image, whichever the consuming stage reads).
XB_API int xb_debug_layer_output(xb_ctx *ctx, int which, int n, uint16_t *hi, uint16_t *second)
{
    if (!ctx || !hi || !second || which < 0 || which > 1) return XB_ERR_INVALID;
    if (n < 1 || n > ctx->cap) return fail(ctx, XB_ERR_INVALID, "batch %d outside [1, %d]", n, ctx->cap);
    if (int rc = enter(ctx, false)) return rc;
    if (int rc = sync_all(ctx)) return rc;
    const size_t bytes = sizeof(uint16_t) * (size_t)ctx->T * n * ctx->cfg.features;
    XB_HIP(ctx, hipMemcpy(hi, ctx->x_hi[which], bytes, hipMemcpyDeviceToHost));
    XB_HIP(ctx, hipMemcpy(second, ctx->x_lo[which], bytes, hipMemcpyDeviceToHost));
    return XB_OK;
}

#ifdef XB_LSTM_STAMPS
// diagnostic build only (csrc/Makefile target `diag`): per-phase cycle sums of the LSTM kernel's workgroup 0
XB_API int xb_debug_lstm_stamps(xb_ctx *ctx, unsigned long long out[10], int reset)
{
    if (!ctx) return XB_ERR_INVALID;
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    xb::lstm_read_stamps(out, reset != 0);
    return XB_OK;
}
#endif
#ifdef XB_GEMM_STAMPS
// diagnostic build only: per-phase cycle sums of gemm4p_kernel<*, 3> (xb_encoder.hip, g_gemm_stamps)
XB_API int xb_debug_gemm_stamps(xb_ctx *ctx, unsigned long long out[8], int reset)
{
    if (!ctx) return XB_ERR_INVALID;
    if (int rc = sync_all(ctx)) return rc;
    xb::gemm_read_stamps(out, reset != 0);
    return XB_OK;
}
#endif

}  // extern "C"
