// xb_run_encoder.hip -- encoder orchestration: the execution of the encoder's plans (xb::plan_layer, xb_schedule.h) as launches
// on the context's streams, the only code that reads a LayerPlan; xb_encode.  The public header declares every XB_API function
// extern "C"; nothing else here is.
#include "xb_api_priv.h"

static int precision_nsplit(int pr)
{
    return pr == XB_PREC_F16 ? 1 : ((pr == XB_PREC_F16F8 || pr == XB_PREC_F16F8_IN1 || pr == XB_PREC_MIXED) ? 2 : 3);
}

void set_stage_arithmetic(xb_ctx *ctx, int x3_mask)
{
    const int base = precision_nsplit(ctx->cfg.precision);
    const bool mix = base == 2;
    for (int l = 0; l < 5; ++l) {
        ctx->ns_in[l] = mix && ((x3_mask >> l) & 1) ? 3 : base;
        ctx->ns_rec[l] = mix && ((x3_mask >> (5 + l)) & 1) ? 3 : base;
    }
    ctx->ns_lin = mix && ((x3_mask >> 10) & 1) ? 3 : base;
    ctx->ns_conv = mix && ((x3_mask >> 11) & 1) ? 3 : base;
}

namespace {

// second part an activation tensor needs for a consumer of arithmetic ns: 2 = q8 image, 1 = fp16 residual, 0 = none read
int second_part(int ns) { return ns == 2 ? 2 : (ns == 3 ? 1 : 0); }

// the GEMM that consumes a layer's output rows of time steps [ta, tb): the input projection of LSTM layer `layer`
// (layer < 5, into `gin_out`) or the CRF linear layer (layer == 5, into the scores)
struct NextGemm {
    int layer;
    const half_t *x_hi, *x_lo;
    float *out;
    int ldc, expand;
};

int launch_row_gemm(xb_ctx *ctx, const NextGemm &ng, int n, int ta, int tb, hipStream_t st, bool shadow = false)
{
    const xb_config &c = ctx->cfg;
    const int F = c.features;
    xb::GemmParams g{};
    const size_t r0 = (size_t)ta * n;
    g.a_hi = ng.x_hi + r0 * F; g.a_lo = ng.x_lo + r0 * F;
    g.M = (tb - ta) * n; g.K = F; g.lda = F; g.ldb = F; g.nsplit = ng.layer < 5 ? ctx->ns_in[ng.layer] : ctx->ns_lin;
    g.ldc = ng.ldc; g.out_f32 = ng.out + r0 * ng.ldc;
    g.one_per_cu = shadow && ctx->knobs.gemm_shadow_wgs == 1;
    g.sn = ctx->knobs.gemm_sn;
    // which kernel: gemm4p_kernel, except for the slabs that run beside the two-groups-per-workgroup recurrence of a batch
    // above 1024 chunks, where the one-workgroup-per-CU gemm8r_kernel disturbs the recurrence less (same box, ms per step at
    // batch 2048: 477 vs 488 (gemm4p, one workgroup per CU) vs 499; batch 1024: 240 vs 246 vs 235; batch 512: 126.7 vs 129.7 vs
    // 123.0 -- profiles/r03_gemm_kernel_by_batch.txt).  XB_GEMM_SHADOW=4 / 8 forces one of them.
    const bool use4 = ctx->knobs.gemm4 && !(shadow && (ctx->knobs.gemm_shadow_kernel == 8 || (ctx->knobs.gemm_shadow_kernel == 0 && n > 1024)));
    if (ng.layer < 5) {
        StageScope sc(ctx, XB_STAGE_LSTM_IN, 1, st);
        g.b_hi = ctx->wih_hi[ng.layer]; g.b_lo = ctx->wih_lo[ng.layer]; g.Nn = 4 * F; g.bias = ctx->lbias[ng.layer];
        // main product only (the q8 images stay unused) -- in1_layers: bit l = input projection of layer l (diagnostic
        // XB_IN1_LAYERS, default all five)
        if (use4) { g.b4 = ctx->wih_f4[ng.layer]; g.b4_kstride = ctx->wih_ks; }
        if (ctx->cfg.precision == XB_PREC_F16F8_IN1 && ((ctx->knobs.in1_layers >> ng.layer) & 1)) {
            g.nsplit = 1;
            if (use4) { g.b4 = ctx->wih_f4h[ng.layer]; g.b4_kstride = ctx->wih_ksh; }
        }
        g.a_exp = ng.layer == 0 ? 0 : 8; g.b_exp = ctx->wih_exp[ng.layer];     // conv3 output / LSTM output
        g.gin_n = n;                                                           // member-major gin (xb_internal.h)
        XB_HIP(ctx, xb::launch_gemm(g, xb::EPI_BIAS_F32, st));
    } else {
        StageScope sc(ctx, XB_STAGE_LINEAR, 1, st);
        g.b_hi = ctx->wl_hi; g.b_lo = ctx->wl_lo; g.Nn = ctx->O; g.bias = ctx->bl;
        g.scale = c.scale; g.nb = c.n_base; g.expand = ng.expand; g.blank = c.blank_score;
        g.a_exp = 8; g.b_exp = ctx->wl_exp;
        if (use4) { g.b4 = ctx->wl_f4; g.b4_kstride = ctx->wl_ks; }
        XB_HIP(ctx, xb::launch_gemm(g, xb::EPI_TANH_SCALE, st));
    }
    return XB_OK;
}

// Recurrence of one layer from `gin` into (xout_hi, xout_lo).  With `next` set, the GEMM that consumes this layer's output
// is issued as well: either afterwards on the main stream, or -- overlapped mode -- slab by slab on the second stream while
// the recurrence (192 of the 256 CUs, latency bound) is still running; the main stream then waits for the last slab.
// Which launches, over which chunks and steps, in which order: xb::plan_layer (xb_schedule.h); this function executes its plan.
static_assert(xb::PLAN_ERR_INVALID == XB_ERR_INVALID, "a refused plan is an invalid argument");

void set_launch(xb::LstmParams &p, const xb::PlanLaunch &l)
{
    p.n0 = l.n0; p.nslab = l.nslab; p.s_begin = l.s_begin; p.s_end = l.s_end; p.dual = l.dual;
    p.grp0 = l.grp0; p.slab = l.slab; p.xcd_local = l.xcd_local; p.sync_base = l.sync_base;
}

// the main stream waits for what the second stream has been given so far
int join_stream2(xb_ctx *ctx)
{
    hipEvent_t ev;
    if (int rc = next_dep(ctx, &ev)) return rc;
    XB_HIP(ctx, hipEventRecord(ev, ctx->stream2));
    XB_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
    return XB_OK;
}

int run_lstm_layer(xb_ctx *ctx, int layer, int n, const float *gin, half_t *xout_hi, half_t *xout_lo, const NextGemm *next)
{
    const int F = ctx->cfg.features, T = ctx->T;
    // what the GEMM that reads this layer's output needs as the second part; the int8-limb recurrence writes hi + q8 only
    const int y_need = second_part(layer < 4 ? ctx->ns_in[layer + 1] : ctx->ns_lin);
    const bool i8 = ctx->knobs.lstm_i8 && ctx->whh_q1[layer] && ctx->ns_rec[layer] == 2 && y_need != 1;
    const int rec_nsplit = i8 ? (ctx->knobs.lstm_i8 == 2 ? 5 : 4) : ctx->ns_rec[layer];
    // the occupancy calculator's word on the persistent kernel, asked once per context and arithmetic
    int (&res)[2] = ctx->lstm_resident[rec_nsplit];
    if (res[0] < 0) res[0] = xb::lstm_resident_per_cu(F, rec_nsplit, 0);
    if (res[1] < 0) res[1] = xb::lstm_resident_per_cu(F, rec_nsplit, 1);
    xb::PlanQuery q{};
    q.F = F; q.n = n; q.T = T; q.cu_count = ctx->cu_count; q.knobs = ctx->knobs;
    if (const char *e = getenv("XB_LSTM_SPREAD")) q.spread = atoi(e) != 0;
    q.has_next = next && ctx->stream2;
    q.resident1 = res[0] >= 1; q.resident2 = res[1] >= 1; q.signal_ok = ctx->sig_flag != nullptr;
    const xb::LayerPlan plan = xb::plan_layer(q);
    if (plan.error) return fail(ctx, plan.error, "%s", plan.message);

    XB_HIP(ctx, hipMemsetAsync(ctx->c_state, 0, sizeof(float) * (size_t)n * F, ctx->stream));
    xb::LstmParams p{};
    p.gin = gin; p.w_hi = ctx->whh_hi[layer]; p.w_lo = ctx->whh_lo[layer];
    p.y_hi = xout_hi; p.y_lo = xout_lo; p.c_state = ctx->c_state; p.xh = ctx->xh;
    p.T = T; p.N = n; p.F = F; p.reverse = (layer % 2) == 0;
    p.sync = ctx->sync; p.error = ctx->error; p.nsplit = ctx->ns_rec[layer]; p.w_exp = ctx->whh_exp[layer];
    p.y_alt = (p.nsplit == 2 || p.nsplit == 3) && y_need != 0 && y_need != second_part(p.nsplit);
    if (i8) {
        p.nsplit = rec_nsplit; p.wq1 = ctx->whh_q1[layer]; p.wq0 = ctx->whh_q0[layer]; p.wscale = ctx->whh_sc[layer];
    }
    p.spread = plan.spread;
    p.persistent = plan.mode == 2;
    // the GEMM of time slab i beside the recurrence, on the second stream
    auto slab_gemm = [&](int i) {
        int ta, tb;
        plan.gemm_rows(i, p.reverse != 0, &ta, &tb);
        return launch_row_gemm(ctx, *next, n, ta, tb, ctx->stream2, true);
    };
    if (!p.persistent) {
        StageScope sc(ctx, XB_STAGE_LSTM_REC, plan.rec_launches);
        set_launch(p, plan.launch(0, 0));
        for (int s = 0; s < T; ++s) {
            p.s_begin = s; p.s_end = s + 1;
            XB_HIP(ctx, xb::launch_lstm(p, ctx->stream));
        }
    } else {
        if (plan.global_groups) XB_HIP(ctx, hipMemsetAsync(ctx->sync, 0, sizeof(unsigned) * SYNC_SLOTS * 32, ctx->stream));
        if (plan.ordering == xb::PLAN_SIGNAL) {
            if (ctx->sig_seq > (1u << 30)) {           // keep the 32-bit flag monotonic: start over from an idle device
                int rc = sync_all(ctx);
                if (rc) return rc;
                XB_HIP(ctx, hipMemset(ctx->sig_flag, 0, 4));
                ctx->sig_seq = 0;
            }
            XB_HIP(ctx, hipMemsetAsync(ctx->sig_done, 0, sizeof(unsigned) * 64, ctx->stream));
            {
                StageScope sc(ctx, XB_STAGE_LSTM_REC, plan.rec_launches);
                set_launch(p, plan.launch(0, 0));
                p.sig_flag = ctx->sig_flag; p.sig_done = ctx->sig_done; p.sig_base = ctx->sig_seq; p.sig_nts = plan.nts;
                XB_HIP(ctx, xb::launch_lstm(p, ctx->stream));
            }
            for (int i = 0; i < plan.nts; ++i) {
                XB_HIP(ctx, hipStreamWaitValue32(ctx->stream2, ctx->sig_flag, ctx->sig_seq + (unsigned)i + 1u, hipStreamWaitValueGte,
                                                 0xffffffffu));
                if (int rc = slab_gemm(i)) return rc;
            }
            ctx->sig_seq += (unsigned)plan.nts;
            return join_stream2(ctx);
        }
        for (int i = 0; i < plan.nts; ++i) {
            {
                StageScope sc(ctx, XB_STAGE_LSTM_REC, i == 0 ? plan.rec_launches : 0);
                for (int j = 0; j < plan.chunk_slabs; ++j) {
                    set_launch(p, plan.launch(i, j));
                    if (!plan.global_groups) XB_HIP(ctx, hipMemsetAsync(ctx->sync, 0, sizeof(unsigned) * SYNC_SLOTS * 32, ctx->stream));
                    XB_HIP(ctx, xb::launch_lstm(p, ctx->stream));
                }
            }
            if (plan.ordering == xb::PLAN_EVENTS) {
                hipEvent_t ev;
                int rc = next_dep(ctx, &ev);
                if (rc) return rc;
                XB_HIP(ctx, hipEventRecord(ev, ctx->stream));
                XB_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ev, 0));
                if ((rc = slab_gemm(i))) return rc;
            }
        }
        if (plan.ordering == xb::PLAN_EVENTS) return join_stream2(ctx);
    }
    // PLAN_SERIAL, PLAN_SLABS_SERIAL_GEMM: the GEMM follows on the main stream
    if (next) return launch_row_gemm(ctx, *next, n, 0, T, ctx->stream);
    return XB_OK;
}

}  // namespace

// scores_out: (T, n, ldc) with ldc given; expand selects the blank-column layout
int run_encoder(xb_ctx *ctx, const float *d_signal, int n, int expand, float *scores_out, int ldc, const float *d_signal2, int split)
{
    const xb_config &c = ctx->cfg;
    const int F = c.features, T = ctx->T;
    const int nsplit = ctx->ns_conv;
    ctx->dep_next = 0;
    ctx->enc_n = n;
    {
        StageScope sc(ctx, XB_STAGE_CONV, 2);
        xb::ConvFrontParams cf{};
        cf.signal = d_signal; cf.signal2 = d_signal2; cf.split = d_signal2 ? split : n; cf.N = n; cf.L = c.chunk_len; cf.T = T; cf.winlen = c.winlen; cf.stride = c.stride;
        cf.kp = ctx->kp; cf.w1 = ctx->w1; cf.b1 = ctx->b1; cf.w2 = ctx->w2; cf.b2 = ctx->b2;
        cf.a_hi = ctx->im_hi; cf.a_lo = ctx->im_lo; cf.q8 = nsplit == 2;
        XB_HIP(ctx, xb::launch_conv_front(cf, ctx->stream));
        xb::GemmParams g{};
        g.a_hi = ctx->im_hi; g.a_lo = ctx->im_lo; g.b_hi = ctx->w3_hi; g.b_lo = ctx->w3_lo;
        g.M = T * n; g.Nn = F; g.K = ctx->kp; g.lda = ctx->kp; g.ldb = ctx->kp;
        g.bias = ctx->b3; g.out_hi = ctx->x_hi[0]; g.out_lo = ctx->x_lo[0]; g.ldc = F; g.nsplit = nsplit;
        g.a_exp = 0; g.b_exp = ctx->w3_exp; g.out_exp = 0;
        g.out_fmt = second_part(ctx->ns_in[0]);            // (0: hi only is read -- the GEMM's own form)
        if (ctx->knobs.gemm4) { g.b4 = ctx->w3_f4; g.b4_kstride = ctx->w3_ks; }
        XB_HIP(ctx, xb::launch_gemm(g, xb::EPI_SILU_SPLIT, ctx->stream));
    }
    // layer l reads gin[l & 1] while the next layer's input projection is written into the other buffer
    float *gin[2] = {ctx->gin, ctx->gin2 ? ctx->gin2 : ctx->gin};
    int cur = 0;
    {
        const NextGemm first{0, ctx->x_hi[0], ctx->x_lo[0], gin[0], 4 * F, 0};
        int rc = launch_row_gemm(ctx, first, n, 0, T, ctx->stream);
        if (rc) return rc;
    }
    for (int l = 0; l < 5; ++l) {
        NextGemm next{l + 1, ctx->x_hi[cur ^ 1], ctx->x_lo[cur ^ 1], l < 4 ? gin[(l + 1) & 1] : scores_out,
                      l < 4 ? 4 * F : ldc, expand};
        int rc = run_lstm_layer(ctx, l, n, gin[l & 1], ctx->x_hi[cur ^ 1], ctx->x_lo[cur ^ 1], &next);
        if (rc) return rc;
        cur ^= 1;
    }
    return XB_OK;
}

// the encoder of n chunks into blank-less scores (T, n, ldc), for xb_head.hip (the trainer's forward pass)
int encoder_run(xb_ctx *ctx, const float *d_signal, int n, float *d_scores, int ldc) { return run_encoder(ctx, d_signal, n, 0, d_scores, ldc); }

// The frozen bottom of a training step (xb_top.hip): run_encoder's launches up to and including LSTM layer `layers` - 1, the
// last of them without a consumer (next = nullptr: run_lstm_layer then plans no slab GEMM and issues none afterwards).  The
// output, fp16 hi + fp16 residual, lies in x_hi / x_lo [layers & 1], as the full pass leaves it there on its way up.
int encoder_bottom_run(xb_ctx *ctx, const float *d_signal, int n, int layers)
{
    const xb_config &c = ctx->cfg;
    const int F = c.features, T = ctx->T;
    const int nsplit = ctx->ns_conv;
    if (layers < 0 || layers > 5) return fail(ctx, XB_ERR_INVALID, "the bottom pass runs 0 .. 5 LSTM layers, got %d", layers);
    if ((layers < 5 ? ctx->ns_in[layers] : ctx->ns_lin) != 3)
        return fail(ctx, XB_ERR_INVALID, "the bottom pass needs the fp16 residual of layer output %d, which this context's stage arithmetic does not write", layers);
    ctx->dep_next = 0;
    ctx->enc_n = layers == 5 ? n : 0;           // below the top, x_hi[1] / x_lo[1] do not hold the last layer's output
    {
        StageScope sc(ctx, XB_STAGE_CONV, 2);
        xb::ConvFrontParams cf{};
        cf.signal = d_signal; cf.signal2 = nullptr; cf.split = n; cf.N = n; cf.L = c.chunk_len; cf.T = T; cf.winlen = c.winlen; cf.stride = c.stride;
        cf.kp = ctx->kp; cf.w1 = ctx->w1; cf.b1 = ctx->b1; cf.w2 = ctx->w2; cf.b2 = ctx->b2;
        cf.a_hi = ctx->im_hi; cf.a_lo = ctx->im_lo; cf.q8 = nsplit == 2;
        XB_HIP(ctx, xb::launch_conv_front(cf, ctx->stream));
        xb::GemmParams g{};
        g.a_hi = ctx->im_hi; g.a_lo = ctx->im_lo; g.b_hi = ctx->w3_hi; g.b_lo = ctx->w3_lo;
        g.M = T * n; g.Nn = F; g.K = ctx->kp; g.lda = ctx->kp; g.ldb = ctx->kp;
        g.bias = ctx->b3; g.out_hi = ctx->x_hi[0]; g.out_lo = ctx->x_lo[0]; g.ldc = F; g.nsplit = nsplit;
        g.a_exp = 0; g.b_exp = ctx->w3_exp; g.out_exp = 0;
        g.out_fmt = second_part(ctx->ns_in[0]);
        if (ctx->knobs.gemm4) { g.b4 = ctx->w3_f4; g.b4_kstride = ctx->w3_ks; }
        XB_HIP(ctx, xb::launch_gemm(g, xb::EPI_SILU_SPLIT, ctx->stream));
    }
    if (layers == 0) return XB_OK;
    float *gin[2] = {ctx->gin, ctx->gin2 ? ctx->gin2 : ctx->gin};
    int cur = 0;
    {
        const NextGemm first{0, ctx->x_hi[0], ctx->x_lo[0], gin[0], 4 * F, 0};
        if (int rc = launch_row_gemm(ctx, first, n, 0, T, ctx->stream)) return rc;
    }
    for (int l = 0; l < layers; ++l) {
        const NextGemm next{l + 1, ctx->x_hi[cur ^ 1], ctx->x_lo[cur ^ 1], gin[(l + 1) & 1], 4 * F, 0};
        if (int rc = run_lstm_layer(ctx, l, n, gin[l & 1], ctx->x_hi[cur ^ 1], ctx->x_lo[cur ^ 1], l + 1 < layers ? &next : nullptr)) return rc;
        cur ^= 1;
    }
    return XB_OK;
}

XB_API int xb_encode_dev(xb_ctx *ctx, const float *d_signal, int n, int expand_blanks, float *d_scores)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    if (!d_signal || !d_scores) return fail(ctx, XB_ERR_INVALID, "null device pointer");
    if ((rc = enter(ctx, true))) return rc;
    const int ldc = expand_blanks ? ctx->S * (ctx->cfg.n_base + 1) : ctx->O;
    return run_encoder(ctx, d_signal, n, expand_blanks ? 1 : 0, d_scores, ldc);
}

XB_API int xb_encode(xb_ctx *ctx, const float *signal, int n, int expand_blanks, float *scores)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    if (!signal || !scores) return fail(ctx, XB_ERR_INVALID, "null host pointer");
    if ((rc = enter(ctx, false))) return rc;
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * (size_t)n * ctx->cfg.chunk_len,
                               hipMemcpyHostToDevice, ctx->stream));
    const int ldc = expand_blanks ? ctx->S * (ctx->cfg.n_base + 1) : ctx->O;
    rc = run_encoder(ctx, ctx->d_signal, n, expand_blanks ? 1 : 0, ctx->scores, ldc);
    if (rc) return rc;
    XB_HIP(ctx, hipMemcpyAsync(scores, ctx->scores, sizeof(float) * (size_t)ctx->T * n * ldc, hipMemcpyDeviceToHost,
                               ctx->stream));
    return xb_synchronize(ctx);
}
