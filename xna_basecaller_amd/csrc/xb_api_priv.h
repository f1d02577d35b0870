// xb_api_priv.h -- what the translation units of the inference calls share beyond xb_ctx.h, under the unit that defines it:
// xb_api.hip (the context core: workspaces, status words, stream housekeeping, StageScope), xb_run_encoder.hip (the stage
// arithmetic and run_encoder), xb_api_scores.hip (the planes and their staging, run_decode, and for xb_basecall_chunks_beam
// run_beam and beam_results_to_host), xb_api_basecall.hip (flush_held, basecall_async; xb_api_data.hip's xb_ctc_chunks basecalls
// too).  Ordinary C++ linkage; none is exported.
#pragma once
#include "xb_ctx.h"

inline int64_t ipow(int64_t b, int e) { int64_t r = 1; while (e-- > 0) r *= b; return r; }

// ---- xb_api.hip ----
int alloc_workspaces(xb_ctx *ctx, int cap);      // the batch-sized workspaces, for `cap` chunks
int check_device_error(xb_ctx *ctx);             // drains the main stream; the status words' condition, if any
int sync_all(xb_ctx *ctx);                       // drains the three streams
int next_dep(xb_ctx *ctx, hipEvent_t *ev);       // the next of the call's timing-less events

// counts a stage's launches and, while profiling, times them on `stream` (the main stream by default)
struct StageScope {
    xb_ctx *c;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st_;
    StageScope(xb_ctx *ctx, int st, int launches, hipStream_t stream = nullptr)
        : c(ctx), stage(st), st_(stream ? stream : ctx->stream)
    {
        c->stage_launches[st] += launches;
        if (c->profiling && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
            (void)hipEventRecord(a, st_);
    }
    ~StageScope()
    {
        if (a && b) {
            (void)hipEventRecord(b, st_);
            c->events.push_back({stage, a, b});
        }
    }
};

// ---- xb_run_encoder.hip ----
// Stage mask of the three-product arithmetic inside an f16f8 context: bits 0-4 = input projection of LSTM layer l, bits 5-9 =
// recurrence of layer l, bit 10 = CRF linear layer, bit 11 = conv3.  XB_PREC_MIXED: every feed-forward projection.  Measured on the
// peaky model (profiles/r04_x3_attribution.txt): the error variance of plain f16f8 splits as input projections 65 %,
// linear 18 %, recurrences 13 %, conv3 5 %; per ms of step time the recurrences buy the least, and they are the critical path.
constexpr int X3_MIXED_STAGES = 0x1f | (1 << 10) | (1 << 11);
void set_stage_arithmetic(xb_ctx *ctx, int x3_mask);
// the arrival counters: SYNC_SLOTS x 32 words, i.e. the 64 group slots of 64 chunks at 64 words each (lstm_kernel LG_SYNC)
constexpr int SYNC_SLOTS = 128;
// scores_out: (T, n, ldc) with ldc given; expand selects the blank-column layout
int run_encoder(xb_ctx *ctx, const float *d_signal, int n, int expand, float *scores_out, int ldc, const float *d_signal2 = nullptr,
                int split = 0);

// ---- xb_api_scores.hip ----
Planes planes(void *seq, void *len, const DecodeOut &o);
int plane_count(int level);
size_t plane_bytes(int T, int nb, int i);
bool has_required(const Planes &o, int level);
int ensure_staging(xb_ctx *ctx, int level);
DecodeOut staging_of(const xb_ctx *ctx, const DecodeOut &o);
int copy_planes(xb_ctx *ctx, int level, const Planes &dst, const Planes &src, int c0, int n, int T, hipMemcpyKind kind, hipStream_t st);
// optional outputs of the Log scans (xb_crf_logz / xb_crf_scans)
struct ScanOut {
    float *alpha = nullptr, *beta = nullptr, *logz = nullptr, *post = nullptr;   // device; post has row stride ldq
};
// the caller has checked T and n (score_args, or a pass of ctx->T steps)
int run_decode(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, int ld, const char *alphabet, int8_t *d_labels,
               int8_t *d_seq, int32_t *d_len, hipStream_t st = nullptr, const ScanOut *scan = nullptr, const DecodeOut *out = nullptr);
int run_beam(xb_ctx *ctx, const float *d_scores, int T, int n, int has_blank, int ld, const char *alphabet, int beam_width,
             float beam_cut, float qscale, float qoffset, int8_t *d_seq, int8_t *d_q, uint8_t *d_moves, float *d_score);
int beam_results_to_host(xb_ctx *ctx, int T, int n, int8_t *sequence, int8_t *qstring, uint8_t *moves, float *score);

// ---- xb_api_basecall.hip ----
int flush_held(xb_ctx *ctx);     // launches a held-back asynchronous basecall on its own
// the asynchronous basecall of n chunks at d_signal into device outputs (seq, len, out), of pipeline slot `slot` or none
int basecall_async(xb_ctx *ctx, const float *d_signal, int n, const char *alphabet, int8_t *seq, int32_t *len, const DecodeOut &out,
                   int slot = -1);
