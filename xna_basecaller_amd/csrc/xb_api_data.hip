// xb_api_data.hip -- the ctc-data tools of the C ABI: template mapping, ctc labels, the UB tally, the barcode distance, DTW segmentation, spliced
// augmentation, synthetic spiking and fully synthetic chunks.  Each has a _dev form on device pointers and a host-pointer form
// that stages through xb_ctx::staging (Staging, xb_ctx.h); the forms that take label rows check and stage them as the trainers'
// steps do (label_batch_check, LabelBatch, xb_ctx.h).
#include "xb_api_priv.h"        // basecall_async, for xb_ctc_chunks

namespace {

// Cells (query row x template column, both strands) one call may ask for, counted with every row as wide as W:
// 2 n W sum(L).  The score pass runs 6.8e11 cells a second on an MI355X (profiles/map_time.txt: 1024 templates of 89 against
// 4096 reads in 106 ms), so the bound keeps a call under a fifth of a second of device time.  The library itself is bounded
// too: beyond a megabyte of templates (the 2.7 MB CPLX full-length library) exhaustive alignment is the wrong tool and a
// seeding stage would be needed.
constexpr double MAP_CELL_BUDGET = 1.2e11;
constexpr size_t MAP_MAX_LIBRARY = (size_t)1 << 20;
constexpr size_t MAP_MAX_SCRATCH = (size_t)256 << 20;

struct MapOut {
    int32_t *tmpl; int8_t *strand; int32_t *score, *second, *q_st, *q_en, *r_st, *r_en; uint8_t *ops; int32_t *n_ops;
};

// a library's extent: *lmax = the longest template, *total = the letters of all, every template within the mapper's bounds
// (who: the entry point a refusal names)
int library_extent(xb_ctx *ctx, const char *who, const char *templates, const int32_t *offsets, int R, int *lmax, size_t *total = nullptr)
{
    if (!templates || !offsets || R < 1 || offsets[0] != 0) return fail(ctx, XB_ERR_INVALID, "%s: empty template library", who);
    *lmax = 0;
    for (int t = 0; t < R; ++t) {
        const int L = offsets[t + 1] - offsets[t];
        if (L < 1 || L > xb::MAP_MAX_TEMPLATE)
            return fail(ctx, XB_ERR_INVALID, "%s: template %d has %d letters; 1 .. %d are supported", who, t, L, xb::MAP_MAX_TEMPLATE);
        *lmax = std::max(*lmax, L);
    }
    if (total) *total = (size_t)offsets[R];
    return XB_OK;
}

// the library's device image (rebuilt only when the bytes change) for n rows of width W: validation, *lmax = the longest template
// (sc: the mapper's scoring, checked where it always was; null for a caller that aligns nothing and is not held to the cell budget;
// who: the entry point a refusal names)
int map_library(xb_ctx *ctx, const char *who, int n, int W, const char *templates, const int32_t *offsets, int R, const int *sc, int *lmax)
{
    if (n < 1 || W < 1 || W > xb::MAP_MAX_ROW)
        return fail(ctx, XB_ERR_INVALID, "%s: n = %d rows of width %d; need n >= 1 and 1 <= W <= %d", who, n, W, xb::MAP_MAX_ROW);
    for (int k = 0; sc && k < 5; ++k)
        if (sc[k] < 0 || sc[k] > 1000) return fail(ctx, XB_ERR_INVALID, "%s: scoring values must lie in [0, 1000]", who);
    size_t total = 0;
    if (int rc = library_extent(ctx, who, templates, offsets, R, lmax, &total)) return rc;
    const double cells = 2.0 * n * W * (double)total;
    if (total > MAP_MAX_LIBRARY || (sc && cells > MAP_CELL_BUDGET))
        return fail(ctx, XB_ERR_INVALID, "%s: a library of %d templates, %zu letters, against %d rows of width %d is %.3g "
                    "cells; one call takes at most %.3g cells and a library of %zu letters (larger libraries need a seeding stage)", who,
                    R, total, n, W, cells, MAP_CELL_BUDGET, MAP_MAX_LIBRARY);
    xb_ctx::MapState &m = ctx->map;
    const bool same = m.image.p && m.lib.size() == total && (int)m.off.size() == R + 1 &&
                      !memcmp(m.lib.data(), templates, total) && !memcmp(m.off.data(), offsets, sizeof(int32_t) * (R + 1));
    if (!same) {
        std::vector<uint8_t> codes(total);
        for (size_t k = 0; k < total; ++k) {
            switch (templates[k]) {
            case 'A': case 'a': codes[k] = 0; break;
            case 'C': case 'c': codes[k] = 1; break;
            case 'G': case 'g': codes[k] = 2; break;
            case 'T': case 't': codes[k] = 3; break;
            default: codes[k] = 4;
            }
        }
        std::vector<int32_t> chunks{0};
        for (int t = 0, used = 0; t < R; ++t) {
            const int L = offsets[t + 1] - offsets[t];
            if (used + L > xb::MAP_CHUNK_BYTES) { chunks.push_back(t); used = 0; }
            used += L;
        }
        chunks.push_back(R);
        const size_t a_off = m.off_at(total), a_chunk = a_off + sizeof(int32_t) * (R + 1);     // what toff() / chunk_first() read
        const size_t a_letters = a_chunk + sizeof(int32_t) * chunks.size();                    // what tletters() reads
        m.lib.clear();                                                  // no image while it is being replaced
        if (int rc = grow(ctx, &m.image, a_letters + total)) return rc;
        XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        uint8_t *img = static_cast<uint8_t *>(m.image.p);
        XB_HIP(ctx, hipMemcpy(img, codes.data(), total, hipMemcpyHostToDevice));
        XB_HIP(ctx, hipMemcpy(img + a_off, offsets, sizeof(int32_t) * (R + 1), hipMemcpyHostToDevice));
        XB_HIP(ctx, hipMemcpy(img + a_chunk, chunks.data(), sizeof(int32_t) * chunks.size(), hipMemcpyHostToDevice));
        XB_HIP(ctx, hipMemcpy(img + a_letters, templates, total, hipMemcpyHostToDevice));
        m.lib.assign(templates, templates + total);
        m.off.assign(offsets, offsets + R + 1);
        m.Lmax = *lmax;
        m.nchunks = (int)chunks.size() - 1;
    }
    return XB_OK;
}

// validation, the library's device image, the two launches: seq, seq_len and o are device pointers
int map_run(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_len, int n, int W, const char *templates, const int32_t *offsets,
            int R, const int sc[5], const MapOut &o)
{
    int Lmax = 0;
    if (int rc = map_library(ctx, "xb_map_templates", n, W, templates, offsets, R, sc, &Lmax)) return rc;
    xb_ctx::MapState &m = ctx->map;
    xb::MapParams p{};
    p.seq = d_seq; p.seq_len = d_len; p.n = n; p.W = W;
    p.tcodes = m.tcodes(); p.toff = m.toff(); p.chunk_first = m.chunk_first();
    p.R = R; p.Lmax = Lmax; p.nchunks = m.nchunks;
    p.match = sc[0]; p.mismatch = sc[1]; p.gap_open = sc[2]; p.gap_extend = sc[3]; p.ambiguous = sc[4];
    if (int rc = grow(ctx, &m.partial, sizeof(int32_t) * xb::MAP_PARTIAL_INTS * (size_t)n * m.nchunks)) return rc;
    p.partial = static_cast<int32_t *>(m.partial.p);
    p.trace_wgs = std::min(n, 2048);
    if (!xb::map_trace_in_lds(W, Lmax)) {
        const size_t one = (size_t)W * Lmax;
        p.trace_wgs = (int)std::max<size_t>(1, std::min<size_t>(p.trace_wgs, MAP_MAX_SCRATCH / one));
        if (int rc = grow(ctx, &m.scratch, one * p.trace_wgs)) return rc;
        p.scratch = static_cast<uint8_t *>(m.scratch.p);
    }
    p.tmpl = o.tmpl; p.strand = o.strand; p.score = o.score; p.second = o.second;
    p.q_st = o.q_st; p.q_en = o.q_en; p.r_st = o.r_st; p.r_en = o.r_en; p.ops = o.ops; p.n_ops = o.n_ops;
    XB_HIP(ctx, xb::launch_map_score(p, ctx->stream));
    XB_HIP(ctx, xb::launch_map_trace(p, ctx->stream));
    return XB_OK;
}

bool map_out_complete(const MapOut &o)
{
    return o.tmpl && o.strand && o.score && o.second && o.q_st && o.q_en && o.r_st && o.r_en && o.ops && o.n_ops;
}

}  // namespace

extern "C" {

// ---- template mapper (xb_map_templates) -----------------------------------------------------------------------------
XB_API int xb_map_templates_dev(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int W, const char *templates,
                                const int32_t *offsets, int R, int match, int mismatch, int gap_open, int gap_extend, int ambiguous,
                                int32_t *d_tmpl, int8_t *d_strand, int32_t *d_score, int32_t *d_second, int32_t *d_q_st,
                                int32_t *d_q_en, int32_t *d_r_st, int32_t *d_r_en, uint8_t *d_ops, int32_t *d_n_ops)
{
    if (!ctx) return XB_ERR_INVALID;
    const MapOut o = {d_tmpl, d_strand, d_score, d_second, d_q_st, d_q_en, d_r_st, d_r_en, d_ops, d_n_ops};
    if (!d_seq || !d_seq_len || !map_out_complete(o)) return fail(ctx, XB_ERR_INVALID, "xb_map_templates: null device pointer");
    if (int rc = enter(ctx, true)) return rc;
    const int sc[5] = {match, mismatch, gap_open, gap_extend, ambiguous};
    return map_run(ctx, d_seq, d_seq_len, n, W, templates, offsets, R, sc, o);
}

XB_API int xb_map_templates(xb_ctx *ctx, const int8_t *seq, const int32_t *seq_len, int n, int W, const char *templates,
                            const int32_t *offsets, int R, int match, int mismatch, int gap_open, int gap_extend, int ambiguous,
                            int32_t *tmpl, int8_t *strand, int32_t *score, int32_t *second, int32_t *q_st, int32_t *q_en,
                            int32_t *r_st, int32_t *r_en, uint8_t *ops, int32_t *n_ops)
{
    if (!ctx) return XB_ERR_INVALID;
    const MapOut h = {tmpl, strand, score, second, q_st, q_en, r_st, r_en, ops, n_ops};
    if (!seq || !seq_len || !map_out_complete(h)) return fail(ctx, XB_ERR_INVALID, "xb_map_templates: null host pointer");
    if (n < 1 || W < 1 || W > xb::MAP_MAX_ROW || !offsets || R < 1)
        return fail(ctx, XB_ERR_INVALID, "xb_map_templates: n = %d rows of width %d, %d templates; need n >= 1, 1 <= W <= %d, R >= 1",
                    n, W, R, xb::MAP_MAX_ROW);
    if (int rc = enter(ctx, false)) return rc;
    int Lmax = 0;
    if (int rc = library_extent(ctx, "xb_map_templates", templates, offsets, R, &Lmax)) return rc;
    const size_t N = (size_t)n, cap = (size_t)W + Lmax;
    Staging st{ctx};
    const auto d_seq = st.take<int8_t>(N * W);
    Staging::Piece<int32_t> d_i32[9];                   // seq_len | tmpl, score, second, q_st, q_en, r_st, r_en, n_ops
    for (auto &piece : d_i32) piece = st.take<int32_t>(N);
    const auto d_strand = st.take<int8_t>(N);
    const auto d_ops = st.take<uint8_t>(N * cap);
    if (st.used > ((size_t)2 << 30))
        return fail(ctx, XB_ERR_INVALID, "xb_map_templates: %d rows of width %d in one call; split the batch", n, W);
    if (int rc = st.ready()) return rc;
    XB_HIP(ctx, hipMemcpyAsync(d_seq, seq, N * W, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_i32[0], seq_len, N * 4, hipMemcpyHostToDevice, ctx->stream));
    const MapOut d = {d_i32[1], d_strand, d_i32[2], d_i32[3], d_i32[4], d_i32[5], d_i32[6], d_i32[7], d_ops, d_i32[8]};
    const int sc[5] = {match, mismatch, gap_open, gap_extend, ambiguous};
    if (int rc = map_run(ctx, d_seq, d_i32[0], n, W, templates, offsets, R, sc, d)) return rc;
    int32_t *const h_i32[8] = {tmpl, score, second, q_st, q_en, r_st, r_en, n_ops};
    for (int k = 0; k < 8; ++k) XB_HIP(ctx, hipMemcpyAsync(h_i32[k], d_i32[k + 1], N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(strand, d.strand, N, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ops, d.ops, N * cap, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// ---- ctc-data labels of mapped rows (xb_ctc_targets, xb_ctc_chunks) ---------------------------------------------------
namespace {

struct CtcIn {
    const int32_t *seq_len, *tmpl; const int8_t *strand; const int32_t *q_st, *q_en, *r_st, *r_en; const uint8_t *ops; const int32_t *n_ops;
};
struct CtcOut {
    int32_t *mlen, *blen; uint8_t *verdict, *target; int32_t *target_len;
};
struct CtcRule {
    double min_accuracy, min_coverage; int ub_only, ub_plus, ub_minus;
};

bool ctc_complete(const CtcIn &i, const CtcOut &o)
{
    return i.seq_len && i.tmpl && i.strand && i.q_st && i.q_en && i.r_st && i.r_en && i.ops && i.n_ops && o.mlen && o.blen && o.verdict &&
           o.target && o.target_len;
}

// validation, the library's device image, the launch: i and o are device pointers
int ctc_run(xb_ctx *ctx, const CtcIn &i, int n, int W, const char *templates, const int32_t *offsets, int R, const CtcRule &rule,
            const CtcOut &o)
{
    if (rule.ub_plus < 1 || rule.ub_plus > 255 || rule.ub_minus < 1 || rule.ub_minus > 255)
        return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: ub_plus = %d, ub_minus = %d; labels are 1 .. 255", rule.ub_plus, rule.ub_minus);
    if (!(rule.min_accuracy == rule.min_accuracy) || !(rule.min_coverage == rule.min_coverage))
        return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: a threshold is not a number");
    if (reinterpret_cast<uintptr_t>(o.target) & 15) return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: target must be 16-byte aligned");
    int Lmax = 0;
    if (int rc = map_library(ctx, "xb_ctc_targets", n, W, templates, offsets, R, nullptr, &Lmax)) return rc;
    xb::CtcTargetParams p{};
    p.seq_len = i.seq_len; p.n = n; p.W = W; p.cap = W + Lmax;
    p.tmpl = i.tmpl; p.strand = i.strand; p.q_st = i.q_st; p.q_en = i.q_en; p.r_st = i.r_st; p.r_en = i.r_en; p.ops = i.ops; p.n_ops = i.n_ops;
    p.tcodes = ctx->map.tcodes(); p.toff = ctx->map.toff();
    p.R = R; p.TW = xb::ctc_target_width(Lmax);
    p.min_accuracy = rule.min_accuracy; p.min_coverage = rule.min_coverage;
    p.ub_only = rule.ub_only != 0; p.ub_plus = rule.ub_plus; p.ub_minus = rule.ub_minus;
    p.mlen = o.mlen; p.blen = o.blen; p.verdict = o.verdict; p.target = o.target; p.target_len = o.target_len;
    XB_HIP(ctx, xb::launch_ctc_targets(p, ctx->stream));
    return XB_OK;
}

}  // namespace

XB_API int xb_ctc_targets_dev(xb_ctx *ctx, const int32_t *d_seq_len, int n, int W, const char *templates, const int32_t *offsets,
                              int R, const int32_t *d_tmpl, const int8_t *d_strand, const int32_t *d_q_st, const int32_t *d_q_en,
                              const int32_t *d_r_st, const int32_t *d_r_en, const uint8_t *d_ops, const int32_t *d_n_ops,
                              double min_accuracy, double min_coverage, int ub_only, int ub_plus, int ub_minus, int32_t *d_mlen,
                              int32_t *d_blen, uint8_t *d_verdict, uint8_t *d_target, int32_t *d_target_len)
{
    if (!ctx) return XB_ERR_INVALID;
    const CtcIn i = {d_seq_len, d_tmpl, d_strand, d_q_st, d_q_en, d_r_st, d_r_en, d_ops, d_n_ops};
    const CtcOut o = {d_mlen, d_blen, d_verdict, d_target, d_target_len};
    if (!ctc_complete(i, o)) return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: null device pointer");
    if (int rc = enter(ctx, true)) return rc;
    return ctc_run(ctx, i, n, W, templates, offsets, R, {min_accuracy, min_coverage, ub_only, ub_plus, ub_minus}, o);
}

XB_API int xb_ctc_targets(xb_ctx *ctx, const int32_t *seq_len, int n, int W, const char *templates, const int32_t *offsets, int R,
                          const int32_t *tmpl, const int8_t *strand, const int32_t *q_st, const int32_t *q_en, const int32_t *r_st,
                          const int32_t *r_en, const uint8_t *ops, const int32_t *n_ops, double min_accuracy, double min_coverage,
                          int ub_only, int ub_plus, int ub_minus, int32_t *mlen, int32_t *blen, uint8_t *verdict, uint8_t *target,
                          int32_t *target_len)
{
    if (!ctx) return XB_ERR_INVALID;
    const CtcIn h = {seq_len, tmpl, strand, q_st, q_en, r_st, r_en, ops, n_ops};
    const CtcOut ho = {mlen, blen, verdict, target, target_len};
    if (!ctc_complete(h, ho)) return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: null host pointer");
    if (n < 1 || W < 1 || W > xb::MAP_MAX_ROW || R < 1)
        return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: n = %d rows of width %d, %d templates; need n >= 1, 1 <= W <= %d, R >= 1", n, W, R,
                    xb::MAP_MAX_ROW);
    int Lmax = 0;
    if (int rc = library_extent(ctx, "xb_ctc_targets", templates, offsets, R, &Lmax)) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t N = (size_t)n, cap = (size_t)W + Lmax, TW = (size_t)xb::ctc_target_width(Lmax);
    if (N * (cap + TW) > ((size_t)2 << 30)) return fail(ctx, XB_ERR_INVALID, "xb_ctc_targets: %d rows of width %d in one call; split the batch", n, W);
    Staging st{ctx};
    Staging::Piece<int32_t> i32[10];                    // seq_len, tmpl, q_st, q_en, r_st, r_en, n_ops | mlen, blen, target_len
    for (auto &piece : i32) piece = st.take<int32_t>(N);
    const auto d_strand = st.take<int8_t>(N);
    const auto d_verdict = st.take<uint8_t>(N), d_ops = st.take<uint8_t>(N * cap), d_target = st.take<uint8_t>(N * TW);
    if (int rc = st.ready()) return rc;
    const int32_t *const src[7] = {seq_len, tmpl, q_st, q_en, r_st, r_en, n_ops};
    for (int k = 0; k < 7; ++k) XB_HIP(ctx, hipMemcpyAsync(i32[k], src[k], N * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_strand, strand, N, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_ops, ops, N * cap, hipMemcpyHostToDevice, ctx->stream));
    const CtcIn d = {i32[0], i32[1], d_strand, i32[2], i32[3], i32[4], i32[5], d_ops, i32[6]};
    const CtcOut o = {i32[7], i32[8], d_verdict, d_target, i32[9]};
    if (int rc = ctc_run(ctx, d, n, W, templates, offsets, R, {min_accuracy, min_coverage, ub_only, ub_plus, ub_minus}, o)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(mlen, o.mlen, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(blen, o.blen, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(target_len, o.target_len, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(verdict, o.verdict, N, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(target, o.target, N * TW, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

XB_API int xb_ctc_chunks(xb_ctx *ctx, const float *signal, int n, const char *alphabet, const char *templates, const int32_t *offsets,
                         int R, int match, int mismatch, int gap_open, int gap_extend, int ambiguous, double min_accuracy,
                         double min_coverage, int ub_only, int ub_plus, int ub_minus, int8_t *seq, int32_t *seq_len, int32_t *tmpl,
                         int8_t *strand, int32_t *score, int32_t *second, int32_t *q_st, int32_t *q_en, int32_t *r_st, int32_t *r_en,
                         uint8_t *ops, int32_t *n_ops, int32_t *mlen, int32_t *blen, uint8_t *verdict, uint8_t *target,
                         int32_t *target_len)
{
    int rc = check_ready(ctx, n);
    if (rc) return rc;
    const MapOut hm = {tmpl, strand, score, second, q_st, q_en, r_st, r_en, ops, n_ops};
    if (!signal || !alphabet || !seq || !seq_len || !map_out_complete(hm) || !mlen || !blen || !verdict || !target || !target_len)
        return fail(ctx, XB_ERR_INVALID, "xb_ctc_chunks: null argument");
    if ((rc = check_alphabet(ctx, alphabet))) return rc;
    const int W = ctx->T;
    if (W > xb::MAP_MAX_ROW) return fail(ctx, XB_ERR_INVALID, "xb_ctc_chunks: rows of %d steps; the mapper takes %d", W, xb::MAP_MAX_ROW);
    int Lmax = 0;
    size_t total = 0;
    if ((rc = library_extent(ctx, "xb_ctc_chunks", templates, offsets, R, &Lmax, &total))) return rc;
    XB_HIP(ctx, hipSetDevice(ctx->device));
    // rows per mapper launch: what its cell budget (2 n W sum(L)) admits
    const double per_row = 2.0 * W * (double)total;
    const int fit = (int)std::min<double>((double)n, std::floor(MAP_CELL_BUDGET / per_row));
    if (fit < 1) return fail(ctx, XB_ERR_INVALID, "xb_ctc_chunks: one row of %d steps against %d letters is over the mapper's cell budget", W, offsets[R]);
    const size_t N = (size_t)n, cap = (size_t)W + Lmax, TW = (size_t)xb::ctc_target_width(Lmax);
    Staging st{ctx};
    Staging::Piece<int32_t> i32[11];                    // tmpl, score, second, q_st, q_en, r_st, r_en, n_ops | mlen, blen, target_len
    for (auto &piece : i32) piece = st.take<int32_t>(N);
    const auto d_strand = st.take<int8_t>(N);
    const auto d_verdict = st.take<uint8_t>(N), d_ops = st.take<uint8_t>(N * cap), d_target = st.take<uint8_t>(N * TW);
    if ((rc = st.ready())) return rc;
    XB_HIP(ctx, hipMemcpyAsync(ctx->d_signal, signal, sizeof(float) * N * ctx->cfg.chunk_len, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = basecall_async(ctx, ctx->d_signal, n, alphabet, ctx->seq, ctx->seq_len, {}))) return rc;
    if ((rc = join_async_decode(ctx))) return rc;
    const int sc[5] = {match, mismatch, gap_open, gap_extend, ambiguous};
    for (int a = 0; a < n; a += fit) {
        const int cnt = std::min(fit, n - a);
        const MapOut d = {i32[0] + a, d_strand + a, i32[1] + a, i32[2] + a, i32[3] + a, i32[4] + a, i32[5] + a, i32[6] + a,
                          d_ops + (size_t)a * cap, i32[7] + a};
        if ((rc = map_run(ctx, ctx->seq + (size_t)a * W, ctx->seq_len + a, cnt, W, templates, offsets, R, sc, d))) return rc;
    }
    const CtcIn ci = {ctx->seq_len, i32[0], d_strand, i32[3], i32[4], i32[5], i32[6], d_ops, i32[7]};
    const CtcOut co = {i32[8], i32[9], d_verdict, d_target, i32[10]};
    if ((rc = ctc_run(ctx, ci, n, W, templates, offsets, R, {min_accuracy, min_coverage, ub_only, ub_plus, ub_minus}, co))) return rc;
    XB_HIP(ctx, hipMemcpyAsync(seq, ctx->seq, N * W, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(seq_len, ctx->seq_len, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    int32_t *const h_i32[11] = {tmpl, score, second, q_st, q_en, r_st, r_en, n_ops, mlen, blen, target_len};
    for (int k = 0; k < 11; ++k) XB_HIP(ctx, hipMemcpyAsync(h_i32[k], i32[k], N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(strand, d_strand, N, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(verdict, co.verdict, N, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ops, d_ops, N * cap, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(target, co.target, N * TW, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// ---- per-position UB accuracy of mapped rows (xb_ub_tally) --------------------------------------------------------------
namespace {

struct UbIn {
    const int8_t *seq; const int32_t *seq_len, *tmpl; const int8_t *strand; const int32_t *q_st, *r_st, *r_en; const uint8_t *ops;
    const int32_t *n_ops;
};
struct UbOut {
    int32_t *counts, *reads, *err; int64_t *cm;
};

bool ub_complete(const UbIn &i, const UbOut &o)
{
    return i.seq && i.seq_len && i.tmpl && i.strand && i.q_st && i.r_st && i.r_en && i.ops && i.n_ops && o.counts && o.reads && o.err && o.cm;
}

// validation, the library's device image, the launch: i and o are device pointers
int ub_run(xb_ctx *ctx, const UbIn &i, int n, int W, const char *templates, const int32_t *offsets, int R, const UbOut &o)
{
    int Lmax = 0;
    if (int rc = map_library(ctx, "xb_ub_tally", n, W, templates, offsets, R, nullptr, &Lmax)) return rc;
    xb::UbTallyParams p{};
    p.seq = i.seq; p.seq_len = i.seq_len; p.n = n; p.W = W; p.cap = W + Lmax;
    p.tmpl = i.tmpl; p.strand = i.strand; p.q_st = i.q_st; p.r_st = i.r_st; p.r_en = i.r_en; p.ops = i.ops; p.n_ops = i.n_ops;
    p.tcodes = ctx->map.tcodes(); p.toff = ctx->map.toff();
    p.R = R; p.total = offsets[R];
    p.counts = o.counts; p.reads = o.reads; p.err = o.err;
    p.cm = reinterpret_cast<unsigned long long *>(o.cm);
    XB_HIP(ctx, xb::launch_ub_tally(p, ctx->stream));
    return XB_OK;
}

}  // namespace

XB_API int xb_ub_tally_dev(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int W, const char *templates,
                           const int32_t *offsets, int R, const int32_t *d_tmpl, const int8_t *d_strand, const int32_t *d_q_st,
                           const int32_t *d_r_st, const int32_t *d_r_en, const uint8_t *d_ops, const int32_t *d_n_ops,
                           int32_t *d_counts, int32_t *d_reads, int32_t *d_err, int64_t *d_cm)
{
    if (!ctx) return XB_ERR_INVALID;
    const UbIn i = {d_seq, d_seq_len, d_tmpl, d_strand, d_q_st, d_r_st, d_r_en, d_ops, d_n_ops};
    const UbOut o = {d_counts, d_reads, d_err, d_cm};
    if (!ub_complete(i, o)) return fail(ctx, XB_ERR_INVALID, "xb_ub_tally: null device pointer");
    if (int rc = enter(ctx, true)) return rc;
    return ub_run(ctx, i, n, W, templates, offsets, R, o);
}

XB_API int xb_ub_tally(xb_ctx *ctx, const int8_t *seq, const int32_t *seq_len, int n, int W, const char *templates,
                       const int32_t *offsets, int R, const int32_t *tmpl, const int8_t *strand, const int32_t *q_st,
                       const int32_t *r_st, const int32_t *r_en, const uint8_t *ops, const int32_t *n_ops, int32_t *counts,
                       int32_t *reads, int32_t *err, int64_t *cm)
{
    if (!ctx) return XB_ERR_INVALID;
    const UbIn h = {seq, seq_len, tmpl, strand, q_st, r_st, r_en, ops, n_ops};
    const UbOut ho = {counts, reads, err, cm};
    if (!ub_complete(h, ho)) return fail(ctx, XB_ERR_INVALID, "xb_ub_tally: null host pointer");
    if (n < 1 || W < 1 || W > xb::MAP_MAX_ROW || !offsets || R < 1 || offsets[0] != 0)
        return fail(ctx, XB_ERR_INVALID, "xb_ub_tally: n = %d rows of width %d, %d templates; need n >= 1, 1 <= W <= %d, R >= 1", n, W, R,
                    xb::MAP_MAX_ROW);
    int Lmax = 0;
    size_t total = 0;
    if (int rc = library_extent(ctx, "xb_ub_tally", templates, offsets, R, &Lmax, &total)) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t N = (size_t)n, cap = (size_t)W + Lmax;
    if (N * (cap + W) > ((size_t)2 << 30)) return fail(ctx, XB_ERR_INVALID, "xb_ub_tally: %d rows of width %d in one call; split the batch", n, W);
    const size_t b_reads = (size_t)R * 2 * 4, b_err = 2 * total * 4, b_cm = (size_t)xb::UB_CM_ROWS * xb::UB_CM_COLS * 8;
    Staging st{ctx};
    Staging::Piece<int32_t> i32[6];                     // seq_len, tmpl, q_st, r_st, r_en, n_ops
    for (auto &piece : i32) piece = st.take<int32_t>(N);
    const auto d_strand = st.take<int8_t>(N), d_seq = st.take<int8_t>(N * W);
    const auto d_ops = st.take<uint8_t>(N * cap);
    const auto d_counts = st.take<int32_t>(N * xb::UB_COUNTS), d_reads = st.take<int32_t>(b_reads / 4), d_err = st.take<int32_t>(b_err / 4);
    const auto d_cm = st.take<int64_t>(b_cm / 8);
    if (int rc = st.ready()) return rc;
    const int32_t *const src[6] = {seq_len, tmpl, q_st, r_st, r_en, n_ops};
    for (int k = 0; k < 6; ++k) XB_HIP(ctx, hipMemcpyAsync(i32[k], src[k], N * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_strand, strand, N, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_seq, seq, N * W, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_ops, ops, N * cap, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_reads, reads, b_reads, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_err, err, b_err, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_cm, cm, b_cm, hipMemcpyHostToDevice, ctx->stream));
    const UbIn d = {d_seq, i32[0], i32[1], d_strand, i32[2], i32[3], i32[4], d_ops, i32[5]};
    const UbOut o = {d_counts, d_reads, d_err, d_cm};
    if (int rc = ub_run(ctx, d, n, W, templates, offsets, R, o)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(counts, o.counts, N * xb::UB_COUNTS * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(reads, o.reads, b_reads, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(err, o.err, b_err, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(cm, o.cm, b_cm, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// ---- barcode distance of mapped rows (xb_barcode_dist) ------------------------------------------------------------------
namespace {

struct BcIn {
    const int8_t *seq; const int32_t *seq_len, *tmpl; const int8_t *strand; const int32_t *q_st, *r_st;
};
struct BcOut {
    int32_t *dist, *start, *end, *obs_len;
};
struct BcRule {
    int bc_pos, bc_len, relax;
};

bool bc_complete(const BcIn &i, const BcOut &o)
{
    return i.seq && i.seq_len && i.tmpl && i.strand && i.q_st && i.r_st && o.dist && o.start && o.end && o.obs_len;
}

// the limits of the contract, before anything is staged or launched
int bc_check(xb_ctx *ctx, const BcRule &rule)
{
    if (rule.bc_pos < 0 || rule.bc_pos > xb::BC_MAX_POS || rule.bc_len < 1 || rule.bc_len > xb::BC_MAX_LEN || rule.relax < 0 ||
        rule.relax > xb::BC_MAX_RELAX)
        return fail(ctx, XB_ERR_INVALID, "xb_barcode_dist: bc_pos = %d, bc_len = %d, relax = %d; need 0 <= bc_pos <= %d, 1 <= bc_len <= %d, "
                    "0 <= relax <= %d", rule.bc_pos, rule.bc_len, rule.relax, xb::BC_MAX_POS, xb::BC_MAX_LEN, xb::BC_MAX_RELAX);
    return XB_OK;
}

// validation, the library's device image, the launch: i and o are device pointers
int bc_run(xb_ctx *ctx, const BcIn &i, int n, int W, const char *templates, const int32_t *offsets, int R, const BcRule &rule,
           const BcOut &o)
{
    if (int rc = bc_check(ctx, rule)) return rc;
    int Lmax = 0;
    if (int rc = map_library(ctx, "xb_barcode_dist", n, W, templates, offsets, R, nullptr, &Lmax)) return rc;
    xb::BarcodeDistParams p{};
    p.seq = i.seq; p.seq_len = i.seq_len; p.n = n; p.W = W;
    p.tmpl = i.tmpl; p.strand = i.strand; p.q_st = i.q_st; p.r_st = i.r_st;
    p.tletters = ctx->map.tletters(); p.toff = ctx->map.toff();
    p.R = R;
    p.bc_pos = rule.bc_pos; p.bc_len = rule.bc_len; p.relax = rule.relax;
    p.dist = o.dist; p.start = o.start; p.end = o.end; p.obs_len = o.obs_len;
    XB_HIP(ctx, xb::launch_barcode_dist(p, ctx->stream));
    return XB_OK;
}

}  // namespace

XB_API int xb_barcode_dist_dev(xb_ctx *ctx, const int8_t *d_seq, const int32_t *d_seq_len, int n, int W, const char *templates,
                               const int32_t *offsets, int R, const int32_t *d_tmpl, const int8_t *d_strand, const int32_t *d_q_st,
                               const int32_t *d_r_st, int bc_pos, int bc_len, int relax, int32_t *d_bc_dist, int32_t *d_bc_start,
                               int32_t *d_bc_end, int32_t *d_bc_obs_len)
{
    if (!ctx) return XB_ERR_INVALID;
    const BcIn i = {d_seq, d_seq_len, d_tmpl, d_strand, d_q_st, d_r_st};
    const BcOut o = {d_bc_dist, d_bc_start, d_bc_end, d_bc_obs_len};
    if (!bc_complete(i, o)) return fail(ctx, XB_ERR_INVALID, "xb_barcode_dist: null device pointer");
    if (int rc = enter(ctx, true)) return rc;
    return bc_run(ctx, i, n, W, templates, offsets, R, {bc_pos, bc_len, relax}, o);
}

XB_API int xb_barcode_dist(xb_ctx *ctx, const int8_t *seq, const int32_t *seq_len, int n, int W, const char *templates,
                           const int32_t *offsets, int R, const int32_t *tmpl, const int8_t *strand, const int32_t *q_st,
                           const int32_t *r_st, int bc_pos, int bc_len, int relax, int32_t *bc_dist, int32_t *bc_start, int32_t *bc_end,
                           int32_t *bc_obs_len)
{
    if (!ctx) return XB_ERR_INVALID;
    const BcIn h = {seq, seq_len, tmpl, strand, q_st, r_st};
    const BcOut ho = {bc_dist, bc_start, bc_end, bc_obs_len};
    if (!bc_complete(h, ho)) return fail(ctx, XB_ERR_INVALID, "xb_barcode_dist: null host pointer");
    if (n < 1 || W < 1 || W > xb::MAP_MAX_ROW || !offsets || R < 1 || offsets[0] != 0)
        return fail(ctx, XB_ERR_INVALID, "xb_barcode_dist: n = %d rows of width %d, %d templates; need n >= 1, 1 <= W <= %d, R >= 1", n, W, R,
                    xb::MAP_MAX_ROW);
    if (int rc = bc_check(ctx, {bc_pos, bc_len, relax})) return rc;
    int Lmax = 0;
    if (int rc = library_extent(ctx, "xb_barcode_dist", templates, offsets, R, &Lmax)) return rc;
    if (int rc = enter(ctx, false)) return rc;
    const size_t N = (size_t)n;
    if (N * W > ((size_t)2 << 30)) return fail(ctx, XB_ERR_INVALID, "xb_barcode_dist: %d rows of width %d in one call; split the batch", n, W);
    Staging st{ctx};
    Staging::Piece<int32_t> i32[8];                     // seq_len, tmpl, q_st, r_st | bc_dist, bc_start, bc_end, bc_obs_len
    for (auto &piece : i32) piece = st.take<int32_t>(N);
    const auto d_strand = st.take<int8_t>(N), d_seq = st.take<int8_t>(N * W);
    if (int rc = st.ready()) return rc;
    const int32_t *const src[4] = {seq_len, tmpl, q_st, r_st};
    for (int k = 0; k < 4; ++k) XB_HIP(ctx, hipMemcpyAsync(i32[k], src[k], N * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_strand, strand, N, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_seq, seq, N * W, hipMemcpyHostToDevice, ctx->stream));
    const BcIn d = {d_seq, i32[0], i32[1], d_strand, i32[2], i32[3]};
    const BcOut o = {i32[4], i32[5], i32[6], i32[7]};
    if (int rc = bc_run(ctx, d, n, W, templates, offsets, R, {bc_pos, bc_len, relax}, o)) return rc;
    int32_t *const dst[4] = {bc_dist, bc_start, bc_end, bc_obs_len};
    for (int k = 0; k < 4; ++k) XB_HIP(ctx, hipMemcpyAsync(dst[k], i32[4 + k], N * 4, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// ---- DTW signal segmentation (xb_dtw_segment) -------------------------------------------------------------------------
namespace {

// Choice-bit scratch one launch may own (XB_DTW_SCRATCH_MB, default 1024): a call is split into launches of as many chunks
// as fit, one chunk when a single chunk needs more (at most 136 MB: 65535 samples against 32768 columns).  A full-size chunk
// (3600 samples, 1200 columns) takes 488 KB, so the default holds 2201 chunks -- two waves on each of the 1024 SIMDs.
size_t dtw_scratch_bound()
{
    long mb = 1024;
    if (const char *e = getenv("XB_DTW_SCRATCH_MB")) mb = atol(e);
    if (mb < 1) mb = 1;
    if (mb > 65536) mb = 65536;
    return (size_t)mb << 20;
}

struct DtwOut {
    int32_t *bp; int8_t *ok; double *cost;
};

// validation, the offsets' device copy, the launches: signal, levels, window and o are device pointers, offsets is host
int dtw_run(xb_ctx *ctx, const float *d_signal, int n, int N, const double *d_levels, const int32_t *offsets, int ref_rep,
            const double *d_window, bool band, int Kmax, const DtwOut &o)
{
    if (n < 1 || N < 1 || N > xb::DTW_MAX_SAMPLES || ref_rep < 1 || ref_rep > xb::DTW_MAX_COLUMNS)
        return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: n = %d chunks of %d samples, ref_rep = %d; need n >= 1, 1 <= N <= %d, "
                    "1 <= ref_rep <= %d", n, N, ref_rep, xb::DTW_MAX_SAMPLES, xb::DTW_MAX_COLUMNS);
    if (!offsets || offsets[0] != 0) return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: offsets must start at 0");
    int Kbig = 0;
    for (int c = 0; c < n; ++c) {
        const int K = offsets[c + 1] - offsets[c];
        if (K < 1 || (int64_t)K * ref_rep > xb::DTW_MAX_COLUMNS)
            return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: chunk %d has %d levels, %lld columns at ref_rep = %d; 1 level .. %d "
                        "columns are supported", c, K, (long long)K * ref_rep, ref_rep, xb::DTW_MAX_COLUMNS);
        Kbig = std::max(Kbig, K);
    }
    if (Kmax < Kbig)
        return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: breakpoint rows of %d entries, the longest chunk has %d levels", Kmax, Kbig);
    const int cols = xb::dtw_cols_per_lane(Kbig * ref_rep);
    size_t choice = 0;
    for (int c = 0; c < n; ++c) choice = std::max(choice, xb::dtw_choice_words(N, (offsets[c + 1] - offsets[c]) * ref_rep, cols));
    const size_t slot_words = choice + 2 * (size_t)N;
    const size_t per_launch = std::max<size_t>(1, std::min<size_t>((size_t)n, dtw_scratch_bound() / (slot_words * 8)));
    xb_ctx::DtwState &s = ctx->dtw;
    if (int rc = grow(ctx, &s.scratch, per_launch * slot_words * 8)) return rc;
    // the offsets: pinned slot (calls & 1), free again once the copy of two calls ago has run
    xb_ctx::DtwState::Slot &slot = s.off[s.calls++ & 1];
    if (slot.copied) XB_HIP(ctx, hipEventSynchronize(slot.copied));
    else XB_HIP(ctx, hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
    if (slot.count < (size_t)n + 1) {
        XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (slot.h) (void)hipHostFree(slot.h);
        slot.h = nullptr;
        slot.d.release();
        slot.count = 0;
        const size_t count = ((size_t)n + 1 + 1023) & ~(size_t)1023;
        XB_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&slot.h), count * sizeof(int32_t), hipHostMallocDefault));
        if (int rc = slot.d.alloc(ctx, count * sizeof(int32_t))) return rc;
        slot.count = count;
    }
    memcpy(slot.h, offsets, sizeof(int32_t) * ((size_t)n + 1));
    XB_HIP(ctx, hipMemcpyAsync(slot.d.p, slot.h, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipEventRecord(slot.copied, ctx->stream));
    xb::DtwParams p{};
    p.signal = d_signal; p.levels = d_levels; p.off = static_cast<const int32_t *>(slot.d.p); p.window = band ? d_window : nullptr;
    p.N = N; p.rep = ref_rep; p.Kmax = Kmax;
    p.scratch = static_cast<unsigned long long *>(s.scratch.p);
    p.choice_words = choice; p.slot_words = slot_words;
    p.bp = o.bp; p.ok = o.ok; p.cost = o.cost;
    s.scratch_written = 0;
    for (int c = 0; c < n; ++c) s.scratch_written += 8 * xb::dtw_choice_words(N, (offsets[c + 1] - offsets[c]) * ref_rep, cols);
    for (size_t first = 0; first < (size_t)n; first += per_launch) {
        p.first = (int)first;
        p.count = (int)std::min<size_t>(per_launch, (size_t)n - first);
        XB_HIP(ctx, xb::launch_dtw(p, cols, band, ctx->stream));
    }
    return XB_OK;
}

}  // namespace

XB_API int xb_dtw_segment_dev(xb_ctx *ctx, const float *d_signal, int n, int N, const double *d_levels, const int32_t *offsets,
                              int ref_rep, const double *d_window, int Kmax, int32_t *d_breakpoints, int8_t *d_ok, double *d_cost)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_signal || !d_levels || !d_breakpoints || !d_ok || !d_cost) return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: null device pointer");
    if (int rc = enter(ctx, true)) return rc;
    return dtw_run(ctx, d_signal, n, N, d_levels, offsets, ref_rep, d_window, d_window != nullptr, Kmax, {d_breakpoints, d_ok, d_cost});
}

XB_API int xb_dtw_segment(xb_ctx *ctx, const float *signal, int n, int N, const double *levels, const int32_t *offsets, int ref_rep,
                          const double *window, int Kmax, int32_t *breakpoints, int8_t *ok, double *cost)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!signal || !levels || !breakpoints || !ok || !cost) return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: null host pointer");
    if (n < 1 || N < 1 || N > xb::DTW_MAX_SAMPLES || !offsets || offsets[0] != 0 || Kmax < 1 || Kmax > xb::DTW_MAX_COLUMNS)
        return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: n = %d chunks of %d samples, breakpoint rows of %d entries; need n >= 1, "
                    "1 <= N <= %d, offsets from 0 with a level or more per chunk, 1 <= Kmax <= %d", n, N, Kmax, xb::DTW_MAX_SAMPLES,
                    xb::DTW_MAX_COLUMNS);
    for (int c = 0; c < n; ++c)
        if (offsets[c + 1] <= offsets[c]) return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: chunk %d has %d levels; at least one is needed",
                                                      c, offsets[c + 1] - offsets[c]);
    if (int rc = enter(ctx, false)) return rc;
    bool band = false;
    for (int c = 0; window && c < n; ++c) band = band || window[c] >= 0.0;
    const size_t C = (size_t)n, total = (size_t)offsets[n];
    Staging st{ctx};
    const auto d_sig = st.take<float>(C * N);
    const auto d_lev = st.take<double>(total), d_win = st.take<double>(C), d_cost = st.take<double>(C);
    const auto d_bp = st.take<int32_t>(C * Kmax);
    const auto d_ok = st.take<int8_t>(C);
    if (st.used > ((size_t)2 << 30)) return fail(ctx, XB_ERR_INVALID, "xb_dtw_segment: %d chunks of %d samples in one call; split the batch", n, N);
    if (int rc = st.ready()) return rc;
    XB_HIP(ctx, hipMemcpyAsync(d_sig, signal, C * N * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_lev, levels, total * 8, hipMemcpyHostToDevice, ctx->stream));
    if (band) XB_HIP(ctx, hipMemcpyAsync(d_win, window, C * 8, hipMemcpyHostToDevice, ctx->stream));
    const DtwOut o = {d_bp, d_ok, d_cost};
    if (int rc = dtw_run(ctx, d_sig, n, N, d_lev, offsets, ref_rep, d_win, band, Kmax, o)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(breakpoints, o.bp, C * Kmax * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ok, o.ok, C, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(cost, o.cost, C * 8, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

XB_API int64_t xb_dtw_scratch_bytes(const xb_ctx *ctx) { return ctx ? (int64_t)ctx->dtw.scratch_written : 0; }

// ---- XNA spliced augmentation (xb_splice_library, xb_splice_chunks) ---------------------------------------------------
XB_API int xb_splice_library(xb_ctx *ctx, const uint16_t *pool, int64_t pool_len, const int32_t *rows, int n_rows,
                             const int32_t *table, int table_len)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!pool || !rows || !table) return fail(ctx, XB_ERR_INVALID, "xb_splice_library: null host pointer");
    if (pool_len < 1 || pool_len > 0x7fffffffLL || n_rows < 1 || table_len != xb::SPLICE_TABLE_LEN)
        return fail(ctx, XB_ERR_INVALID, "xb_splice_library: a pool of %lld samples, %d rows, a table of %d groups; need 1 <= pool < 2^31, "
                    "n_rows >= 1 and %d groups", (long long)pool_len, n_rows, table_len, xb::SPLICE_TABLE_LEN);
    for (int r = 0; r < n_rows; ++r) {
        const int64_t off = rows[2 * r], len = rows[2 * r + 1];
        if (off < 0 || len < 1 || len > xb::SPLICE_MAX_KMER || off + len > pool_len)
            return fail(ctx, XB_ERR_INVALID, "xb_splice_library: row %d has %lld samples at offset %lld of a pool of %lld; 1 .. %d samples "
                        "inside the pool are supported", r, (long long)len, (long long)off, (long long)pool_len, xb::SPLICE_MAX_KMER);
    }
    for (int g = 0; g < table_len; ++g) {
        const int64_t first = table[2 * g], count = table[2 * g + 1];
        if (count < 0 || (count > 0 && (first < 0 || first + count > n_rows)))
            return fail(ctx, XB_ERR_INVALID, "xb_splice_library: group %d holds rows %lld .. %lld of %d", g, (long long)first,
                        (long long)(first + count), n_rows);
    }
    if (int rc = enter(ctx, false)) return rc;
    xb_ctx::SpliceState &s = ctx->splice;
    s.loaded = false;
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));                     // nothing in flight reads the library it replaces
    if (int rc = grow(ctx, &s.pool, (size_t)pool_len * 2)) return rc;
    if (int rc = grow(ctx, &s.rows, (size_t)n_rows * 8)) return rc;
    if (int rc = grow(ctx, &s.table, (size_t)table_len * 8)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(s.pool.p, pool, (size_t)pool_len * 2, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(s.rows.p, rows, (size_t)n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(s.table.p, table, (size_t)table_len * 8, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s.loaded = true;
    return XB_OK;
}

namespace {

struct SpliceArgs {
    int n, N, Lt;
    int64_t first_index;
    uint64_t seed;
    int ubs_mask;
    double prop, var_prop;
    int cand, pad;
};

// the limits of the contract, before any launch
int splice_check(xb_ctx *ctx, const SpliceArgs &a)
{
    if (!ctx->splice.loaded) return fail(ctx, XB_ERR_STATE, "xb_splice_chunks: no library: call xb_splice_library first");
    if (a.n < 1 || a.N < 1 || a.N > xb::SPLICE_MAX_SAMPLES || a.Lt < 1 || a.Lt > xb::SPLICE_MAX_LABELS)
        return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: n = %d chunks of %d samples, label rows of %d entries; need n >= 1, "
                    "1 <= N <= %d, 1 <= Lt <= %d", a.n, a.N, a.Lt, xb::SPLICE_MAX_SAMPLES, xb::SPLICE_MAX_LABELS);
    if (a.cand < 1 || a.cand > xb::SPLICE_MAX_CAND)
        return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: cand_sample_size = %d; 1 .. %d are supported", a.cand, xb::SPLICE_MAX_CAND);
    if (a.pad < 0) return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: pad = %d is negative", a.pad);
    if (a.ubs_mask < 1 || a.ubs_mask > 3) return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: ubs_mask = %d; 1 (X), 2 (Y) or 3 (both)", a.ubs_mask);
    if (!(a.prop >= 0.0) || !(a.var_prop >= 0.0) || !(a.prop + a.var_prop <= 1.0))
        return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: prop = %g, var_prop = %g; both at least 0, their sum at most 1", a.prop, a.var_prop);
    if (a.first_index < 0) return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: first_index = %lld is negative", (long long)a.first_index);
    return XB_OK;
}

int splice_run(xb_ctx *ctx, const SpliceArgs &a, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
               const uint16_t *d_bkps, float *d_out_signal, uint8_t *d_out_targets, int8_t *d_success, int32_t *d_inserted)
{
    xb::SpliceParams p{};
    p.signal = d_signal; p.targets = d_targets; p.lengths = d_lengths; p.bkps = d_bkps;
    p.n = a.n; p.N = a.N; p.Lt = a.Lt;
    p.first_index = (unsigned long long)a.first_index; p.seed = a.seed;
    p.n_ubs = 0;
    if (a.ubs_mask & 1) p.ubs[p.n_ubs++] = 5;
    if (a.ubs_mask & 2) p.ubs[p.n_ubs++] = 6;
    p.prop = a.prop; p.var_prop = a.var_prop; p.cand = a.cand; p.pad = a.pad;
    p.pool = static_cast<const xb::half_t *>(ctx->splice.pool.p);
    p.rows = static_cast<const int32_t *>(ctx->splice.rows.p);
    p.table = static_cast<const int32_t *>(ctx->splice.table.p);
    p.out_signal = d_out_signal; p.out_targets = d_out_targets; p.success = d_success; p.inserted = d_inserted;
    XB_HIP(ctx, xb::launch_splice(p, ctx->stream));
    return XB_OK;
}

}  // namespace

XB_API int xb_splice_chunks_dev(xb_ctx *ctx, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
                                const uint16_t *d_breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                                double prop, double var_prop, int cand_sample_size, int pad, float *d_out_signal,
                                uint8_t *d_out_targets, int8_t *d_success, int32_t *d_inserted)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!d_signal || !d_targets || !d_lengths || !d_breakpoints || !d_out_signal || !d_out_targets || !d_success || !d_inserted)
        return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: null device pointer");
    if (d_signal == d_out_signal || d_targets == d_out_targets) return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: outputs alias inputs");
    const SpliceArgs a{n, N, Lt, first_index, seed, ubs_mask, prop, var_prop, cand_sample_size, pad};
    if (int rc = splice_check(ctx, a)) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return splice_run(ctx, a, d_signal, d_targets, d_lengths, d_breakpoints, d_out_signal, d_out_targets, d_success, d_inserted);
}

XB_API int xb_splice_chunks(xb_ctx *ctx, const float *signal, const uint8_t *targets, const int32_t *lengths,
                            const uint16_t *breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                            double prop, double var_prop, int cand_sample_size, int pad, float *out_signal, uint8_t *out_targets,
                            int8_t *success, int32_t *inserted)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!signal || !targets || !lengths || !breakpoints || !out_signal || !out_targets || !success || !inserted)
        return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: null host pointer");
    const SpliceArgs a{n, N, Lt, first_index, seed, ubs_mask, prop, var_prop, cand_sample_size, pad};
    if (int rc = splice_check(ctx, a)) return rc;
    for (int c = 0; c < n; ++c) {                                       // what the kernel would otherwise clamp
        const int len = lengths[c];
        if (len < 0 || len > Lt) return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: chunk %d has %d labels in a row of %d", c, len, Lt);
        const uint16_t *b = breakpoints + (size_t)c * Lt;
        for (int l = 0; l < len; ++l)
            if (b[l] > N || (l && b[l] < b[l - 1]))
                return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: chunk %d: breakpoint %d of base %d (the one before: %d, samples: %d)", c,
                            (int)b[l], l, l ? (int)b[l - 1] : 0, N);
    }
    if (int rc = enter(ctx, false)) return rc;
    const size_t C = (size_t)n;
    Staging st{ctx};
    const auto d_sig = st.take<float>(C * N), d_out = st.take<float>(C * N);
    const auto d_ins = st.take<int32_t>(C), d_len = st.take<int32_t>(C);
    const auto d_bk = st.take<uint16_t>(C * Lt);
    const auto d_t = st.take<uint8_t>(C * Lt), d_ot = st.take<uint8_t>(C * Lt);
    const auto d_ok = st.take<int8_t>(C);
    if (st.used > ((size_t)2 << 30)) return fail(ctx, XB_ERR_INVALID, "xb_splice_chunks: %d chunks of %d samples in one call; split the batch", n, N);
    if (int rc = st.ready()) return rc;
    XB_HIP(ctx, hipMemcpyAsync(d_sig, signal, C * N * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_len, lengths, C * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_bk, breakpoints, C * Lt * 2, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_t, targets, C * Lt, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = splice_run(ctx, a, d_sig, d_t, d_len, d_bk, d_out, d_ot, d_ok, d_ins)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(out_signal, d_out, C * N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(out_targets, d_ot, C * Lt, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(success, d_ok, C, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(inserted, d_ins, C * 4, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

// ---- XNA synthetic spiking (xb_spike_model, xb_spike_chunks) -----------------------------------------------------------
XB_API int xb_spike_model(xb_ctx *ctx, const double *mean, const double *stdv, int64_t n)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!mean || !stdv) return fail(ctx, XB_ERR_INVALID, "xb_spike_model: null host pointer");
    if (n != xb::SPIKE_MODEL_KMERS)
        return fail(ctx, XB_ERR_INVALID, "xb_spike_model: a table of %lld k-mers; need 7^6 = %d", (long long)n, xb::SPIKE_MODEL_KMERS);
    std::vector<double> rows(2 * (size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const double m = mean[k], s = stdv[k];
        if (m == m && (std::isinf(m) || !(s >= 0.0) || std::isinf(s)))
            return fail(ctx, XB_ERR_INVALID, "xb_spike_model: k-mer %lld has mean %g, stdv %g; a finite mean (or NaN: no such k-mer) "
                        "and a finite stdv >= 0 are supported", (long long)k, m, s);
        rows[2 * k] = m;
        rows[2 * k + 1] = m == m ? s : 0.0;
    }
    if (int rc = enter(ctx, false)) return rc;
    xb_ctx::SpikeState &s = ctx->spike;
    s.loaded = false;
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));                     // nothing in flight reads the table it replaces
    if (int rc = grow(ctx, &s.model, rows.size() * 8)) return rc;
    XB_HIP(ctx, hipMemcpyAsync(s.model.p, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s.loaded = true;
    return XB_OK;
}

namespace {

struct SpikeArgs {
    int n, N, Lt;
    int64_t first_index;
    uint64_t seed;
    int ubs_mask;
    double prop, var_prop;
    int pad, dist_rows;
    const double *phi;
    double noise_std;
    int variable_noise;
};
struct SpikeIn {
    const float *signal; const uint8_t *targets; const int32_t *lengths; const uint16_t *bkps;
};
struct SpikeOut {
    float *signal; uint8_t *targets; int32_t *spiked; double *med, *mad; int8_t *status;
};
// the two entry points over one model and one argument list: windows around the positions, or the whole chunk
struct SpikeCall {
    const char *who;
    hipError_t (*launch)(const xb::SpikeParams &, hipStream_t);
};
constexpr SpikeCall SPIKE_WINDOWS{"xb_spike_chunks", xb::launch_spike}, SPIKE_WHOLE{"xb_synth_chunks", xb::launch_synth};

bool spike_complete(const SpikeIn &i, const SpikeOut &o)
{
    return i.signal && i.targets && i.lengths && i.bkps && o.signal && o.targets && o.spiked && o.med && o.mad && o.status;
}

// the limits of the contract, before any launch
int spike_check(xb_ctx *ctx, const char *who, const SpikeArgs &a)
{
    if (!ctx->spike.loaded) return fail(ctx, XB_ERR_STATE, "%s: no model: call xb_spike_model first", who);
    if (a.n < 1 || a.N < 1 || a.N > xb::SPLICE_MAX_SAMPLES || a.Lt < 1 || a.Lt > xb::SPLICE_MAX_LABELS)
        return fail(ctx, XB_ERR_INVALID, "%s: n = %d chunks of %d samples, label rows of %d entries; need n >= 1, "
                    "1 <= N <= %d, 1 <= Lt <= %d", who, a.n, a.N, a.Lt, xb::SPLICE_MAX_SAMPLES, xb::SPLICE_MAX_LABELS);
    if (a.pad < 0) return fail(ctx, XB_ERR_INVALID, "%s: pad = %d is negative", who, a.pad);
    if (a.ubs_mask < 0 || a.ubs_mask > 3)
        return fail(ctx, XB_ERR_INVALID, "%s: ubs_mask = %d; 0 (none), 1 (X), 2 (Y) or 3 (both)", who, a.ubs_mask);
    if (!(a.prop >= 0.0) || !(a.var_prop >= 0.0) || !(a.prop + a.var_prop <= 1.0))
        return fail(ctx, XB_ERR_INVALID, "%s: prop = %g, var_prop = %g; both at least 0, their sum at most 1", who, a.prop, a.var_prop);
    if (a.first_index < 0) return fail(ctx, XB_ERR_INVALID, "%s: first_index = %lld is negative", who, (long long)a.first_index);
    if (a.dist_rows < 0 || a.dist_rows > xb::SPIKE_MAX_ROWS)
        return fail(ctx, XB_ERR_INVALID, "%s: dist_rows = %d; 0 (uniform) .. %d shift values are supported", who, a.dist_rows,
                    xb::SPIKE_MAX_ROWS);
    if (!(a.noise_std >= 0.0) || std::isinf(a.noise_std))
        return fail(ctx, XB_ERR_INVALID, "%s: noise_std = %g; a finite value >= 0 is supported", who, a.noise_std);
    // the rows the kernel reads: every quantile pa + unit * pw must stay inside (0, 1) and normal
    for (int r = 0; r <= a.dist_rows; ++r) {
        if (r == a.dist_rows && !(a.noise_std > 0.0)) break;
        if (!a.phi) return fail(ctx, XB_ERR_INVALID, "%s: null distribution table", who);
        const double pa = a.phi[2 * r], pw = a.phi[2 * r + 1];
        if (!(pa >= 1e-300) || !(pw > 0.0) || !(pa + pw < 1.0))
            return fail(ctx, XB_ERR_INVALID, "%s: distribution row %d is Phi(a) = %g, Phi(b) - Phi(a) = %g; need "
                        "1e-300 <= Phi(a), 0 < Phi(b) - Phi(a), Phi(b) < 1", who, r, pa, pw);
    }
    return XB_OK;
}

// the launch: i and o are device pointers
int spike_run(xb_ctx *ctx, const SpikeCall &call, const SpikeArgs &a, const SpikeIn &i, const SpikeOut &o)
{
    xb::SpikeParams p{};
    p.signal = i.signal; p.targets = i.targets; p.lengths = i.lengths; p.bkps = i.bkps;
    p.n = a.n; p.N = a.N; p.Lt = a.Lt;
    p.first_index = (unsigned long long)a.first_index; p.seed = a.seed;
    p.ubs_mask = a.ubs_mask; p.prop = a.prop; p.var_prop = a.var_prop; p.pad = a.pad;
    p.dist_rows = a.dist_rows;
    for (int r = 0; r <= a.dist_rows; ++r) {
        const bool read = r < a.dist_rows || a.noise_std > 0.0;
        p.phi[r][0] = read ? a.phi[2 * r] : 0.25;
        p.phi[r][1] = read ? a.phi[2 * r + 1] : 0.5;
    }
    p.noise_std = a.noise_std; p.variable_noise = a.variable_noise != 0;
    p.model = static_cast<const double *>(ctx->spike.model.p);
    p.out_signal = o.signal; p.out_targets = o.targets; p.spiked = o.spiked; p.med = o.med; p.mad = o.mad; p.status = o.status;
    XB_HIP(ctx, call.launch(p, ctx->stream));
    return XB_OK;
}

// the _dev form of either entry point
int spike_dev(xb_ctx *ctx, const SpikeCall &call, const SpikeArgs &a, const SpikeIn &i, const SpikeOut &o)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!spike_complete(i, o)) return fail(ctx, XB_ERR_INVALID, "%s: null device pointer", call.who);
    if (i.signal == o.signal || i.targets == o.targets) return fail(ctx, XB_ERR_INVALID, "%s: outputs alias inputs", call.who);
    if (int rc = spike_check(ctx, call.who, a)) return rc;
    if (int rc = enter(ctx, true)) return rc;
    return spike_run(ctx, call, a, i, o);
}

// the host-pointer form of either entry point
int spike_host(xb_ctx *ctx, const SpikeCall &call, const SpikeArgs &a, const SpikeIn &h, const SpikeOut &ho)
{
    if (!ctx) return XB_ERR_INVALID;
    if (!spike_complete(h, ho)) return fail(ctx, XB_ERR_INVALID, "%s: null host pointer", call.who);
    if (int rc = spike_check(ctx, call.who, a)) return rc;
    const int n = a.n, N = a.N, Lt = a.Lt;
    for (int c = 0; c < n; ++c) {                                       // what the kernel would otherwise clamp
        const int len = h.lengths[c];
        if (len < 0 || len > Lt) return fail(ctx, XB_ERR_INVALID, "%s: chunk %d has %d labels in a row of %d", call.who, c, len, Lt);
        const uint16_t *b = h.bkps + (size_t)c * Lt;
        for (int l = 0; l < len; ++l)
            if (b[l] > N || (l && b[l] < b[l - 1]))
                return fail(ctx, XB_ERR_INVALID, "%s: chunk %d: breakpoint %d of base %d (the one before: %d, samples: %d)", call.who, c,
                            (int)b[l], l, l ? (int)b[l - 1] : 0, N);
    }
    if (int rc = enter(ctx, false)) return rc;
    const size_t C = (size_t)n;
    Staging st{ctx};
    const auto d_sig = st.take<float>(C * N), d_out = st.take<float>(C * N);
    const auto d_med = st.take<double>(C), d_mad = st.take<double>(C);
    const auto d_cnt = st.take<int32_t>(C), d_len = st.take<int32_t>(C);
    const auto d_bk = st.take<uint16_t>(C * Lt);
    const auto d_t = st.take<uint8_t>(C * Lt), d_ot = st.take<uint8_t>(C * Lt);
    const auto d_st = st.take<int8_t>(C);
    if (st.used > ((size_t)2 << 30)) return fail(ctx, XB_ERR_INVALID, "%s: %d chunks of %d samples in one call; split the batch", call.who, n, N);
    if (int rc = st.ready()) return rc;
    XB_HIP(ctx, hipMemcpyAsync(d_sig, h.signal, C * N * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_len, h.lengths, C * 4, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_bk, h.bkps, C * Lt * 2, hipMemcpyHostToDevice, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(d_t, h.targets, C * Lt, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = spike_run(ctx, call, a, {d_sig, d_t, d_len, d_bk}, {d_out, d_ot, d_cnt, d_med, d_mad, d_st})) return rc;
    XB_HIP(ctx, hipMemcpyAsync(ho.signal, d_out, C * N * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ho.targets, d_ot, C * Lt, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ho.spiked, d_cnt, C * 4, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ho.med, d_med, C * 8, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ho.mad, d_mad, C * 8, hipMemcpyDeviceToHost, ctx->stream));
    XB_HIP(ctx, hipMemcpyAsync(ho.status, d_st, C, hipMemcpyDeviceToHost, ctx->stream));
    return xb_synchronize(ctx);
}

}  // namespace

XB_API int xb_spike_chunks_dev(xb_ctx *ctx, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
                               const uint16_t *d_breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                               double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                               int variable_noise, float *d_out_signal, uint8_t *d_out_targets, int32_t *d_spiked, double *d_med,
                               double *d_mad, int8_t *d_status)
{
    return spike_dev(ctx, SPIKE_WINDOWS, {n, N, Lt, first_index, seed, ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std, variable_noise},
                     {d_signal, d_targets, d_lengths, d_breakpoints}, {d_out_signal, d_out_targets, d_spiked, d_med, d_mad, d_status});
}

XB_API int xb_spike_chunks(xb_ctx *ctx, const float *signal, const uint8_t *targets, const int32_t *lengths,
                           const uint16_t *breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                           double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                           int variable_noise, float *out_signal, uint8_t *out_targets, int32_t *spiked, double *med, double *mad,
                           int8_t *status)
{
    return spike_host(ctx, SPIKE_WINDOWS, {n, N, Lt, first_index, seed, ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std, variable_noise},
                      {signal, targets, lengths, breakpoints}, {out_signal, out_targets, spiked, med, mad, status});
}

// ---- XNA fully synthetic chunks (xb_synth_chunks): xb_spike_chunks' arguments, model and checks, the whole chunk synthesised
XB_API int xb_synth_chunks_dev(xb_ctx *ctx, const float *d_signal, const uint8_t *d_targets, const int32_t *d_lengths,
                               const uint16_t *d_breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                               double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                               int variable_noise, float *d_out_signal, uint8_t *d_out_targets, int32_t *d_spiked, double *d_med,
                               double *d_mad, int8_t *d_status)
{
    return spike_dev(ctx, SPIKE_WHOLE, {n, N, Lt, first_index, seed, ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std, variable_noise},
                     {d_signal, d_targets, d_lengths, d_breakpoints}, {d_out_signal, d_out_targets, d_spiked, d_med, d_mad, d_status});
}

XB_API int xb_synth_chunks(xb_ctx *ctx, const float *signal, const uint8_t *targets, const int32_t *lengths,
                           const uint16_t *breakpoints, int n, int N, int Lt, int64_t first_index, uint64_t seed, int ubs_mask,
                           double prop, double var_prop, int pad, int dist_rows, const double *phi, double noise_std,
                           int variable_noise, float *out_signal, uint8_t *out_targets, int32_t *spiked, double *med, double *mad,
                           int8_t *status)
{
    return spike_host(ctx, SPIKE_WHOLE, {n, N, Lt, first_index, seed, ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std, variable_noise},
                      {signal, targets, lengths, breakpoints}, {out_signal, out_targets, spiked, med, mad, status});
}

}  // extern "C"
