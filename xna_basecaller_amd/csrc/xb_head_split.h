// xb_head_split.h -- how xb_head_grad divides its reduction dW = dZ^T X over workgroups and launches: the M rows are cut into
// slabs of whole k-tiles (HEAD_KT rows), every slab's partial sums lie in a workspace of the context that one launch may own
// only XB_HEAD_SCRATCH_MB megabytes of, and a call whose partial sums do not fit is split over its output rows (blocks of
// HEAD_TO score columns), slabs unchanged, so that the order of every sum -- and with it every byte -- stays what it was.
// No HIP, no context: checked on its own (tools/head_split_check.cpp).
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace xb {

constexpr int HEAD_KT = 32;            // rows of one k-tile (the MFMA's K)
constexpr int HEAD_TO = 64;            // score columns (rows of dW) of one workgroup tile
constexpr int HEAD_TF = 128;           // features (columns of dW) of one workgroup tile
constexpr int HEAD_MIN_STEPS = 8;      // k-tiles a slab holds at least: below 256 rows a further slab costs more than it spreads
constexpr int HEAD_WGS_PER_CU = 8;     // workgroups per CU the slab count aims at
constexpr long HEAD_SCRATCH_DEFAULT_MB = 256, HEAD_SCRATCH_MAX_MB = 65536;

// the byte bound from the environment's text (null: the default), clamped to [1, HEAD_SCRATCH_MAX_MB] MB
inline size_t head_scratch_bound(const char *env)
{
    long mb = env ? atol(env) : HEAD_SCRATCH_DEFAULT_MB;
    if (mb < 1) mb = 1;
    if (mb > HEAD_SCRATCH_MAX_MB) mb = HEAD_SCRATCH_MAX_MB;
    return (size_t)mb << 20;
}

struct HeadPlan {
    int error;                 // 1: a single slab of a single block of rows exceeds the bound (F too wide for it), nothing else set
    long ksteps;               // k-tiles of the call: ceil(M / HEAD_KT)
    int nslabs;                // slabs of the reduction, each of whole k-tiles, none empty
    int o_tiles, f_tiles;      // workgroup tiles of the output
    int o_tiles_per_launch;    // blocks of HEAD_TO output rows one launch serves (the last launch may serve fewer)
    int launches;
    size_t row_bytes;          // workspace of one slab of one block of output rows: HEAD_TO x (F floats + one double)
    size_t bytes;              // workspace of one launch = o_tiles_per_launch * nslabs * row_bytes <= bound
    bool order_kept;           // the slabs are those an unbounded workspace would give: the bound only split the call

    // slab s = k-tiles [step_begin(s), step_begin(s + 1)), rows [row_begin(s), row_begin(s + 1)) clipped to M
    long step_begin(int s) const { return ksteps * (long)s / nslabs; }
    long row_begin(int s, long M) const { const long r = step_begin(s) * HEAD_KT; return r < M ? r : M; }
};

inline HeadPlan head_plan(long M, int O, int F, int cu_count, size_t bound)
{
    HeadPlan p{};
    p.ksteps = (M + HEAD_KT - 1) / HEAD_KT;
    p.o_tiles = (O + HEAD_TO - 1) / HEAD_TO;
    p.f_tiles = (F + HEAD_TF - 1) / HEAD_TF;
    p.row_bytes = (size_t)HEAD_TO * ((size_t)F * sizeof(float) + sizeof(double));
    if (p.row_bytes > bound) { p.error = 1; return p; }
    const long tiles = (long)p.o_tiles * p.f_tiles;
    long want = ((long)HEAD_WGS_PER_CU * cu_count + tiles - 1) / tiles;
    const long most = (p.ksteps + HEAD_MIN_STEPS - 1) / HEAD_MIN_STEPS;
    if (want > most) want = most;
    if (want < 1) want = 1;
    const size_t fit = bound / p.row_bytes;            // (slab, block of rows) pairs the bound holds, >= 1
    p.order_kept = (size_t)want <= fit;
    p.nslabs = p.order_kept ? (int)want : (int)fit;
    size_t per = fit / (size_t)p.nslabs;
    if (per > (size_t)p.o_tiles) per = (size_t)p.o_tiles;
    p.o_tiles_per_launch = (int)per;
    p.launches = (p.o_tiles + p.o_tiles_per_launch - 1) / p.o_tiles_per_launch;
    p.bytes = (size_t)p.o_tiles_per_launch * (size_t)p.nslabs * p.row_bytes;
    return p;
}

}  // namespace xb
