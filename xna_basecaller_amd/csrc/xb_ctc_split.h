// xb_ctc_split.h -- how xb_ctc_loss_grad divides a call over launches of its lattice kernel: the alpha stash one launch may own
// is bounded in bytes (XB_CTC_SCRATCH_MB), a chunk's slot holds (T + 1) rows of the call's positions.  No HIP, no context:
// checked on its own (tools/ctc_split_check.cpp).
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace xb {

constexpr long CTC_SCRATCH_DEFAULT_MB = 1024, CTC_SCRATCH_MAX_MB = 65536;

// floats of one chunk's alpha stash: alpha_0 .. alpha_T over `positions` lattice positions
inline size_t ctc_grad_slot_floats(int T, int positions) { return ((size_t)T + 1) * (size_t)positions; }

// the byte bound from the environment's text (null: the default), clamped to [1, CTC_SCRATCH_MAX_MB] MB
inline size_t ctc_scratch_bound(const char *env)
{
    long mb = env ? atol(env) : CTC_SCRATCH_DEFAULT_MB;
    if (mb < 1) mb = 1;
    if (mb > CTC_SCRATCH_MAX_MB) mb = CTC_SCRATCH_MAX_MB;
    return (size_t)mb << 20;
}

// chunks per launch for a call of n chunks: as many slots as fit the bound, one at least, n at most
inline size_t ctc_grad_chunks_per_launch(int T, int positions, int n, size_t bound)
{
    const size_t fit = bound / (ctc_grad_slot_floats(T, positions) * sizeof(float));
    return fit < 1 ? 1 : (fit > (size_t)n ? (size_t)n : fit);
}

}  // namespace xb
