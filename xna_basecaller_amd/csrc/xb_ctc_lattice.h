// xb_ctc_lattice.h -- the two pure rules of the CTC lattice kernels (xb_ctc.hip): the score columns a position of a label row
// reads, and the launch a row of a given width gets.  No HIP, no context: the kernels and their launchers use them as they
// stand, and the CPU tests reach them through xb_internal_ctc_columns / xb_internal_ctc_launch (xb_api.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define XB_CTC_RULE __host__ __device__ __forceinline__
#else
#define XB_CTC_RULE inline
#endif

namespace xb {

// one workgroup per chunk: CTC_MAX_THREADS threads at most, CTC_PMAX positions per thread at most
constexpr int CTC_MAX_THREADS = 256, CTC_PMAX = 8;
constexpr int ctc_max_positions() { return CTC_MAX_THREADS * CTC_PMAX; }

// The gather columns of prepare_ctc_scores (ub-bonito/bonito/crf/model.py:102-116) for position l of a label row: the k-mer
// state st_l = sum_i base[l + i] nb^(sl - 1 - i), base = max(label - 1, 0) (torch.clamp(targets - 1, 0)).
//   cs: the stay column st_l (nb + 1) (HB only: the blank-less layout has no stay column);
//   cm: the move column into l (l - 1 -> l): st_l (nb + 1) + base[l - 1] + 1 with the blank column, st_l nb + base[l - 1] without;
//   cp: that move column in the posteriors' (blank) layout.  Position 0 has no move into it: cm = cp = 0.
XB_CTC_RULE int ctc_base(uint8_t label)
{
    const int b = (int)label - 1;
    return b > 0 ? b : 0;
}

template <bool HB>
XB_CTC_RULE void ctc_columns(const uint8_t *lab, int l, int nb, int sl, int &cs, int &cm, int &cp)
{
    const int E = nb + 1;
    int st = 0;
    for (int i = 0; i < sl; ++i) st = st * nb + ctc_base(lab[l + i]);
    const int base = l > 0 ? ctc_base(lab[l - 1]) : 0;
    cs = st * E;
    cp = l > 0 ? st * E + base + 1 : 0;
    cm = l > 0 ? (HB ? cp : st * nb + base) : 0;
}

// One wave while the positions fit it one per lane (the barrier then costs nothing), else as many waves as give every lane
// a position, four at most: a time step is a chain of dependent instructions, and its length grows with the positions per lane.
inline int ctc_loss_threads(int positions) { return positions <= 64 ? 64 : (positions <= 128 ? 128 : CTC_MAX_THREADS); }

struct CtcLaunch {
    int threads;                 // the workgroup
    int pmax;                    // the kernels' PMAX instantiation: 1, 2, 4 or 8; 0: the row is too wide for the workgroup
    size_t lds;                  // dynamic LDS bytes
};

// The launch of a lattice kernel for label rows of `positions` positions.  override: 64, 128 or 256 threads where they hold the
// row (XB_CTC_LOSS_THREADS), anything else leaves the rule.  LDS: the double-buffered position vector [2][positions + 2]; with
// chains (ctc_grad_kernel) also g [2][2][positions] floats, next [2][positions] u16 and not-head [2][positions] u8.
inline CtcLaunch ctc_launch(int positions, int override, bool chains)
{
    int threads = ctc_loss_threads(positions);
    if ((override == 64 || override == 128 || override == 256) && override * CTC_PMAX >= positions) threads = override;
    const int per = (positions + threads - 1) / threads;
    const size_t np = (size_t)positions;
    return {threads, per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : (per <= CTC_PMAX ? CTC_PMAX : 0))),
            sizeof(float) * 2 * (np + 2) + (chains ? sizeof(float) * 4 * np + 4 * np + 2 * np : 0)};
}

}  // namespace xb
