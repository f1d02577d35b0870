// xb_top_plan.h -- the layout of the trainer of the head and the top L LSTM layers (xb_top.hip: xb_top_train_begin .. _end): where
// each unfrozen tensor lies in the flat parameter buffers, and where a step of (T, n, F, C, L) keeps its activations.  Tensors in state-dict order: for each unfrozen LSTM layer
// encoder.(9 - L) .. encoder.8 weight_ih_l0 (4F, F), weight_hh_l0 (4F, F), bias_ih_l0 (4F), bias_hh_l0 (4F), then
// encoder.9.linear.weight (C, F) and .bias (C).  Four buffers of that layout follow one another, each starting on a 16-byte boundary: p, g, m, v.  The activations of
// a step, in floats per (t, chunk) row: x0 F | gin 4F (dy lies in its first F floats once the forward is done) | dgin 4F | per
// layer y F, gates 4F, c F | scores C | dscores C | dz C -- T n (L 6F + 9F + 3C) floats.  No HIP, no context: checked on its own
// (tools/top_plan_check.cpp).
#pragma once
#include <stddef.h>

namespace xb {

constexpr int TOP_MAX_LAYERS = 5;
constexpr int TOP_MAX_TENSORS = 4 * TOP_MAX_LAYERS + 2;

struct TopPlan {
    int error;                          // 1: L outside 1 .. 5, or F, C < 1
    int L, F, C;
    int tensors;                        // 4 L + 2
    size_t off[TOP_MAX_TENSORS];        // floats from the start of a buffer
    size_t len[TOP_MAX_TENSORS];
    size_t params;                      // floats of the tensors
    size_t stride;                      // floats from one buffer to the next (p, g, m, v): params rounded up to 16 bytes
    size_t bias_sum;                    // floats of the layers' summed biases: L * 4F
    size_t turned;                      // floats of the transposed weight of one dx product: max(4F F, C F)

    int layer_index(int i) const { return 9 - L + i; }              // encoder.N of unfrozen layer i (0 = lowest)
    int bottom_layers() const { return 5 - L; }                     // LSTM layers of the frozen bottom
    const size_t *layer(int i) const { return off + 4 * i; }        // w_ih, w_hh, b_ih, b_hh
    size_t head_w() const { return off[4 * L]; }
    size_t head_b() const { return off[4 * L + 1]; }
    size_t small_floats() const { return bias_sum + turned; }

    // the activations of a step of T x n rows, in floats from the start of the buffer
    size_t row_floats() const { return (size_t)L * 6 * F + (size_t)9 * F + (size_t)3 * C; }
    size_t act_floats(size_t rows) const { return rows * row_floats(); }
    size_t x0(size_t) const { return 0; }
    size_t gin(size_t rows) const { return rows * F; }
    size_t dy(size_t rows) const { return gin(rows); }
    size_t dgin(size_t rows) const { return rows * 5 * F; }
    size_t y(size_t rows, int i) const { return rows * ((size_t)9 * F + (size_t)i * 6 * F); }
    size_t gates(size_t rows, int i) const { return y(rows, i) + rows * F; }
    size_t c(size_t rows, int i) const { return y(rows, i) + rows * 5 * F; }
    size_t scores(size_t rows) const { return rows * ((size_t)9 * F + (size_t)L * 6 * F); }
    size_t dscores(size_t rows) const { return scores(rows) + rows * C; }
    size_t dz(size_t rows) const { return scores(rows) + rows * 2 * C; }
    // bytes a step needs on the device beside the context's own workspaces
    size_t step_bytes(size_t rows) const { return sizeof(float) * (act_floats(rows) + 4 * stride + small_floats()); }
};

inline TopPlan top_plan(int L, int F, int C)
{
    TopPlan p{};
    if (L < 1 || L > TOP_MAX_LAYERS || F < 1 || C < 1) { p.error = 1; return p; }
    p.L = L; p.F = F; p.C = C; p.tensors = 4 * L + 2;
    size_t at = 0;
    int k = 0;
    for (int i = 0; i < L; ++i)
        for (size_t len : {(size_t)4 * F * F, (size_t)4 * F * F, (size_t)4 * F, (size_t)4 * F}) {
            p.off[k] = at; p.len[k] = len; at += len; ++k;
        }
    p.off[k] = at; p.len[k] = (size_t)C * F; at += p.len[k]; ++k;
    p.off[k] = at; p.len[k] = (size_t)C; at += p.len[k]; ++k;
    p.params = at;
    p.stride = (at + 3) & ~(size_t)3;
    p.bias_sum = (size_t)L * 4 * F;
    const size_t a = (size_t)4 * F * F, b = (size_t)C * F;
    p.turned = a > b ? a : b;
    return p;
}

}  // namespace xb
