// xb_conv_plan.h -- the layouts of the convolutions' training (xb_conv_train.hip, and the trainer of every layer in xb_top.hip:
// xb_full_train_begin): which of the two routes a convolution takes, what the routes keep in the context's workspaces, where the
// six conv tensors lie in front of the trainer's flat parameter buffers, and where a step of n chunks keeps the conv stack's
// activations.  The conv stack is rnn_encoder's: Conv1d(1, 4, 5), Conv1d(4, 16, 5), Conv1d(16, F, W, stride S), each with
// padding K / 2, a bias and swish.  Tensors in state-dict order: encoder.0.conv.weight (4, 1, 5), .bias (4), encoder.1.conv.weight
// (16, 4, 5), .bias (16), encoder.2.conv.weight (F, 16, W), .bias (F) -- 360 + F (16 W + 1) floats, then the 4 * 5 + 2 tensors of
// xb_top_plan.h.  The activations of a step, per chunk of L samples: z1 4 L1 | y1 4 L1 | z2 16 L2 | y2 16 L2 | col T 16 W |
// z3 T F | dy2 16 L2 (conv3's dx) | dy1 4 L1 (conv2's dx); y3 is the x0 of xb_top_plan.h.  Every piece starts on a 16-byte
// boundary.  No HIP, no context: checked on its own (tools/conv_plan_check.cpp).
#pragma once
#include <stddef.h>

namespace xb {

// Lout of Conv1d(K, stride, padding = K / 2) on Lin >= 1 samples: at least 1
inline long conv_out_len(long Lin, int K, int stride) { return (Lin + 2 * (long)(K / 2) - K) / stride + 1; }

// ---- the two routes ------------------------------------------------------------------------------------------------------------
// THE RULE, which reads the shape alone: a convolution of stride 1 with at most 16 channels on either side and Cin K <= 64 takes
// the narrow route (direct kernels: a workgroup stages its x tile, halo and all weights in LDS; conv1 and conv2), every other
// one the wide route (im2col and the fp32 products of xb_train_gemm.hip; conv3).  Cin K <= 4096 either way.
constexpr int CONV_MAX_CK = 4096;
constexpr int CONV_NARROW_MAX_C = 16, CONV_NARROW_MAX_CK = 64;
constexpr int CONV_TILE = 256;                       // positions of one narrow workgroup, one a thread

inline bool conv_is_narrow(int Cin, int Cout, int K, int stride)
{
    return stride == 1 && Cin <= CONV_NARROW_MAX_C && Cout <= CONV_NARROW_MAX_C && (long)Cin * K <= CONV_NARROW_MAX_CK;
}

// narrow backward: one workgroup per chunk and tile of CONV_TILE positions of max(Lin, Lout); each writes one float64 partial of
// every dw and db element (`outputs` of them) to scratch, and a second kernel adds the workgroups' partials in ascending order
struct ConvNarrow {
    size_t tiles, blocks, outputs, scratch_doubles;
};
inline ConvNarrow conv_narrow(int n, int Cin, long Lin, int Cout, int K)
{
    ConvNarrow c{};
    const long Lout = conv_out_len(Lin, K, 1), P = Lin > Lout ? Lin : Lout;
    c.tiles = (size_t)((P + CONV_TILE - 1) / CONV_TILE);
    c.blocks = c.tiles * (size_t)n;
    c.outputs = (size_t)Cout * Cin * K + (size_t)Cout;
    c.scratch_doubles = c.blocks * c.outputs;
    return c;
}

// wide: the workspace of one call in floats, rows = Lout n (row t n + b), CK = Cin K: dz (rows, Cout) -- the forward's z in
// row order before the swish lays it out -- | col (rows, CK) | dcol (rows, CK) | wt (CK, Cout); the forward uses the first two
struct ConvWide {
    size_t dz, col, dcol, wt, forward_floats, backward_floats;
};
inline size_t conv_round4(size_t v) { return (v + 3) & ~(size_t)3; }
inline ConvWide conv_wide(size_t rows, int CK, int Cout)
{
    ConvWide c{};
    c.dz = 0;
    c.col = conv_round4(rows * Cout);
    c.dcol = c.col + conv_round4(rows * CK);
    c.forward_floats = c.dcol;
    c.wt = c.dcol + conv_round4(rows * CK);
    c.backward_floats = c.wt + conv_round4((size_t)CK * Cout);
    return c;
}

// ---- the trainer of every layer --------------------------------------------------------------------------------------------------
constexpr int CONV_C1 = 4, CONV_C2 = 16, CONV_K12 = 5;
constexpr int CONV_TENSORS = 6;

struct ConvAct {                        // floats from the start of the conv activations of a step of n chunks
    size_t z1, y1, z2, y2, col, z3, dy2, dy1, floats;
};

struct ConvPlan {
    int error;                          // 1: chunk, F, W or S < 1, or 16 W > CONV_MAX_CK
    int chunk, F, W, S;
    long L1, L2, T;                     // samples a chunk has behind conv1 and conv2, time steps behind conv3
    size_t off[CONV_TENSORS];           // floats from the start of a flat buffer: w1, b1, w2, b2, w3, b3
    size_t len[CONV_TENSORS];
    size_t params;                      // 360 + F (16 W + 1): the LSTM section starts here

    ConvAct act(size_t n) const
    {
        ConvAct a{};
        size_t at = 0;
        auto piece = [&at](size_t floats) { const size_t here = at; at += conv_round4(floats); return here; };
        a.z1 = piece(n * CONV_C1 * L1); a.y1 = piece(n * CONV_C1 * L1);
        a.z2 = piece(n * CONV_C2 * L2); a.y2 = piece(n * CONV_C2 * L2);
        a.col = piece(n * T * CONV_C2 * W); a.z3 = piece(n * T * F);
        a.dy2 = piece(n * CONV_C2 * L2); a.dy1 = piece(n * CONV_C1 * L1);
        a.floats = at;
        return a;
    }
};

inline ConvPlan conv_plan(int chunk, int F, int W, int S)
{
    ConvPlan p{};
    if (chunk < 1 || F < 1 || W < 1 || S < 1 || (long)CONV_C2 * W > CONV_MAX_CK) { p.error = 1; return p; }
    p.chunk = chunk; p.F = F; p.W = W; p.S = S;
    p.L1 = conv_out_len(chunk, CONV_K12, 1);
    p.L2 = conv_out_len(p.L1, CONV_K12, 1);
    p.T = conv_out_len(p.L2, W, S);
    const size_t lens[CONV_TENSORS] = {(size_t)CONV_C1 * 1 * CONV_K12, (size_t)CONV_C1, (size_t)CONV_C2 * CONV_C1 * CONV_K12, (size_t)CONV_C2,
                                       (size_t)F * CONV_C2 * W, (size_t)F};
    size_t at = 0;
    for (int k = 0; k < CONV_TENSORS; ++k) { p.off[k] = at; p.len[k] = lens[k]; at += lens[k]; }
    p.params = at;
    return p;
}

}  // namespace xb
